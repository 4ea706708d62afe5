#!/usr/bin/env python3
"""Generate step_dusty1_ltau.npz / step_dusty2_ltau.npz: `make_golden.make_step_golden` (the reference's own modules under
the restated Trainer.step) with `model.gen.tau: null`, i.e. a learnable Gumbel temperature (models/dusty.py:25-26, 38-43:
inverse_tau = softplus(weight) + 1 / tau_max, one scalar weight per GumbelSigmoid).  Defaults: 32x64, B = 2, two steps, fp32.

Besides what every step fixture holds, each step records per temperature weight the MAGNITUDE of what its gradient sums:
    s{it}/grad_G_mag/<name> = A = sigmoid(w) * sum |g_out * s (1 - s) * l|
(g_out the upstream of the soft mask, s the soft mask, l the noisy logit; the gradient itself is sigmoid(w) * the signed sum).
The sum cancels 20- to 50-fold, so a test bounds the gradient's error by 1e-3 * A (rel-L2's normalisation: the error over the
magnitude of what was summed).  A seed is accepted only if every recorded step has |grad| >= 0.01 * A: a wrong constant
factor of 2 then misses that bound ten times over.

Seeds: the first from 31 upward that meets the condition (dusty1), 32 for dusty2.  Ratios |grad| / A obtained:
    dusty1, seed 31: 0.0205, 0.0033 - rejected (step 1)
    dusty1, seed 32: 0.0173, 0.0247
    dusty2, seed 32: pixel 0.0605, 0.0231; image 0.0550, 0.0524
(RATIOS below holds the same figures: rewrite both from the generator's output when the fixtures are regenerated.)

usage:  python tests/golden/make_learnable_tau_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (puts the reference on sys.path and imports its `models`)
from models import dusty as ref_dusty  # noqa: E402

# |grad| / A per fixture, weight and step, as obtained when the committed fixtures were written
RATIOS = {
    "dusty1_ltau (seed 32)": {"gumbel.weight": (0.0173, 0.0247)},
    "dusty2_ltau (seed 32)": {"gumbel_pixel.weight": (0.0605, 0.0231), "gumbel_image.weight": (0.0550, 0.0524)},
}
MIN_RATIO = 0.01

_base_cfg = mg.make_cfg


def make_cfg_ltau(*a, **kw):
    cfg = _base_cfg(*a, **kw)
    cfg.model.gen["tau"] = None
    return cfg


_records = []   # (pixelwise, A) in firing order: one per GumbelSigmoid and backward pass


def _hooked(self, logits):
    assert self.tau is None
    inverse_tau = torch.nn.functional.softplus(self.weight) + 1.0 / self.tau_max
    out = torch.sigmoid(logits * inverse_tau)
    if out.requires_grad:
        def hook(g, s=out.detach(), l=logits.detach(), w=self.weight.detach(), px=self.pixelwise):
            terms = g.double() * s.double() * (1 - s.double()) * l.double()
            _records.append((px, float(torch.sigmoid(w.double()) * terms.abs().sum())))
        out.register_hook(hook)
    return out


WEIGHTS = {"dusty1": {True: "gumbel.weight"}, "dusty2": {True: "gumbel_pixel.weight", False: "gumbel_image.weight"}}


def make(name, arch, seed, **kw):
    """write step_<name>.npz; returns {weight: [|grad| / A per step]}"""
    del _records[:]
    mg.make_cfg = make_cfg_ltau
    ref_dusty.GumbelSigmoid.sigmoid_with_temperature = _hooked
    mg.make_step_golden(name, arch, True, seed=seed, **kw)
    path = os.path.join(HERE, f"step_{name}.npz")
    data = dict(np.load(path))
    steps = int(data["meta/steps"])
    per = {}
    for px, A in _records:
        per.setdefault(WEIGHTS[arch][px], []).append(A)
    ratios = {}
    for wname, mags in per.items():
        assert len(mags) == steps, (wname, len(mags))
        for it, A in enumerate(mags):
            data[f"s{it}/grad_G_mag/{wname}"] = np.array(A, dtype=np.float64)
            ratios.setdefault(wname, []).append(abs(float(data[f"s{it}/grad_G/{wname}"])) / A)
    data["meta/seed"] = np.array(seed)
    np.savez_compressed(path, **data)
    return ratios


def main():
    torch.set_num_threads(4)
    seed = 31
    while True:
        r = make("dusty1_ltau", "dusty1", seed)
        print("dusty1 seed", seed, r)
        if all(v >= MIN_RATIO for vs in r.values() for v in vs):
            break
        seed += 1
    r = make("dusty2_ltau", "dusty2", 32)
    print("dusty2 seed 32", r)
    for wname, vs in r.items():
        for it, v in enumerate(vs):
            assert v >= MIN_RATIO, ("dusty2_ltau", wname, it, v)
    for n in ("dusty1_ltau", "dusty2_ltau"):
        p = os.path.join(HERE, f"step_{n}.npz")
        print(p, f"{os.path.getsize(p) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
