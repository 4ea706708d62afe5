#!/usr/bin/env python3
"""Generate the fixtures of DiffAugment(policy, p < 1) from the REFERENCE's own module (utils/diff_augment.py, imported by path as
make_golden.py does).  Runs only where the reference's sources are at hand; the vectors are data, no reference source travels.

1. aug_gate_8x16.npz and aug_gate_32x64_<policy>_p<i>.npz: `DiffAugment(policy, p)(x)` and its autograd input gradient for
   p in {0, 0.3, 0.7, 1}, the full policy and `translation,cutout` alone, B = 64, with the draws captured by replaying torch's
   generator.  A gated-off stage is recorded the way the kernels take it: t_h[b] = OFF (translation), o_x[b] = OFF (cutout).
   x and the upstream gradient are multiples of 1/8 and 1/4 in [-1, 1], the range of the images DiffAugment sees: the module's
   fp32 roundings (ulp 2.4e-7 below 4) then stay inside the 1e-6 the test allows, and the gradient sums of `translation,cutout`,
   which only moves values, are exact.  The seed of
   a case is the first from SEED0 upward at which - for p = 0.3 and 0.7 - each of the four gate states occurs at least twice.
2. step_none_augp.npz, step_dusty2_augp.npz: make_golden.make_step_golden (the reference's modules under the restated
   Trainer.step) with DiffAugment(p = 0.5): 32x64, B = 4, two steps, fp32.  The seed is the first from STEP_SEED0 upward at which
   every A(.) call of every step holds at least two gate states and the G phase's fake sets (aug3) hold all four over the fixture.

usage:  python tests/golden/make_aug_gate_golden.py [ops | steps]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (puts the reference on sys.path; loads its utils/diff_augment.py by path)

OFF = -2 ** 31
PS = (0.0, 0.3, 0.7, 1.0)
POLICIES = {"full": ["brightness", "saturation", "contrast", "translation", "cutout"], "tc": ["translation", "cutout"]}
SHAPES = ((8, 16), (32, 64))
B_OPS = 64
SEED0, STEP_SEED0 = 100, 40
STEP_P = 0.5


def capture_aug_p(B, H, W, policy, p):
    """make_golden.capture_aug for any p: the same draws in the same order, the Bernoulli draws with the module's p.  The colour
    stages' Bernoulli draw is overwritten by their uniform draw (one tensor); translation's and cutout's is their gate."""
    rp = {}
    for s in policy:
        if s in ("brightness", "saturation", "contrast"):
            f = torch.empty((B, 1, 1, 1))
            f.bernoulli_(p=p)
            f.uniform_(-1, 1)
            rp[{"brightness": "u_b", "saturation": "u_s", "contrast": "u_c"}[s]] = f.flatten().clone()
        elif s == "translation":
            sh, sw = int(H * (1 / 8) / 2 + 0.5), int(W * (1 / 8) / 2 + 0.5)
            rp["t_h"] = torch.randint(-sh, sh + 1, size=[B, 1, 1]).flatten()
            rp["t_w"] = torch.randint(-sw, sw + 1, size=[B, 1, 1]).flatten()
            rp["t_h"][~torch.empty(B).bernoulli_(p=p).bool()] = OFF
        elif s == "cutout":
            ch, cw = int(H * 0.5 + 0.5), int(W * 0.5 + 0.5)
            rp["o_x"] = torch.randint(0, H + (1 - ch % 2), size=[B, 1, 1]).flatten()
            rp["o_y"] = torch.randint(0, W + (1 - cw % 2), size=[B, 1, 1]).flatten()
            rp["o_x"][~torch.empty(B).bernoulli_(p=p).bool()] = OFF
    return rp


def states(rp):
    return (rp["t_h"] != OFF).long() + 2 * (rp["o_x"] != OFF).long()


def ops_case(H, W, tag, p, seed):
    torch.manual_seed(seed)
    x = (torch.randint(-8, 9, (B_OPS, 1, H, W)).float() / 8).requires_grad_()
    gy = torch.randint(-4, 5, (B_OPS, 1, H, W)).float() / 4
    A = mg.diff_augment.DiffAugment(policy=POLICIES[tag], p=p)
    y, rp = mg.run_and_capture(lambda: A(x), lambda: capture_aug_p(B_OPS, H, W, POLICIES[tag], p))
    (gx,) = torch.autograd.grad(y, x, gy)
    d = {"x": x.detach().numpy(), "gy": gy.numpy(), "y": y.detach().numpy(), "gx": gx.numpy(), "p": np.array(p),
         "seed": np.array(seed), "policy": np.array(",".join(POLICIES[tag]))}
    for k, v in rp.items():
        d["rp/" + k] = v.numpy()
    return d, rp


def make_ops():
    for H, W in SHAPES:
        small = {}
        for tag in POLICIES:
            seed = SEED0
            while True:   # one seed per (shape, policy): the first at which p = 0.3 and p = 0.7 both show every state twice
                ok = all(int(torch.bincount(states(ops_case(H, W, tag, p, seed)[1]), minlength=4).min()) >= 2 for p in (0.3, 0.7))
                if ok:
                    break
                seed += 1
            for i, p in enumerate(PS):
                d, rp = ops_case(H, W, tag, p, seed)
                cnt = torch.bincount(states(rp), minlength=4).tolist()
                print(f"{H}x{W} {tag} p={p} seed={seed}: gate states (none, t, c, both) = {cnt}")
                assert (p not in (0.3, 0.7)) or min(cnt) >= 2
                assert p != 1.0 or cnt == [0, 0, 0, B_OPS]
                assert p != 0.0 or cnt == [B_OPS, 0, 0, 0]
                if (H, W) == SHAPES[0]:
                    small.update({f"{tag}/p{i}/{k}": v for k, v in d.items()})
                else:
                    path = os.path.join(HERE, f"aug_gate_{H}x{W}_{tag}_p{i}.npz")
                    np.savez_compressed(path, **d)
                    print("wrote", path, f"{os.path.getsize(path) / 1024:.0f} KiB")
        if small:
            path = os.path.join(HERE, f"aug_gate_{H}x{W}.npz")
            np.savez_compressed(path, **small)
            print("wrote", path, f"{os.path.getsize(path) / 1024:.0f} KiB")


class _RefP(mg.diff_augment.DiffAugment):
    def __init__(self, policy=None):
        super().__init__(policy=policy, p=STEP_P)


def step_ok(name):
    g = np.load(os.path.join(HERE, f"step_{name}.npz"))
    steps, fake = int(g["meta/steps"]), []
    for it in range(steps):
        for j in range(4):
            st = (g[f"s{it}/aug{j}/t_h"] != OFF).astype(int) + 2 * (g[f"s{it}/aug{j}/o_x"] != OFF).astype(int)
            if len(set(st.tolist())) < 2:
                return False
            if j == 3:
                fake += st.tolist()
    return set(fake) == {0, 1, 2, 3}


def make_steps():
    torch.set_num_threads(4)
    ref_cls, ref_cap = mg.diff_augment.DiffAugment, mg.capture_aug
    mg.diff_augment.DiffAugment = _RefP
    mg.capture_aug = lambda B, H, W, policy: capture_aug_p(B, H, W, policy, STEP_P)
    try:
        for name, arch in (("none_augp", "none"), ("dusty2_augp", "dusty2")):
            seed = STEP_SEED0
            while True:
                mg.make_step_golden(name, arch, True, seed=seed, B=4)
                if step_ok(name):
                    break
                print(f"{name}: seed {seed} rejected")
                seed += 1
            path = os.path.join(HERE, f"step_{name}.npz")
            data = dict(np.load(path))
            data["meta/seed"], data["meta/augment_p"] = np.array(seed), np.array(STEP_P)
            np.savez_compressed(path, **data)
            print(f"{name}: seed {seed}", f"{os.path.getsize(path) / 1024:.0f} KiB")
    finally:
        mg.diff_augment.DiffAugment, mg.capture_aug = ref_cls, ref_cap


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what in ("all", "ops"):
        make_ops()
    if what in ("all", "steps"):
        make_steps()
