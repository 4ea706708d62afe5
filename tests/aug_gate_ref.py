"""DiffAugment(policy, p < 1) restated in float64 (no GPU): the reference's per-sample gate (utils/diff_augment.py:77-78, 99-100:
`mask = empty(B).bernoulli_(p)`, `y[~mask] = x[~mask]`) composed from the per-policy functions of tests/image_exact_util.py.

A gated-off stage for sample b IS "this stage is not in the policy, for sample b": the samples are grouped by gate state (translation
on / off, cutout on / off), each group runs the per-policy function of the policy that is left, and the results are put back in
place.  Only translation and cutout have a gate: the colour stages form `factor.bernoulli_(p) * factor.uniform_(-1, 1)` on ONE
tensor, the Bernoulli draw is overwritten and the factor is u * u whatever p is.

A parameter set marks a gated-off stage the way the kernels take it (include/dusty_gan_hip.h): t_h[b] == OFF switches the
translation off for sample b (t_w[b] is ignored), o_x[b] == OFF the cutout (o_y[b] is ignored).

Defect switches (tests/test_aug_gate_cpu.py shows that the reference's fixture rejects each):
    gate_colour   the colour stages are gated too (by the translation gate)
    zero_shift    "off" as a translation by (0, 0): not the identity - the wrap modulo W - 1 folds column W - 1 onto column 0
    shared_gate   one gate for both stages (the translation's)
"""
from unittest import mock

import torch

from tests import image_exact_util as U

OFF = -2 ** 31
COLOUR = ("brightness", "saturation", "contrast")
DEFECTS = ("gate_colour", "zero_shift", "shared_gate")


def gates(rp):
    """(translation on [B], cutout on [B]) bool; a parameter set without a stage's arrays has that stage on (the policy decides)"""
    B = next(iter(rp.values())).shape[0]
    on = torch.ones(B, dtype=torch.bool)
    return (torch.as_tensor(rp["t_h"]) != OFF if "t_h" in rp else on), (torch.as_tensor(rp["o_x"]) != OFF if "o_x" in rp else on)


def with_gates(rp, g_t, g_c):
    """rp with the sentinel written where a gate is off (the ignored partner array keeps its value)"""
    out = {k: torch.as_tensor(v).clone() for k, v in rp.items()}
    out["t_h"][~g_t] = OFF
    out["o_x"][~g_c] = OFF
    return out


def gate_state(rp):
    """[B] in {0, 1, 2, 3}: translation on + 2 cutout on"""
    g_t, g_c = gates(rp)
    return g_t.long() + 2 * g_c.long()


def _call(fn, t, rp, policy):
    """fn(t, rp, <name of `policy`>): image_exact_util's per-policy functions take the NAME of a policy in its POLICIES table.  A
    policy the table does not list is filed there under a name of this file's for the duration of the call only (patch.dict puts
    the table back): that helper's shared state is what it was before and after."""
    policy = tuple(policy)
    for k, v in U.POLICIES.items():
        if tuple(v) == policy:
            return fn(t, rp, k)
    name = "gate:" + ",".join(policy)
    with mock.patch.dict(U.POLICIES, {name: policy}):
        return fn(t, rp, name)


def _groups(rp, policy, defect):
    """[(sample indices, the policy those samples run, their parameters with every sentinel replaced by a drawable 0)]"""
    policy = tuple(policy)
    g_t, g_c = gates(rp)
    if defect == "shared_gate":
        g_c = g_t.clone()
    clean = {k: torch.as_tensor(v).clone() for k, v in rp.items()}
    for k in ("t_h", "t_w"):
        if k in clean:
            clean[k][~g_t] = 0
    for k in ("o_x", "o_y"):
        if k in clean:
            clean[k][~g_c] = 0
    for k in ("u_b", "u_s", "u_c"):          # (a policy without colour stages draws none; the per-policy functions read them)
        clean.setdefault(k, torch.zeros(g_t.shape[0], dtype=torch.float64))
    out = []
    for t_on in (True, False):
        for c_on in (True, False):
            idx = ((g_t == t_on) & (g_c == c_on)).nonzero().flatten()
            if idx.numel() == 0:
                continue
            drop = set()
            if not t_on and defect != "zero_shift":
                drop.add("translation")
            if not c_on:
                drop.add("cutout")
            if not t_on and defect == "gate_colour":
                drop.update(COLOUR)
            out.append((idx, tuple(s for s in policy if s not in drop), {k: v[idx] for k, v in clean.items()}))
    return out


def _compose(fn, t, rp, policy, defect):
    out = torch.empty_like(t)
    for idx, pol, sub in _groups(rp, policy, defect):
        out[idx] = _call(fn, t[idx], sub, pol)
    return out


def fwd(x, rp, policy, defect=None):
    """A(x) [B,1,H,W] float64 with the gates of rp (image_exact_util.aug_fwd_r per gate state)"""
    return _compose(U.aug_fwd_r, x, rp, policy, defect)


def fwd_oracle(x, rp, policy):
    """the same from the oracle's map (image_exact_util.aug64) per gate state"""
    return _compose(U.aug64, x, rp, policy, None)


def adj(e, rp, policy, defect=None):
    """A^T(e) [B,1,H,W] float64 (image_exact_util.aug_adj_r per gate state)"""
    return _compose(U.aug_adj_r, e, rp, policy, defect)


def adj_oracle(e, rp, policy):
    """autograd of the oracle's map per gate state"""
    return _compose(U.aug_adj64, e, rp, policy, None)


def window_sum(e, rp, policy, defect=None):
    """[B]: the sum of e over the pixels of the augmented image that come from the source image - the contrast pivot's gradient"""
    out = torch.empty(e.shape[0], dtype=e.dtype)
    for idx, pol, sub in _groups(rp, policy, defect):
        out[idx] = _call(U.window_sum_r, e[idx], sub, pol)
    return out


def interleaved(rp):
    """every parameter set of rp under each of the four gate states, as ONE batch of 4 B samples in which neighbours differ in
    gate state: sample 4 i + k is draw i in state (k + i) % 4 (so that a state does not always sit at the same index mod 4)"""
    B = rp["t_h"].shape[0]
    i = torch.arange(4 * B)
    src, state = i // 4, (i % 4 + i // 4) % 4
    out = {k: torch.as_tensor(v)[src].clone() for k, v in rp.items()}
    return with_gates(out, (state & 1).bool(), (state & 2).bool())


# ---- the exact-data cases of tests/test_gpu_aug_gate_exact.py (image_exact_util's data and preconditions, with gates) --------------
class GateAug:
    """image_exact_util.Aug with gates: at H x W, every draw of `all_draws` (or `some_draws`) under each of the four gate states as
    one interleaved batch; integer image x and upstream e [B,1,H,W]; the references are this file's restatement.  which = 1: the
    second source set of the fused forward (other images, the batch reversed)."""

    def __init__(self, H, W, draws, which=0):
        import functools
        g = U.X.gen(91009 + 4099 * H + W + 1000003 * which)
        self.H, self.W = H, W
        base = U.all_draws(H, W) if draws == "all" else U.some_draws(H, W, U.X.gen(5 + H + W))
        rp = interleaved(U.with_factors(base))
        if which:
            rp = {k: v.flip(0).contiguous() for k, v in rp.items()}
        self.rp, self.B = rp, rp["t_h"].shape[0]
        self.x = U.images((self.B, 1, H, W), g)
        self.e = U.gradients((self.B, 1, H, W), g)
        self.xsum = self.x.sum(dim=[1, 2, 3])
        self.y = functools.lru_cache(maxsize=None)(self._y)
        self.gx = functools.lru_cache(maxsize=None)(self._gx)
        self.gsum = functools.lru_cache(maxsize=None)(self._gsum)

    def upstream(self, of="e"):
        return self.e if of == "e" else U.blur(self.H, self.W, self.B).adj(True)

    def _y(self, policy):
        return fwd(self.x, self.rp, U.POLICIES[policy])

    def _gx(self, policy, of="e"):
        return adj(self.upstream(of), self.rp, U.POLICIES[policy])

    def _gsum(self, policy, of="e"):
        return window_sum(self.upstream(of), self.rp, U.POLICIES[policy])

    def fused(self, policy, ring):
        return U.blur64(self.y(policy), ring)


_GATE_AUG = {}


def gate_aug(H, W, draws, which=0):
    key = (H, W, draws, which)
    if key not in _GATE_AUG:
        _GATE_AUG[key] = GateAug(H, W, draws, which)
    return _GATE_AUG[key]


# 8 x 16: every draw x every gate state (1377 x 4).  2 x 8 and 5 x 7: the smallest shapes a kernel takes (5 x 7: the scalar forms,
# an odd box).  4 x 2048: a second trip of every 256-thread loop.  16 x 64: several bands and blocks per sample.
GATE_AUG = [(8, 16, "all"), (2, 8, "some"), (5, 7, "some"), (4, 2048, "some"), (16, 64, "some")]
GATE_FUSED = [(8, 16, "all"), (4, 2048, "some"), (16, 64, "some")]          # W % 4 == 0 and H % 4 == 0
GATE_AUGSUM = [(8, 16, "all"), (2, 8, "some"), (4, 2048, "some"), (16, 64, "some")]   # W % 4 == 0, W >= 8, H >= 2
GATE_HEAD = [(8, 16, "all"), (4, 2048, "some"), (16, 64, "some")]   # 4 x 2048: several blocks per sample, a second loop trip


def assert_gate_inputs(H, W, draws):
    """the premise of `bit for bit` for a gated case, as image_exact_util.assert_exact_inputs states it: the sums are exact in any
    order (also through the arena's fixed point) and every reference and intermediate is an fp32 number"""
    a = gate_aug(H, W, draws)
    what = f"gate {H}x{W} {draws}"
    U._sum_ok(a.x, what + " xsum")
    U._sum_ok(a.e, what + " gsum (any window: a subset of the terms)")
    HW = float(H * W)
    for policy in U.policies_for(H, W):
        P = U.POLICIES[policy]
        ub, uc = a.rp["u_b"].view(-1, 1, 1, 1), a.rp["u_c"].view(-1, 1, 1, 1)
        br = 0.5 * ub * ub if "brightness" in P else torch.zeros_like(ub)
        cc = 1 + 0.5 * uc * uc if "contrast" in P else torch.ones_like(uc)
        steps = [br, cc, a.x + br, a.y(policy)]
        if "contrast" in P:
            assert U.is_pow2(H * W) and H * W <= 2 ** 13, what
            mean = a.xsum.view(-1, 1, 1, 1) / HW + br
            steps += [a.xsum / HW, mean, (a.x + br) - mean, cc * ((a.x + br) - mean)]
        for t in steps:
            U._f32(t, what + " " + policy + " forward")
        gsum, gx = a.gsum(policy), a.gx(policy)
        gm = (1 - cc.view(-1)) * gsum / HW
        g2 = (gx - gm.view(-1, 1, 1, 1)) / cc
        for t in (gsum, (1 - cc.view(-1)) * gsum, gm, g2, cc * g2, gx, U.S_DEPTH * gx):
            U._f32(t, what + " " + policy + " adjoint")
