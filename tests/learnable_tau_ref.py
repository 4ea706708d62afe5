"""The head post-processing with a LEARNABLE Gumbel temperature (csrc/head_post.h head_px_fwd_lt / head_px_bwd_lt, the `_lt` entry
points of csrc/head_post.hip) in float64, with the per-element criteria the kernels are held to - the companion of
tests/net_end_ref.py, whose units, borrowed figures (EXP_ULPS, RCP_ULPS, LOG1P_ULPS), input makers and product / sum rules it uses.
Imports no GPU and nothing of the project.  tests/test_learnable_tau_cpu.py vouches for it on the CPU (the float32 restatement stays
inside, the defects fall outside, the reference's recorded gradients are met); tests/test_gpu_learnable_tau_kernels.py holds the kernels
to it.

What the kernels compute (reference models/dusty.py:25-26, 38-43).  Sigmoid k (pixel, image) has a scalar weight w_k and the slope
    inv_k = log1pf(__expf(w_k)) + inv_min,            inv_min = 1 / tau_max.
Forward: the masks are [sigmoid(l inv_k) > 0.5] = [l > 0] - they do not depend on a positive slope; dusty2's eval-mode image mask is
the sign of the clean logit.  Backward, in head_px_bwd's symbols (t the saved tanh, c drop_const, go the upstream, l1 / l2 the noisy
logits, mp / mi the saved masks):
    q1 = ((go (t - c) [mi]) sp)(1 - sp)      d1 = q1 inv_pixel      G_pixel = sum q1 l1
    q2 = ((go (t - c) mp) si)(1 - si)        d2 = q2 inv_image      G_image = sum q2 l2
    dtau_w[k] += sigma(w_k) G_k,              sigma(w) = 1 / (1 + __expf(-w))      (d inv_k / d w_k)

Criteria.
slope      e = __expf(w) is good to exp_rel(w) relative; d log1p(e) = de / (1 + e), so it reaches the logarithm as sigma(w) exp_rel(w),
           absolute; log1pf adds its own LOG1P_ULPS (2 LOG1P_ULPS D24 softplus(w)); the addition of inv_min rounds once:
               |inv - inv64| <= sigma(w) exp_rel(w) + 2 LOG1P_ULPS D24 softplus(w) + D24 inv                         [slope]
sigmoid    the kernel's argument is z = fl(l inv) with inv known to e_inv only: |z - l inv64| <= |l| e_inv + D24 |z|, which reaches
           s as s (1 - s) e_z on top of net_end_ref.sig_parts' own error (and 1 - s alike)                           [sig_lt]
d0         head_bwd_ref's, unchanged.  d1 / d2: prod_bound of (pre, s, 1 - s, inv) with three roundings, inv known to e_inv.
terms      prod_bound of (pre, s, 1 - s, l) with three roundings; l = fl(h + noise) is the kernel's own float.  At the largest slope
           a saturated logit takes the exponential out of the normal range (e^-107): s (1 - s) may be flushed, so d1, d2 and the
           terms carry net_end_ref's TINY of absolute slack.
dtau_w[k]  sigma(w) G_k in float64 within
               sigma [sum of the terms' bounds + sum_bound(head_bwd_adds, sum |terms|) + 2^-33 per fixed-point contribution]
               + |G_k| sigma relerr(sigma) + 2 D24 sigma sum |terms|
           - sigma's own bound is sig_parts' (relerr(sigma) = (1 - sigma) exp_rel(w) + 2 D24); the last term covers the product
           sigma x total (once per launch on the fixed-point path, once per block with float atomics) and the add onto dtau_w.
"""
import numpy as np

from tests import net_end_ref as N
from tests.net_end_ref import D24, SLACK, TINY, F, Ref, f64

WEIGHTS = (0.0, -3.0, 2.5)        # the temperature weights under test; pixel and image take different ones
INV_MIN = 1.0                     # 1 / tau_max as the wrappers build it


def softplus64(w):
    return np.logaddexp(0.0, f64(w))


def sigma64(w):
    return 1.0 / (1.0 + np.exp(-f64(w)))


def slope(w, inv_min=INV_MIN, defect=None):
    """(inv64, bound) of the slope the kernel forms from the float w.  defect no_min: 1 / tau_max left out"""
    w, inv_min = float(F(w)), float(F(inv_min))
    sp = float(softplus64(w))
    inv = sp + (0.0 if defect == "no_min" else inv_min)
    e = float(sigma64(w) * N.exp_rel(w)) + 2.0 * N.LOG1P_ULPS * D24 * sp + D24 * inv
    return inv, e * SLACK + TINY


def slope32(w, inv_min=INV_MIN):
    """the kernel's arithmetic in float32 (np.exp / np.log1p for __expf / log1pf)"""
    return F(np.log1p(np.exp(F(w))).astype(F) + F(inv_min))


def sigma_parts(w):
    """sigma(w) and its relative error bound"""
    s, s_rel, _, _ = N.sig_parts(F(w))
    return float(s), float(s_rel)


def sig_lt(l, inv, e_inv):
    """z = l inv64, s, |err s|, 1 - s, |err (1 - s)| for the kernel's z = fl(l inv32)"""
    z = f64(l) * inv
    e_z = np.abs(f64(l)) * e_inv + D24 * np.abs(z)
    s, s_rel, oms, e_oms = N.sig_parts(z)
    reach = s * oms * e_z
    return z, s, s * s_rel + reach, oms, e_oms + reach


def formed_l(inp):
    """the noisy logits as the kernel forms them, float32: l1 = fl(h1 + noise_pixel), l2 = fl(h2 + noise_image)"""
    l1 = (np.asarray(inp.h1, dtype=F) + np.asarray(inp.npx, dtype=F)).astype(F)
    l2 = (np.asarray(inp.h2, dtype=F) + np.asarray(inp.nim, dtype=F)[:, None]).astype(F)
    return l1, l2


def excluded_pixels_lt(inp, wp, wi, inv_min=INV_MIN):
    """pixels whose mask an fp32 sigmoid at the learnable slopes could decide either way (must be 0)"""
    l1, l2 = formed_l(inp)
    bad = 0
    for l, w in (((l1, wp),) if inp.arch == 1 else ((l1, wp), (l2, wi))):
        inv, e = slope(w, inv_min)
        z = np.abs(f64(l)) * (inv - e)
        bad += int(((l != 0) & (z < 2.0 ** -7)).sum())
    return bad


def lt_inputs(tier, arch, B, HW, seed=0):
    """net_end_ref.head_inputs at tau = 1: every slope under test is at least 1, so its promise (no noisy logit within 2^-7 of zero
    unless exactly zero) holds at the learnable slopes too - excluded_pixels_lt asserts it case by case"""
    return N.head_inputs(tier, arch, B, HW, seed=seed, tau=1.0)


def lt_bwd_ref(inp, wp, wi, inv_min=INV_MIN, defect=None):
    """unscaled head gradients d [3][B,HW] with bounds b, the temperature terms g [2][B,HW] with bounds gb, the slopes and sigma(w).
    defects: si_for_sp (the pixel sum from the image sigmoid), clean_l (l taken without its noise), no_min (the slope without
    1 / tau_max), d_uses_other (d1 scaled by the image slope)"""
    arch, c = inp.arch, inp.c
    t, go, mp, mi = f64(inp.t), f64(inp.go), f64(inp.mp), f64(inp.mi)
    l1, l2 = formed_l(inp)
    inv_p, e_p = slope(wp, inv_min, defect)
    inv_i, e_i = slope(wi, inv_min, defect) if arch == 2 else (inv_p, e_p)
    dt = 1.0 - t * t
    e_dt = D24 * (t * t + np.abs(dt))
    zero = np.zeros_like(t)
    m = mp * mi if arch == 2 else mp
    d0, b0 = N.prod_bound([m * go, dt], [None, e_dt], 1)
    tc = t - c
    dmask, e_dm = N.prod_bound([go, tc], [None, D24 * np.abs(tc)], 1)
    _, sp, e_sp, omp, e_omp = sig_lt(l1, inv_p, e_p)
    lt1 = f64(inp.h1) if defect == "clean_l" else f64(l1)
    if arch == 1:
        d1, b1 = N.prod_bound([dmask, sp, omp, inv_p], [e_dm, e_sp, e_omp, e_p], 3)
        g1, gb1 = N.prod_bound([dmask, sp, omp, lt1], [e_dm, e_sp, e_omp, None], 3)
        return Ref(d=[d0, d1, zero], b=[b0 * SLACK, b1 * SLACK + TINY, zero], g=[g1, zero], gb=[gb1 * SLACK + TINY, zero],
                   inv=(inv_p, inv_p), e_inv=(e_p, e_p))
    _, si, e_si, omi, e_omi = sig_lt(l2, inv_i, e_i)
    lt2 = f64(inp.h2) if defect == "clean_l" else f64(l2)
    pre1, pre2 = dmask * mi, dmask * mp
    if defect == "si_for_sp":
        g1, gb1 = N.prod_bound([pre1, si, omi, lt1], [e_dm * mi, e_si, e_omi, None], 3)
    else:
        g1, gb1 = N.prod_bound([pre1, sp, omp, lt1], [e_dm * mi, e_sp, e_omp, None], 3)
    k1, ek1 = (inv_i, e_i) if defect == "d_uses_other" else (inv_p, e_p)
    d1, b1 = N.prod_bound([pre1, sp, omp, k1], [e_dm * mi, e_sp, e_omp, ek1], 3)
    d2, b2 = N.prod_bound([pre2, si, omi, inv_i], [e_dm * mp, e_si, e_omi, e_i], 3)
    g2, gb2 = N.prod_bound([pre2, si, omi, lt2], [e_dm * mp, e_si, e_omi, None], 3)
    return Ref(d=[d0, d1, d2], b=[b0 * SLACK, b1 * SLACK + TINY, b2 * SLACK + TINY], g=[g1, g2],
               gb=[gb1 * SLACK + TINY, gb2 * SLACK + TINY], inv=(inv_p, inv_i), e_inv=(e_p, e_i))


def dtau_ref(r, k, w, adds, nfix, defect=None):
    """(sigma(w) G_k, bound) from lt_bwd_ref's terms; adds = head_bwd_adds' count, nfix = the fixed-point contributions (0 on the
    float-atomic path).  defect no_sigma: G_k itself"""
    G, mag = float(r.g[k].sum()), float(np.abs(r.g[k]).sum())
    sg, sg_rel = sigma_parts(w)
    if defect == "no_sigma":
        sg, sg_rel = 1.0, 0.0
    bound = sg * (float(r.gb[k].sum()) + N.sum_bound(adds, mag) + nfix * 2.0 ** -33) + abs(G) * sg * sg_rel + 2.0 * D24 * sg * mag
    return sg * G, bound * SLACK + TINY


def lt_bwd32(inp, wp, wi, inv_min=INV_MIN):
    """head_px_bwd_lt's arithmetic in float32, in its order: (d [3], g [2])"""
    arch = inp.arch
    t, go, mp, mi = (np.asarray(a, dtype=F) for a in (inp.t, inp.go, inp.mp, inp.mi))
    l1, l2 = formed_l(inp)
    one, c = F(1.0), F(inp.c)
    ip = slope32(wp, inv_min)
    ii = slope32(wi, inv_min) if arch == 2 else ip
    dt = one - t * t
    zero = np.zeros_like(t)
    with np.errstate(over="ignore"):                # (a saturated logit at the largest slope: e^107 is inf, the sigmoid exactly 0)
        sp = one / (one + np.exp(-l1 * ip))
        si = one / (one + np.exp(-l2 * ii))
    dmask = go * (t - c)
    if arch == 1:
        q1 = dmask * sp * (one - sp)
        return [mp * go * dt, q1 * ip, zero], [q1 * l1, zero]
    q1, q2 = dmask * mi * sp * (one - sp), dmask * mp * si * (one - si)
    return [mp * mi * go * dt, q1 * ip, q2 * ii], [q1 * l1, q2 * l2]


def lt_intermediates(inp, wp, wi, inv_min=INV_MIN):
    """what assert_normal looks at, beyond net_end_ref.head_intermediates: the sigmoids' arguments at the learnable slopes"""
    l1, l2 = formed_l(inp)
    out = [l1, f64(l1) * slope(wp, inv_min)[0]]
    if inp.arch == 2:
        out += [l2, f64(l2) * slope(wi, inv_min)[0]]
    return out


# ---- the case table of tests/test_gpu_learnable_tau_kernels.py -----------------------------------------------------------------------
# (tier, arch, B, HW, w_pixel, w_image): (3, 21) the scalar form with float atomics, (3, 1024) the four-pixel form with one block per
# sample, (3, 4096) tickets within a sample, (128, 8196) both ticket levels and two grid-stride trips
LT_BWD = [(t, a, 3, hw, wp, wi) for hw in (21, 1024, 4096) for t in N.TIERS for a, wp, wi in ((1, -3.0, 0.0), (2, 0.0, 2.5), (2, 2.5, -3.0))] + \
         [("random", 1, 128, 8196, 2.5, 0.0), ("random", 2, 128, 8196, -3.0, 2.5), ("grid", 2, 128, 8196, 0.0, -3.0)]
LT_AUG = [(2, 32, 64), (3, 64, 256)]     # (B, H, W) of the aug form, full policy


def lt_case_id(c):
    return "-".join(str(v) for v in c)


def lt_case_inputs(case):
    tier, arch, B, HW, wp, wi = case
    return lt_inputs(tier, arch, B, HW, seed=1 if arch == 2 else 0)     # (arch 2: c = 0.5)
