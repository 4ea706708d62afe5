"""The step's network end in float64 - head post-processing (csrc/head_post.hip, head_post.h, dg_tanh of common.h), the final conv's
16-byte kernels, the GAN losses, the path-length penalty and the small reductions (csrc/pointwise.hip) - with the input makers and
the per-element criteria the kernels are held to.  Imports no GPU and nothing of the project.  tests/test_net_end_ref_cpu.py proves
on the CPU that these restatements equal autograd in float64, that the same arithmetic carried out in float32 stays inside the
criteria and that the wrong variants (the `defect` switches below) fall outside; tests/test_gpu_net_end.py holds the kernels to them.

Every function is written once and is dtype-generic: on float64 arrays it is the reference, on float32 arrays it is the float32
restatement of the kernel's arithmetic (numpy rounds every float32 operation correctly, without multiply-add contraction).

Units.  D24 = 2^-24 bounds the relative error of one correctly rounded fp32 operation.  The Makefile passes no fast-math flag, so
`/` and sqrtf are correctly rounded; FMA contraction only removes roundings, so a count of one rounding per operation is an upper
bound.  Results below the smallest normal number may be flushed: every bounded criterion carries TINY = 2^-126 of absolute slack
where a transcendental can underflow, and the inputs keep every other intermediate normal or exactly zero (assert_normal).
Every bound is first order; SLACK = 1 + 2^-10 covers the products of the relative errors (each below 2^-14 here).

Borrowed figures (NOT measured here; constants with their sources):
  EXP_ULPS = 1    __expf(x) is __builtin_amdgcn_exp2f(0x1.715476p+0f * x) in this toolchain's __clang_hip_math.h; the base-2
                  exponential instruction is taken as good to 1 ulp (AMD's ISA manuals; no copy at hand: borrowed).  One ulp is at
                  most 2 D24 relative; the rounded product x log2e and the rounded constant move the argument by at most 1.5 D24 |x| log2e, i.e. the result by 1.04 |x| D24 relative - taken as 2 |x| D24:
                      relerr(__expf(x)) <= (2 EXP_ULPS + 2 |x|) D24                                             [exp_rel]
  RCP_ULPS = 1    __frcp_rn(x) is __ocml_div_rte_f32(1.0f, x) / 1.0f / x there: correctly rounded, half an ulp; the issue's figure of
                  one ulp is kept (2 D24 relative).
  LOG1P_ULPS = 2  log1pf, OpenCL full-profile bound the device math library is written to (as powf in tests/optim_ref.py).

Criteria, operation by operation.

dg_tanh(x), t against tanh in float64 [tanh_bound]:
  |x| < 0.25   small = ax + (ax x2) P(x2), P the degree-3 Horner form of the odd Taylor series through x^9.  The series alternates
               with decreasing terms, so the truncation is below the x^11 term, 1382/155925 |x|^11.  The correction C = (ax x2) P has
               |C| <= |x|^3 / 3 and relative error 6 D24: x2 (1), ax x2 (1), the product with P (1), and P itself 3 - its leading
               coefficient's rounding (1), the last addition (1), and everything under it, worth at most 2.6 % of P with 8 roundings
               (< 1).  The final addition rounds once: D24 |t|.
  |x| >= 0.25  e = __expf(-2 ax) (the argument is exact), (1 - e) __frcp_rn(1 + e): relative error
               [1 + e r / (1 - e)] + [1 + e r / (1 + e)] + 2 RCP_ULPS + 1 in D24, r = exp_rel(2 ax) / D24.  1 - e >= 0.39: no
               cancellation.  Beyond |x| = 9 the kernel returns exactly +-1 (e is below half an ulp of 1).
  x = +-0      exactly +-0.
sigmoid s = 1 / (1 + __expf(-z)) on the float z the kernel formed (z = fl(l inv_tau), l = fl(h + noise), inv_tau = fl(1 / tau)):
               e's error reaches s scaled by e / (1 + e) = 1 - s; the addition and the division round once each:
                   relerr(s) <= (1 - s) exp_rel(z) + 2 D24                                                     [sig_parts]
               1 - s in fp32: |err| <= s relerr(s) + D24 (1 - s) - absolute, since it cancels for large z.
masks        exact.  The inputs keep |z| >= 2^-7 or l == 0: e <= exp(-2^-7)(1 + 1e-6) puts s above 0.5019, l = 0 gives e = 1 and
               s = 0.5 exactly, and the mask is [s > 0.5]: it is [l > 0] whatever the exponential's last bits.
depth        m t + (1 - m) c on the kernel's own stored t, value for value (m is 0 or 1).
a product of fp32 factors f_i known to e_i with k roundings: sum_i e_i prod_{j != i} |f_j| + k D24 |prod|          [prod_bound]
head_post_bwd  dt = 1 - t t: D24 (t^2 + |dt|); d0 = (m go) dt one product.  tc = t - c and dmask = go tc round once each,
               d1 = ((dmask mi) sp)(1 - sp) inv_tau three products on sig_parts' errors; d2 alike.  The planar output times a
               power-of-two scale is exact; the pixel-major copy is its RNE, bit for bit.
head_post_bwd2 each Hessian term is a prod_bound of its own factors (sp' = s (1 - s) inv_tau two products, sp'' = sp' (1 - 2 s)
               inv_tau with 1 - 2 s known to 2 s relerr(s) + D24 |1 - 2 s|); a row adds three terms (2 roundings, each at most
               D24 sum |T_k|) and multiplies by y (1): bound = |y| (sum_k err(T_k) + 3 D24 sum_k |T_k|).  A term 1e-3 of the row
               is still 1e4 times the bound.
float sums   (serial adds per thread + tree depth + 1) D24 sum |terms| over the sum's own terms [sum_bound], plus the terms' own
               bounds; a 32.32 fixed-point stage adds 2^-33 per contribution.
final conv   y, dwf: integers times dyadics, exact in any order.  dd4 = fl32(fl32(u w) c32), c32 = sqrt2f or fl32(0.2f sqrt2f):
               u w is exact, ONE rounding, then RNE to bf16.  dbias: float-sum rule over the terms rs[b] g[b][i] (1 rounding each).
GAN losses   means by the float-sum rule; x = y - mean carries the mean's error e_x; softplus(a) = log1pf(__expf(a)):
               sigmoid(a) (exp_rel(a) + e_x) + 2 LOG1P_ULPS D24 softplus(a), and e^-a where the kernel may have taken the
               x > 20 branch; sigmoid as above with e_x added to exp_rel; square and hinge round once per operation; a hinge
               derivative may flip only where |1 + s x| <= e_x (never for the non-relativistic metrics: e_x = 0, and a rounded sum
               keeps its sign).  dy = k (d - mean d'), k = fl(w_gan / B).
pl_penalty   sum of squares: non-negative terms, relative (1 + ceil(K / 64) + 6) D24; sqrtf halves it and rounds once; the
               baseline, the deviations, the penalty, dl and v = ((w dl) dz) / len follow term by term in pl_bounds, with len's error
               carried through dl and through the division.  A zero sample gives v = 0 exactly.  0.01f is not dyadic and the
               kernel's a = ema + 0.01f (mu - ema) may contract: bit-exactness is asserted where it does not depend on either - equal
               lengths with ema = their common value (a = ema, every deviation 0, v = +-0) - and at K = 1 otherwise bounded.
"""
import numpy as np

from tests.optim_ref import D24, RATIOS, TINY, bf16_rne_bits, bf16_value, f64, failure_report, note, ratio_of, u, w32  # noqa: F401

EXP_ULPS = 1.0
RCP_ULPS = 1.0
LOG1P_ULPS = 2.0
SLACK = 1.0 + 2.0 ** -10
F = np.float32
METRICS = ("nsgan", "wgan", "lsgan", "hinge", "ragan", "rahinge", "ralsgan")
EXACT_METRICS = ("wgan", "lsgan", "hinge", "rahinge", "ralsgan")
SQRT2F = F(1.4142135623730951)
C_POS, C_NEG = SQRT2F, F(F(0.2) * SQRT2F)            # the folded float constants of lrelu' sqrt2
C01 = w32(0.01)                                      # `0.01f`


class Ref(dict):
    __getattr__ = dict.__getitem__


def _like(x, v):
    """the scalar v in x's dtype (keeps float32 arithmetic float32)"""
    return np.asarray(x).dtype.type(v)


def exp_rel(x):
    return (2.0 * EXP_ULPS + 2.0 * np.abs(f64(x))) * D24


def prod_bound(fs, es, nmul):
    """(value, error bound) of the fp32 product of factors fs known to es, nmul roundings"""
    fs = [f64(f) for f in fs]
    val = fs[0]
    for f in fs[1:]:
        val = val * f
    err = nmul * D24 * np.abs(val)
    for i, e in enumerate(es):
        if e is None:
            continue
        p = f64(e)
        for j, f in enumerate(fs):
            if j != i:
                p = p * np.abs(f)
        err = err + p
    return val, err


def sum_bound(n_adds, mag):
    return (n_adds + 1) * D24 * mag


# ---- dg_tanh -----------------------------------------------------------------------------------------------------------------
TANH_C = (F(-0.33333333333), F(0.13333333333), F(-0.05396825397), F(0.02186948854))


def dg_tanh32(x, seam=0.25, drop_last=False):
    """common.h's dg_tanh in float32 (np.exp for __expf, a correctly rounded reciprocal).  defects: seam, drop_last"""
    x = np.asarray(x, dtype=F)
    ax = np.abs(x)
    e = np.exp(F(-2.0) * ax)
    big = (F(1.0) - e) * (F(1.0) / (F(1.0) + e))
    x2 = x * x
    c = TANH_C
    inner = c[2] if drop_last else c[2] + x2 * c[3]
    small = ax + ax * x2 * (c[0] + x2 * (c[1] + x2 * inner))
    return np.copysign(np.where(ax < F(seam), small, big), x).astype(F)


def tanh_bound(x):
    ax = np.abs(f64(x))
    t = np.tanh(ax)
    small = (1382.0 / 155925.0) * ax ** 11 + 6.0 * D24 * ax ** 3 / 3.0 + D24 * t
    e = np.exp(-2.0 * ax)
    r = exp_rel(2.0 * ax)
    om = np.where(ax >= 0.25, 1.0 - e, 1.0)
    big = t * ((D24 + e * r / om) + (D24 + e * r / (1.0 + e)) + 2.0 * RCP_ULPS * D24 + D24)
    return np.where(ax == 0, 0.0, np.where(ax < 0.25, small, big) * SLACK + TINY)


def tanh_sweep():
    """8192 points geometric in [2^-24, 16], both neighbourhoods of 0.25 within 4 ulp, and their negatives: 16384 values"""
    g = np.exp2(np.linspace(-24.0, 4.0, 8192 - 9)).astype(F)
    # below 0.25 an ulp is 2^-26; above, 2^-25: every neighbour within 4 ulp
    near = np.concatenate([F(0.25) - np.arange(1, 5) * F(2.0 ** -26), [F(0.25)], F(0.25) + np.arange(1, 5) * F(2.0 ** -25)]).astype(F)
    pos = np.sort(np.concatenate([g, near]))
    assert pos.size == 8192
    return np.concatenate([pos, -pos]).astype(F)


# ---- sigmoid pieces ------------------------------------------------------------------------------------------------------------
def sigmoid(z):
    one = _like(z, 1.0)
    return one / (one + np.exp(-z))


def sig_parts(z):
    """s, relerr(s), 1 - s, abs err of the fp32 1 - s, for the float z the kernel formed (widened)"""
    z = f64(z)
    s, oms = 1.0 / (1.0 + np.exp(-z)), 1.0 / (1.0 + np.exp(z))
    s_rel = oms * exp_rel(z) + 2.0 * D24
    return s, s_rel, oms, s * s_rel + D24 * oms


def formed(h, noise, tau):
    """the noisy logit and the sigmoid's argument as the kernel forms them: l = fl(h + noise), z = fl(l fl(1 / tau)); float32"""
    inv_tau = F(1.0) / F(tau)
    l = np.asarray(h, dtype=F) + np.asarray(noise, dtype=F)
    return l, (l * inv_tau).astype(F), inv_tau


# ---- head inputs ---------------------------------------------------------------------------------------------------------------
RAW_PLANTS = [0.25, -0.25, np.nextafter(F(0.25), F(0)), np.nextafter(F(0.25), F(1)), -np.nextafter(F(0.25), F(0)),
              -np.nextafter(F(0.25), F(1)), 0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 9.0, -9.0, 90.0, -90.0]
TAUS = (1.0, 0.5, 2.0)


def head_inputs(tier, arch, B, HW, seed=0, tau=None):
    """One case's operands, float32.  tier 'grid': logits and noise multiples of 2^-6 in [-8, 8], zeros planted in l1 and l2, saved
    t a multiple of 1/8, go of 1/4; 'random': seeded normals, tau 0.8, the planted raw values and saturated logits; 'sat': the grid
    tier with raw in {0, +-16, +-90} - tanh is exactly 0, +-1 and every depth sum is a sum of integers."""
    rng = np.random.default_rng(1000 * seed + 7 * HW + 31 * B + arch + {"grid": 0, "random": 1, "sat": 2}[tier])
    sh = (B, HW)
    if tier == "random":
        tau = 0.8 if tau is None else tau
        raw = (rng.standard_normal(sh) * 1.5).astype(F)
        h1, h2 = (rng.standard_normal(sh) * 2.0).astype(F), (rng.standard_normal(sh) * 2.0).astype(F)
        npx, nim = rng.logistic(size=sh).astype(F), rng.logistic(size=B).astype(F)
        t = np.tanh(rng.standard_normal(sh)).astype(F)
        go = rng.standard_normal(sh).astype(F)
        th = rng.standard_normal((B, 3, HW)).astype(F)
        k = min(len(RAW_PLANTS), HW)
        raw[:, :k] = np.asarray(RAW_PLANTS[:k], dtype=F)
        if HW >= 20:                                    # saturated logits: the derivatives underflow to exactly 0 on one side
            for j, v in ((14, 30.0 / tau), (15, -30.0 / tau)):
                h1[:, j], npx[:, j] = v, 0.0
                h2[:, j + 2] = F(v) - nim                # (l2 = fl(h2 + nim) is then within an ulp of +-30 / tau)
    else:
        tau = TAUS[seed % 3] if tau is None else tau
        q = lambda: (rng.integers(-512, 513, sh) / 64.0).astype(F)
        raw, h1, h2, npx = q(), q(), q(), q()
        nim = (rng.integers(-512, 513, B) / 64.0).astype(F)
        if tier == "sat":
            raw = rng.choice(np.asarray([0.0, 16.0, -16.0, 90.0, -90.0], dtype=F), sh)
        else:
            raw[:, :min(4, HW)] = np.asarray([0.25, -0.25, 0.0, 8.0], dtype=F)[:min(4, HW)]
        z = rng.random(sh) < 0.05                       # zeros planted: l1 = 0, l2 = 0
        npx = np.where(z, -h1, npx).astype(F)
        z2 = rng.random(sh) < 0.05
        h2 = np.where(z2, -nim[:, None], h2).astype(F)
        z3 = (rng.random(sh) < 0.05) & ~z2              # h2 = 0 with a live image noise: the eval mask differs from the training mask
        h2 = np.where(z3, 0.0, h2).astype(F)
        t = (rng.integers(-8, 9, sh) / 8.0).astype(F)
        go = (rng.integers(-16, 17, sh) / 4.0).astype(F)
        th = (rng.integers(-8, 9, (B, 3, HW)) / 4.0).astype(F)
    # no pixel may sit where an fp32 sigmoid could land on the other side of 0.5: 0 < |z| < 2^-7 is resampled to l = 0.5
    for _ in range(2):
        l1, z1, _i = formed(h1, npx, tau)
        bad = (z1 != 0) & (np.abs(z1) < 2.0 ** -7)
        npx = np.where(bad, F(0.5) - h1, npx).astype(F)
        l2, z2_, _i = formed(h2, nim[:, None], tau)
        bad2 = (z2_ != 0) & (np.abs(z2_) < 2.0 ** -7)
        h2 = np.where(bad2, F(0.5) - nim[:, None], h2).astype(F)
    mp = (rng.random(sh) < 0.6).astype(F)
    mi = (rng.random(sh) < 0.6).astype(F)
    return Ref(tier=tier, arch=arch, B=B, HW=HW, tau=w32(tau), c=-1.0 if seed % 2 == 0 else 0.5, raw=raw, h1=h1, h2=h2, npx=npx, nim=nim,
               t=t, go=go, th=th[:, :1 + arch].copy(), mp=mp, mi=mi)


def head_formed(inp):
    """(l1, z1, l2, z2, inv_tau) float32 as the kernel forms them"""
    l1, z1, it = formed(inp.h1, inp.npx, inp.tau)
    l2, z2, _ = formed(inp.h2, inp.nim[:, None], inp.tau)
    return l1, z1, l2, z2, it


def excluded_pixels(inp):
    """pixels whose mask an fp32 sigmoid could decide either way (must be 0: asserted case by case), and the count of exact zeros"""
    _, z1, _, z2, _ = head_formed(inp)
    bad = 0
    for z in ((z1,) if inp.arch == 1 else (z1, z2) if inp.arch == 2 else ()):
        bad += int(((z != 0) & (np.abs(z) < 2.0 ** -7)).sum())
    return bad


def assert_normal(arrays, what=""):
    """every value is zero or a normal fp32 number"""
    for k, x in enumerate(arrays):
        a = np.abs(f64(x))
        bad = (a > 0) & (a < TINY)
        assert not bad.any(), f"{what} intermediate {k}: {int(bad.sum())} denormal values, e.g. {float(a[bad][0])!r}"
        assert np.isfinite(a).all() and float(a.max(initial=0.0)) < 3e38, f"{what} intermediate {k}: not finite"


# ---- head forward --------------------------------------------------------------------------------------------------------------
def head_fwd_ref(raw, l1, l2, h2, arch, training, c, defect=None):
    """t = tanh(raw) (float64) with its bound, the masks and the overall mask; l1, l2 the formed noisy logits, h2 the clean one.
    defects: ge (threshold >=), eval_noisy (the eval branch reads the noisy logit)"""
    gt = (lambda a: a >= 0) if defect == "ge" else (lambda a: a > 0)
    t = np.tanh(f64(raw))
    one = np.ones_like(t)
    mp = gt(f64(l1)).astype(np.float64) if arch >= 1 else one
    mi = one
    if arch == 2:
        mi = gt(f64(l2 if (training or defect == "eval_noisy") else h2)).astype(np.float64)
    return Ref(t=t, bt=tanh_bound(raw), mp=mp, mi=mi, m=mp * mi)


def depth_of(t, m, c):
    """m t + (1 - m) c on a stored t (m in {0, 1}: exact)"""
    return np.where(f64(m) != 0, f64(t), c)


def head_sum_adds(HW, quad):
    """additions on the way to dsum[b] (head_post_fwd_kernel): the thread's serial adds, a quad's pairwise tree, six shuffle levels,
    four waves, the contributors of the sample, the add onto the accumulator"""
    chunk = 256
    while chunk < 4096 and HW % (2 * chunk) == 0:
        chunk *= 2
    return (chunk // 1024 + 2 if quad else chunk // 256) + 6 + 4 + HW // chunk + 1


# ---- head backward -------------------------------------------------------------------------------------------------------------
def head_bwd_ref(t, go, z1, z2, mp, mi, inv_tau, c, arch, defect=None):
    """unscaled gradients w.r.t. the head outputs [3][...] and their bounds; z1, z2 the sigmoids' arguments.
    defects: si_for_sp (d1 from the image sigmoid), dtanh_raw (the saved plane read as raw: 1 - tanh(t)^2)"""
    t, go, mp, mi = f64(t), f64(go), f64(mp), f64(mi)
    tt = np.tanh(t) if defect == "dtanh_raw" else t
    dt = 1.0 - tt * tt
    e_dt = D24 * (tt * tt + np.abs(dt))
    zero = np.zeros_like(t)
    if arch == 0:
        d0, b0 = prod_bound([go, dt], [None, e_dt], 1)
        return Ref(d=[d0, zero, zero], b=[b0 * SLACK, zero, zero])
    m = mp * mi if arch == 2 else mp
    d0, b0 = prod_bound([m * go, dt], [None, e_dt], 1)
    tc = t - c
    dmask, e_dm = prod_bound([go, tc], [None, D24 * np.abs(tc)], 1)
    sp, sp_rel, omp, e_omp = sig_parts(z1)
    if arch == 1:
        d1, b1 = prod_bound([dmask, sp, omp, inv_tau], [e_dm, sp * sp_rel, e_omp, None], 3)
        return Ref(d=[d0, d1, zero], b=[b0 * SLACK, b1 * SLACK, zero])
    si, si_rel, omi, e_omi = sig_parts(z2)
    if defect == "si_for_sp":
        d1, b1 = prod_bound([dmask * mi, si, omi, inv_tau], [e_dm * mi, si * si_rel, e_omi, None], 3)
    else:
        d1, b1 = prod_bound([dmask * mi, sp, omp, inv_tau], [e_dm * mi, sp * sp_rel, e_omp, None], 3)
    d2, b2 = prod_bound([dmask * mp, si, omi, inv_tau], [e_dm * mp, si * si_rel, e_omi, None], 3)
    return Ref(d=[d0, d1, d2], b=[b0 * SLACK, b1 * SLACK, b2 * SLACK])


def head_bwd32(t, go, z1, z2, mp, mi, inv_tau, c, arch):
    """head_px_bwd's arithmetic in float32, in its order"""
    t, go, mp, mi, z1, z2 = (np.asarray(a, dtype=F) for a in (t, go, mp, mi, z1, z2))
    one, it, c = F(1.0), F(inv_tau), F(c)
    dt = one - t * t
    zero = np.zeros_like(t)
    if arch == 0:
        return [go * dt, zero, zero]
    sp = one / (one + np.exp(-z1))
    dmask = go * (t - c)
    if arch == 1:
        return [mp * go * dt, dmask * sp * (one - sp) * it, zero]
    si = one / (one + np.exp(-z2))
    return [mp * mi * go * dt, dmask * mi * sp * (one - sp) * it, dmask * mp * si * (one - si) * it]


def head_bwd_adds(B, HW, quad):
    """additions on the way to dbias[h] (head_post_bwd_kernel): grid-stride trips, the quad's tree, shuffles, waves, one add per block
    and sample (atomics in arrival order, or the fixed-point stages), the final add"""
    px = 4 if quad else 1
    per = 1 if B >= 1024 else 1024 // B
    hb = min((HW // px + 255) // 256, per)
    trips = -(-HW // (hb * 256 * px))
    return trips + (2 if quad else 0) + 6 + 4 + hb * B + 2, hb


def sig_derivs(z, inv_tau, defect=None):
    """sp, sp' = s (1 - s) inv_tau and sp'' = sp' (1 - 2 s) inv_tau with their error bounds.  defect sp2_tau: sp'' without its inv_tau"""
    s, s_rel, oms, e_oms = sig_parts(z)
    s1, e_s1 = prod_bound([s, oms, inv_tau], [s * s_rel, e_oms, None], 2)
    k = 1.0 - 2.0 * s
    e_k = 2.0 * s * s_rel + D24 * np.abs(k)
    if defect == "sp2_tau":
        s2, e_s2 = prod_bound([s1, k], [e_s1, e_k], 1)
    else:
        s2, e_s2 = prod_bound([s1, k, inv_tau], [e_s1, e_k, None], 2)
    return s1, e_s1, s2, e_s2


def head_bwd2_ref(t, y, th, z1, z2, mp, mi, inv_tau, c, arch, defect=None):
    """the tangent of head_bwd_ref along th [B,1+arch,...]: unscaled rows [3][...] and bounds.  defects: no_H12, sp2_tau"""
    t, y, th, mp, mi = f64(t), f64(y), f64(th), f64(mp), f64(mi)
    dt = 1.0 - t * t
    e_dt = D24 * (t * t + np.abs(dt))
    q, e_q = prod_bound([-2.0 * t, dt], [None, e_dt], 1)
    t0 = th[:, 0]
    zero = np.zeros_like(t)

    def row(terms):
        tot, err, mag = zero, zero, zero
        for v, e in terms:
            tot, err, mag = tot + v, err + e, mag + np.abs(v)
        return y * tot, np.abs(y) * (err + 3.0 * D24 * mag) * SLACK

    if arch == 0:
        d0, b0 = row([prod_bound([q, t0], [e_q, None], 1)])
        return Ref(d=[d0, zero, zero], b=[b0, zero, zero])
    tc = t - c
    e_tc = D24 * np.abs(tc)
    sp1, e_sp1, sp2, e_sp2 = sig_derivs(z1, inv_tau, defect)
    t1 = th[:, 1]
    if arch == 1:
        d0, b0 = row([prod_bound([mp, q, t0], [None, e_q, None], 2), prod_bound([sp1, dt, t1], [e_sp1, e_dt, None], 2)])
        d1, b1 = row([prod_bound([sp1, dt, t0], [e_sp1, e_dt, None], 2), prod_bound([tc, sp2, t1], [e_tc, e_sp2, None], 2)])
        return Ref(d=[d0, d1, zero], b=[b0, b1, zero])
    si1, e_si1, si2, e_si2 = sig_derivs(z2, inv_tau, defect)
    t2 = th[:, 2]
    h12 = (lambda tv: (zero, zero)) if defect == "no_H12" else (lambda tv: prod_bound([tc, sp1, si1, tv], [e_tc, e_sp1, e_si1, None], 3))
    d0, b0 = row([prod_bound([mp * mi, q, t0], [None, e_q, None], 2), prod_bound([mi, sp1, dt, t1], [None, e_sp1, e_dt, None], 3),
                  prod_bound([mp, si1, dt, t2], [None, e_si1, e_dt, None], 3)])
    d1, b1 = row([prod_bound([mi, sp1, dt, t0], [None, e_sp1, e_dt, None], 3), prod_bound([tc, mi, sp2, t1], [e_tc, None, e_sp2, None], 3),
                  h12(t2)])
    d2, b2 = row([prod_bound([mp, si1, dt, t0], [None, e_si1, e_dt, None], 3), h12(t1),
                  prod_bound([tc, mp, si2, t2], [e_tc, None, e_si2, None], 3)])
    return Ref(d=[d0, d1, d2], b=[b0, b1, b2])


def head_bwd2_32(t, y, th, z1, z2, mp, mi, inv_tau, c, arch):
    """head_post_bwd2_kernel's arithmetic in float32, in its order"""
    t, y, th, mp, mi, z1, z2 = (np.asarray(a, dtype=F) for a in (t, y, th, mp, mi, z1, z2))
    one, two, it, c = F(1.0), F(2.0), F(inv_tau), F(c)
    dt = one - t * t
    t0 = th[:, 0]
    zero = np.zeros_like(t)
    q = -two * t * dt
    if arch == 0:
        return [y * q * t0, zero, zero]
    sp = one / (one + np.exp(-z1))
    sp1 = one * sp * (one - sp) * it
    sp2 = sp1 * (one - two * sp) * it
    t1, tc = th[:, 1], t - c
    if arch == 1:
        return [y * (mp * q * t0 + sp1 * dt * t1), y * (sp1 * dt * t0 + tc * sp2 * t1), zero]
    si = one / (one + np.exp(-z2))
    si1 = one * si * (one - si) * it
    si2 = si1 * (one - two * si) * it
    t2 = th[:, 2]
    return [y * (mp * mi * q * t0 + mi * sp1 * dt * t1 + mp * si1 * dt * t2),
            y * (mi * sp1 * dt * t0 + tc * mi * sp2 * t1 + tc * sp1 * si1 * t2),
            y * (mp * si1 * dt * t0 + tc * sp1 * si1 * t1 + tc * mp * si2 * t2)]


# ---- the pixel-major copy ------------------------------------------------------------------------------------------------------
def pm_problems(pm_bits, planar, nch):
    """structural: pm_bits [B,HW,cp] uint16 must be bf16_rne(planar [B,nch,HW]) channel by channel, padded channels zero.
    Returns a list of complaints (empty: fine)."""
    out = []
    B, HW, cp = pm_bits.shape
    for ch in range(min(nch, cp)):
        want = bf16_rne_bits(planar[:, ch])
        bad = pm_bits[:, :, ch] != want
        if bad.any():
            b, p = np.argwhere(bad)[0]
            out.append(f"pixel-major channel {ch}: {int(bad.sum())} of {bad.size} elements are not the RNE of the planar value, first at "
                       f"sample {b} pixel {p} (p % 4 = {p % 4}): got bits {int(pm_bits[b, p, ch]):#x}, want {int(want[b, p]):#x}")
    if cp > nch and (pm_bits[:, :, nch:] & 0x7FFF).any():
        out.append(f"padded channels of the pixel-major copy are not zero ({int((pm_bits[:, :, nch:] & 0x7FFF != 0).sum())} elements)")
    return out


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def check(what, got, want, bound, fail=True):
    """|got - want| <= bound per element (a zero bound demands equality, a NaN never passes); returns the largest ratio, or
    (ratio, report) with fail = False"""
    bad, q = ratio_of(got, want, bound)
    rep = failure_report(what, bad, got, want, bound) if bad.any() else ""
    if rep and fail:
        raise AssertionError(rep)
    return q if fail else (q, rep)


def same_values(what, got, want, fail=True):
    """value for value (+0 == -0), no NaN: the exact criterion on arrays"""
    return check(what, got, want, 0.0, fail)


TABLE_KEY = "net-end"


def note_ratio(kernel, output, q):
    note(TABLE_KEY, kernel, {output: q})


def format_table():
    slots = {t: s for (k, t), s in RATIOS.items() if k == TABLE_KEY}
    lines = ["kernel | output: largest |got - ref| / bound"]
    for kernel in sorted(slots):
        lines.append(f"{kernel} | " + "  ".join(f"{o}: {q:.3f}" for o, q in sorted(slots[kernel].items())))
    return "\n".join(lines)


# ---- the final conv ------------------------------------------------------------------------------------------------------------
FINAL_N = {"bf16": (8, 512 * 2 + 8, 8192 + 8), "f32": (4, 256 * 2 + 4, 4096 + 4)}   # one lane; three workgroups, the last with one
FINAL_C = (8, 24)                                                                  # live lane; two slabs and three trips
FINAL_B = (1, 3, 4, 5, 9, 256, 257)                                                # 256: the table limit; 257: the scalar form
FINAL_SCALE = 2.0 ** -5


def final_inputs(B, n, seed=0):
    """d4 small integers of both signs with zeros planted, wf small integers, up / rs / coef dyadic, a preloaded y"""
    rng = np.random.default_rng(99 + 13 * B + n + seed)
    d4 = rng.integers(-4, 5, (B, n)).astype(F)
    d4[rng.random((B, n)) < 0.1] = 0.0
    wf = rng.integers(-3, 4, n).astype(F)
    up = (rng.integers(-8, 9, B) / 8.0).astype(F)
    rs = (rng.integers(-8, 9, B) / 4.0).astype(F)
    coef = (rng.integers(-8, 9, B) / 8.0).astype(F)
    return Ref(d4=d4, wf=wf, up=up, rs=rs, coef=coef, bias=F(0.75), y0=(rng.integers(-8, 9, B) / 2.0).astype(F),
               out0=rng.integers(-2, 3, n).astype(F))


def final_fwd_ref(d4, wf, bias, scale, y0=None):
    y = w32(scale) * (f64(d4) @ f64(wf)) + float(bias)
    return y if y0 is None else y + f64(y0)


def final_dd4_ref(d4, wf, u_, scale, defect=None):
    """fl32(fl32(u w) c32), w = wf scale: float32 [B,n].  defect ge: the slope decided by a >= 0"""
    w = (np.asarray(wf, dtype=F) * F(scale))
    uw = np.asarray(u_, dtype=F)[:, None] * w[None, :]
    pos = (d4 >= 0) if defect == "ge" else (d4 > 0)
    return (uw * np.where(pos, C_POS, C_NEG).astype(F)).astype(F)


def final_dbias_ref(g, rs, C, adds, defect=None):
    """dbias[c] = sum over b and the elements i with i % C == c of rs[b] g[b][i], and its bound.  defect ie_div_C: indexed i / C"""
    terms = f64(rs)[:, None] * f64(g)
    n = g.shape[1]
    idx = (np.arange(n) // C) % C if defect == "ie_div_C" else np.arange(n) % C
    db, mag = np.zeros(C), np.zeros(C)
    np.add.at(db, idx, terms.sum(axis=0))
    np.add.at(mag, idx, np.abs(terms).sum(axis=0))
    return db, (adds + 2) * D24 * mag * SLACK


def wsum_ref(src, coef, scale, out0=None, rows=None):
    """out0 + scale sum_b coef[b] src[b]; rows: the samples that contribute (a defect: a sample skipped)"""
    src, coef = f64(src), f64(coef)
    if rows is not None:
        src, coef = src[rows], coef[rows]
    o = w32(scale) * (coef @ src)
    return o if out0 is None else o + f64(out0)


def exact_sum_ok(terms, axis):
    """every partial sum of `terms` along axis is exact in fp32 whatever the order: a multiple of the common unit (>= 2^-32: the arena's
    fixed point holds it too) below 2^24 units"""
    t = np.abs(f64(terms))
    if not t.any():
        return True
    unit = 2.0 ** -40
    while np.array_equal(t / (2 * unit), np.round(t / (2 * unit))):
        unit *= 2
    return unit >= 2.0 ** -32 and float(t.sum(axis=axis).max()) / unit < 2 ** 24


def exact_prefix(terms):
    """the most leading samples of terms [B, ...] whose total is exact in any order (exact_sum_ok over all their elements)"""
    t = np.abs(f64(terms)).reshape(len(terms), -1)
    if not t.any():
        return len(terms)
    unit = 2.0 ** -40
    while np.array_equal(t / (2 * unit), np.round(t / (2 * unit))):
        unit *= 2
    return int((np.cumsum(t.sum(axis=1)) / unit < 2 ** 24).sum()) if unit >= 2.0 ** -32 else 0


# ---- the GAN losses --------------------------------------------------------------------------------------------------------------
def gan_form(metric, mode_g, smoothing, defect=None):
    """(kind_r, kind_f, sign_r, sign_f, target_r, target_f, relativistic) of loss = mean phi_r(a) + mean phi_f(b), read off
    models/loss.py (oracle.gan_loss): softplus(s x), s x, (x - c)^2, relu(1 + s x).  defect lsgan_g_smoothed"""
    rel = metric in ("ragan", "rahinge", "ralsgan")
    kind = {"nsgan": "softplus", "ragan": "softplus", "wgan": "linear", "lsgan": "square", "ralsgan": "square", "hinge": "hinge",
            "rahinge": "hinge"}[metric]
    if not mode_g:
        cr, cf = (smoothing, 0.0) if metric == "lsgan" else (1.0, -1.0)
        return kind, kind, -1.0, 1.0, cr, cf, rel
    if not rel:
        cf = smoothing if defect == "lsgan_g_smoothed" else 1.0
        return None, ("linear" if metric == "hinge" else kind), 0.0, -1.0, 0.0, cf, rel
    return kind, kind, 1.0, -1.0, -1.0, 1.0, rel


def phi(kind, s, c, x):
    """value and derivative, in x's dtype; softplus as the kernel switches it (x > 20: x)"""
    one = _like(x, 1.0)
    if kind == "softplus":
        a = _like(x, s) * x
        with np.errstate(over="ignore"):
            v = np.where(a > _like(x, 20.0), a, np.log1p(np.exp(np.minimum(a, _like(x, 20.0))))) if x.dtype == F else \
                np.logaddexp(0.0, a)
            d = _like(x, s) * (one / (one + np.exp(-a)))
        return v.astype(x.dtype), d.astype(x.dtype)
    if kind == "linear":
        return _like(x, s) * x, np.full_like(x, s)
    if kind == "square":
        q = x - _like(x, c)
        return q * q, _like(x, 2.0) * q
    t = one + _like(x, s) * x
    return np.where(t > 0, t, 0).astype(x.dtype), np.where(t > 0, _like(x, s), 0).astype(x.dtype)


def gan_ref(metric, mode_g, yr, yf, w_gan, smoothing=1.0, defect=None, dtype=np.float64):
    """gan_step_body: means, loss, dy (D: [real | fake], G: fake), up / rs (D), sum dy.  defects: cross_swap, lsgan_g_smoothed"""
    kr, kf, sr, sf, cr, cf, rel = gan_form(metric, mode_g, w32(smoothing), defect)   # (the floats the ABI receives, widened)
    w_gan = w32(w_gan)
    yf = np.asarray(yf, dtype=dtype)
    B = yf.size
    nB = dtype(B)
    has_r = kr is not None or not mode_g
    yr = np.asarray(yr, dtype=dtype) if has_r else None
    mr = (yr.sum(dtype=dtype) / nB) if has_r else dtype(0)
    mf = yf.sum(dtype=dtype) / nB
    offr, offf = (mf, mr) if rel else (dtype(0), dtype(0))
    vf, df_ = phi(kf, sf, cf, yf - offf)
    lsum, mdr = vf.sum(dtype=dtype), dtype(0)
    if kr is not None:
        vr, dr_ = phi(kr, sr, cr, yr - offr)
        lsum, mdr = lsum + vr.sum(dtype=dtype), dr_.sum(dtype=dtype) / nB
    mdf = df_.sum(dtype=dtype) / nB
    if defect == "cross_swap":
        mdr, mdf = mdf, mdr
    k = dtype(np.asarray(w_gan, dtype=dtype) / nB)
    zero = dtype(0)
    df = k * (df_ - (mdr if rel else zero))
    if mode_g:
        return Ref(loss=lsum / nB, dy=df, mr=mr, mf=mf)
    dr = k * (dr_ - (mdf if rel else zero))
    one = np.ones(B, dtype=dtype)
    return Ref(loss=lsum / nB, dy=np.concatenate([dr, df]), up=np.concatenate([one, df]), rs=np.concatenate([dr, one]),
               mr=mr, mf=mf, sum_dy=(dr + df).sum(dtype=dtype))


def gan_bounds(metric, mode_g, yr, yf, w_gan, smoothing=1.0):
    """bounds on gan_ref's outputs, term by term (head comment)"""
    kr, kf, sr, sf, cr, cf, rel = gan_form(metric, mode_g, w32(smoothing))
    yf = f64(yf)
    B = yf.size
    NS = -(-B // 256) + 6 + 4 + 1                     # serial adds, shuffles, waves, the division
    has_r = kr is not None or not mode_g
    yr = f64(yr) if has_r else None
    e_mr = NS * D24 * np.abs(yr).sum() / B if has_r else 0.0
    e_mf = NS * D24 * np.abs(yf).sum() / B
    mr = yr.mean() if has_r else 0.0
    mf = yf.mean()

    def side(kind, s, c, y, off, e_off):
        x = y - off
        ex = (e_off + D24 * np.abs(x)) if rel else np.zeros_like(x)
        if kind == "softplus":
            a = s * x
            sg = 1.0 / (1.0 + np.exp(-a))
            re = exp_rel(a) + ex
            v = np.logaddexp(0.0, a)
            ev = sg * re + 2.0 * LOG1P_ULPS * D24 * v + np.where(a > 20.0 - 2.0 * ex - 1e-6, np.exp(-np.maximum(a, 0.0)) + ex, 0.0) + TINY
            ed = sg * ((1.0 - sg) * re + 2.0 * D24) + TINY
            return v, s * sg, ev, ed
        if kind == "linear":
            return s * x, np.full_like(x, s), ex, np.zeros_like(x)
        if kind == "square":
            q = x - c
            eq = ex + D24 * np.abs(q)
            return q * q, 2.0 * q, 2.0 * np.abs(q) * eq + D24 * q * q, 2.0 * eq
        t = 1.0 + s * x
        et = ex + D24 * np.abs(t)
        return np.maximum(t, 0.0), np.where(t > 0, s, 0.0), et, np.where((np.abs(t) <= ex) & (ex > 0), 1.0, 0.0)

    vf, df_, evf, edf = side(kf, sf, cf, yf, mr if rel else 0.0, e_mr)
    lmag, lerr, nterm = np.abs(vf).sum(), evf.sum(), 1
    mdr, e_mdr = 0.0, 0.0
    if kr is not None:
        vr, dr_, evr, edr = side(kr, sr, cr, yr, mf if rel else 0.0, e_mf)
        lmag, lerr, nterm = lmag + np.abs(vr).sum(), lerr + evr.sum(), 2
        mdr, e_mdr = dr_.mean(), edr.sum() / B + NS * D24 * np.abs(dr_).sum() / B
    mdf, e_mdf = df_.mean(), edf.sum() / B + NS * D24 * np.abs(df_).sum() / B
    k = w32(w_gan) / B
    b_loss = (lerr + (nterm * -(-B // 256) + 11) * D24 * lmag) / B * SLACK

    def grad(d_, ed, md, e_md):
        inner = d_ - (md if rel else 0.0)
        return k * inner, (abs(k) * (ed + (e_md + D24 * np.abs(inner) if rel else 0.0)) + 2.0 * D24 * np.abs(k * inner)) * SLACK

    df, b_df = grad(df_, edf, mdr, e_mdr)
    if mode_g:
        return Ref(loss=b_loss, dy=b_df, mr=e_mr, mf=e_mf)
    dr, b_dr = grad(dr_, edr, mdf, e_mdf)
    one0 = np.zeros(B)
    b_sum = (b_dr + b_df).sum() + (NS + 1) * D24 * (np.abs(dr) + np.abs(df)).sum() * SLACK
    return Ref(loss=b_loss, dy=np.concatenate([b_dr, b_df]), up=np.concatenate([one0, b_df]), rs=np.concatenate([b_dr, one0]),
               mr=e_mr, mf=e_mf, sum_dy=b_sum)


def gan_exact_logits(B, small=False):
    """dyadic logits whose every sum is exact and whose means are the dyadic 0.5 (real) and -0.25 (fake) for ANY B: the values come in
    +- pairs around the mean (an odd B adds one element at the mean).  Planted, hinge arguments exactly on the kink: real[0] = 1 + mf
    and fake[0] = mr - 1 (rahinge, D), real[1] = 1 and fake[1] = -1 (hinge, D), real[2] = mf - 1 and fake[2] = 1 + mr (rahinge, G).
    small: |base| <= 1/8 and no plants - every hinge argument stays strictly positive (the derivative's mean is then +-1 whatever B)."""
    if B == 1:
        return np.asarray([0.0], dtype=F), np.asarray([-1.0], dtype=F)
    rng = np.random.default_rng(B)
    h = B // 2
    if small:
        br, bf_ = rng.integers(-4, 5, h) / 32.0, rng.integers(-4, 5, h) / 32.0
    else:
        br, bf_ = rng.integers(-16, 17, h) / 4.0, rng.integers(-16, 17, h) / 4.0
        if h >= 3:
            br[:3] = [0.25, 0.5, -1.75]
            bf_[:3] = [-0.25, -0.75, 1.75]
    mid = [0.0] * (B - 2 * h)
    real = np.concatenate([br, -br, mid]) + 0.5
    fake = np.concatenate([bf_, -bf_, mid]) - 0.25
    return real.astype(F), fake.astype(F)


def gan_random_logits(B, kind="normal", seed=0):
    """normal: N(0, 1.5); saturated: the same with +-25, +-90, 20 and the float after 20 planted; equal: every logit of a side equal"""
    rng = np.random.default_rng(4242 + B + seed)
    yr, yf = (rng.standard_normal(B) * 1.5).astype(F), (rng.standard_normal(B) * 1.5).astype(F)
    if kind == "saturated":
        plants = np.asarray([25.0, -25.0, 90.0, -90.0, 20.0, np.nextafter(F(20.0), F(30.0)), -20.0], dtype=F)
        yr[:7], yf[3:10] = plants, -plants
    if kind == "equal":
        yr[:], yf[:] = F(0.7), F(-1.3)
    return yr, yf


# ---- path-length penalty, mean_acc, scale ------------------------------------------------------------------------------------------
def pl_ref(dz, w, ema, dtype=np.float64, defect=None):
    """pl_penalty_kernel: lengths, baseline a, penalty, v.  defects: no_mdev (the 0.01 mdev term dropped), mean_over_K"""
    dz = np.asarray(dz, dtype=dtype)
    B, K = dz.shape
    nB = dtype(K if defect == "mean_over_K" else B)
    ln = np.sqrt((dz * dz).sum(axis=1, dtype=dtype))
    mu = ln.sum(dtype=dtype) / nB
    ema, c01, w = dtype(ema), dtype(C01), dtype(w)
    a = ema + c01 * (mu - ema)
    e = ln - a
    pen = (e * e).sum(dtype=dtype) / nB
    mdev = e.sum(dtype=dtype) / nB
    inner = e if defect == "no_mdev" else e - c01 * mdev
    dl = (dtype(2.0) / nB) * inner
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(ln[:, None] > 0, (w * dl)[:, None] * dz / ln[:, None], dtype(0))
    return Ref(len=ln, a=a, pen=pen, mdev=mdev, dl=dl, v=v.astype(dtype))


def pl_bounds(dz, w, ema):
    dz = f64(dz)
    B, K = dz.shape
    r = pl_ref(dz, w32(w), w32(ema))
    ln = r.len
    e_len = ln * (0.5 * (1 + -(-K // 64) + 6) + 1.0) * D24
    mu = ln.sum() / B
    e_mu = e_len.sum() / B + (B + 1) * D24 * mu
    ema = w32(ema)
    e_a = C01 * (e_mu + D24 * abs(mu - ema)) + D24 * abs(C01 * (mu - ema)) + D24 * abs(r.a)
    e = ln - r.a
    ee = e_len + e_a + D24 * np.abs(e)
    b_pen = ((2.0 * np.abs(e) * ee).sum() + (B + 2) * D24 * (e * e).sum()) / B
    e_mdev = (ee.sum() + B * D24 * np.abs(e).sum()) / B + D24 * abs(r.mdev)
    inner = e - C01 * r.mdev
    e_dl = (2.0 / B) * (ee + C01 * e_mdev + D24 * abs(C01 * r.mdev) + D24 * np.abs(inner)) + 2.0 * D24 * np.abs(r.dl)
    with np.errstate(divide="ignore", invalid="ignore"):
        lb = np.where(ln > 0, ln, 1.0)[:, None]
        b_v = np.where(ln[:, None] > 0, np.abs(w32(w) * dz / lb) * e_dl[:, None] + np.abs(r.v) * (e_len[:, None] / lb + 3.0 * D24), 0.0)
    return Ref(a=e_a * SLACK, pen=b_pen * SLACK, v=b_v * SLACK, len=e_len)


PL_B = (1, 3, 4, 5, 256)
PL_K = (1, 63, 64, 65, 512)


def pl_inputs(B, K, seed=0):
    """seeded normals, one all-zero sample where B >= 3"""
    dz = np.random.default_rng(17 + 1000 * B + K + seed).standard_normal((B, K)).astype(F)
    if B >= 3:
        dz[1] = 0.0
    return dz


def mean_inputs(n):
    """integers whose sum is a multiple of n: the mean is an integer, every partial sum exact"""
    x = np.random.default_rng(n).integers(-4, 5, n).astype(np.float64)
    x[-1] -= x.sum() % n
    return x.astype(F)


# ---- the case tables: what tests/test_gpu_net_end.py runs and tests/test_net_end_ref_cpu.py vouches for --------------------------------
S_DEPTH, S_CONF = 0.25, 0.5                           # powers of two, never 1: the planar outputs are the unscaled rows, exactly
HEAD_FWD_HW = (21, 256, 768, 1024, 2048, 3072, 4096, 8192)
TIERS = ("grid", "random")
# (tier, arch, B, HW): the small shapes in both tiers and every arch; the large ones once per arch
HEAD_BWD = [(t, a, 3, hw) for hw in (21, 1024, 4096) for t in TIERS for a in (0, 1, 2)] + \
           [("grid", 0, 128, 8196), ("random", 1, 128, 8196), ("random", 2, 128, 8196)]
HEAD_BWD2 = [(t, a, 3, hw) for hw in (21, 256) for t in TIERS for a in (0, 1, 2)] + \
            [("grid", 0, 2, 131200), ("random", 1, 2, 131200), ("random", 2, 2, 131200)]


def case_id(c):
    return "-".join(str(v) for v in c)


def head_case_inputs(case, seed=0):
    tier, arch, B, HW = case
    return head_inputs(tier, arch, B, HW, seed=seed + (1 if arch == 2 else 0))      # (arch 2: tau = 0.5 on the grid, c = 0.5)


def head_bwd_case(inp, defect=None):
    _, z1, _, z2, it = head_formed(inp)
    return head_bwd_ref(inp.t, inp.go, z1, z2, inp.mp, inp.mi, float(it), inp.c, inp.arch, defect)


def head_bwd2_case(inp, defect=None):
    _, z1, _, z2, it = head_formed(inp)
    return head_bwd2_ref(inp.t, inp.go, inp.th, z1, z2, inp.mp, inp.mi, float(it), inp.c, inp.arch, defect)


def head_fwd_case(inp, training, defect=None):
    l1, _, l2, _, _ = head_formed(inp)
    return head_fwd_ref(inp.raw, l1, l2, inp.h2, inp.arch, training, inp.c, defect)


def head_intermediates(inp):
    """what assert_normal looks at: the inputs, the formed logits and arguments, the derivative factors"""
    l1, z1, l2, z2, it = head_formed(inp)
    t = f64(inp.t)
    out = [inp.raw, inp.h1, inp.h2, inp.npx, inp.nim, inp.t, inp.go, inp.th, l1, z1, 1.0 - t * t, t - inp.c, f64(inp.go) * (t - inp.c)]
    if inp.arch == 2:
        out += [l2, z2]
    return out
