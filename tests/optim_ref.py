"""Adam as the six optimizer kernels run it, in float64, and the per-element criteria they are held to.  Imports no GPU and nothing
of the project; tests/test_optim_ref_cpu.py proves on the CPU that a float32 restatement stays inside the criteria and that the
wrong variants an almost-right kernel produces do not, tests/test_gpu_optim.py holds the kernels to them.

The arithmetic (csrc/optim.hip's head comment, oracle/dusty_oracle.py::adam_update), every scalar the float32 value the C ABI
receives, widened:
    gg = g gscale;  m' = b1 m + (1 - b1) gg (= gg at b1 = 0);  v' = b2 v + (1 - b2) gg^2
    delta = (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps),  bc1 = 1 - b1^t,  bc2 = 1 - b2^t;  p' = p - delta
    ema' = d ema + (1 - d) p'
sphere_adam / alpha_adam restate torch's single-tensor Adam on a host-made table row (step_size, bc2s):
    m' = m + (1 - b1)(g - m);  v' = v b2 + (1 - b2) g^2;  x' = x - step_size m' / (sqrt(v') / bc2s + eps)

Units.  D24 = 2^-24 is the relative error of one correctly rounded fp32 operation, u(x) one ulp of fp32 at |x| (u(0) = 0), so a
rounding costs at most 0.5 u(result) <= D24 |result|.  The Makefile passes no fast-math flag: division and sqrtf are correctly
rounded; FMA contraction only removes roundings.  1 - b for b in [0.5, 1) is exact in fp32 (a multiple of 2^-24 below 0.5), so
1 - b1, 1 - b2 and 1 - d cost nothing.

Everything here assumes NORMAL fp32 numbers: the project promises nothing about denormals (the GPU may flush them), so the inputs
keep every input and every intermediate normal or exactly zero - assert_normal() checks it, the CPU tests call it for every case.
The one exception is harmless by construction: powf(b, t) for large t underflows (to a denormal or to zero) and 1 - it is 1 either way.

The criteria, per element:
  v'     |got - want| <= 4 u(want), exactly 0 where g = v = 0.  gg, gg^2, the two products and the sum round once each and every
         term is non-negative.  (The tests use gscale = 0.5, a power of two, as 1 / world_size is: gg is then exact.)
  m'     beta1 > 0: ABSOLUTE, 1.5 u(max(|b1 m|, |(1 - b1) gg|)) - the two terms may cancel; carried into delta through the division.
         The two products and the sum round once each, 0.5 u apiece.  Where the terms ADD and the sum carries into the next binade
         its own half ulp is a whole u of the larger term, and IEEE float32 arithmetic itself reaches 1.9 u there (the CPU test's
         restatement does): the sum's share is 0.5 u(|m'| + u(larger term)), which is the 1.5 u above everywhere else.
         beta1 = 0 with m passed: m' = gg, 0.5 u(gg).  Table form (lerp): 1.5 u(max(|m|, |g|)).
  delta  read where p = 0 (p' = -delta is then rounded once, by the product lr q itself): |got - want| <= rho(t) |want| (+ the m' term),
         rho(t) = (A + P b2^t / bc2(t)) D24 - RHO below.
  p'     where p != 0: 0.5 u(want) + the delta bound.
  ema'   2 u(max(|d ema|, |(1 - d) p'|)) + (1 - d) bound(p').
  shadow the round-to-nearest-even bf16 of the kernel's own p' (fp32 mode: the same bits).

A, operation by operation, from v' to lr q (units of D24):
  v' is within 4 of the truth, the square root halves that      2
  sqrtf, correctly rounded                                       1
  * inv_sqrt_bc2 (or / bc2s)                                     1
  + eps (both summands positive: their errors do not grow)       1
  m' = gg (beta1 = 0: the product g gscale)                      1
  the division                                                   1
  lr * q                                                         1
                                                          A_HOST = 8   dg_adam_ema_step: lr / bc1 and 1 / sqrt(bc2) are made on the
                                                                       host and the reference takes those very floats (P = 0)
                                                         A_TABLE = 7   sphere_adam, alpha_adam: no gscale product; the table row is
                                                                       an input (P = 0)
  in-kernel bias correction rsqrtf(1.f - powf(b2, t)):
  1 - pow rounds once (exact while pow >= 0.5), halved by the root, rounded up   1
  rsqrtf: 2 ulp                                                  2
                                                           A_DEV = 11  every kernel that reads the device step counter
  powf itself: P = 16 ulp, the OpenCL full-profile bound the device math library is written to; bc2 = 1 - b2^t turns a relative
  error e of the power into e b2^t / bc2 (the root would halve it; the bound does not take that).
  beta1 > 0 in-kernel, lr / (1.f - powf(b1, t)): the subtraction and the division, A_BC1 = 2, and P b1^t / bc1.
rho is 9.5e-5 at t = 1 (b2 = 0.99f) and 6.6e-7 from t = 1000 on; a step count off by one is a 15-40 % error at small t.
Nothing here is tuned to what a GPU returns.
"""
import numpy as np

D24 = 2.0 ** -24
POW_ULPS = 16
A_HOST, A_TABLE, A_DEV, A_BC1 = 8, 7, 11, 2
TINY = 2.0 ** -126                                  # smallest normal fp32 number

CLASSES = ("padding", "idle", "eps-bound", "first step", "ordinary", "dominated", "large")


def w32(x):
    """the float32 value the C ABI receives, as a Python float"""
    return float(np.float32(x))


def u(x):
    """one ulp of fp32 at |x| (normal-number formula, u(0) = 0)"""
    a = np.abs(np.asarray(x, dtype=np.float64))
    e = np.maximum(np.floor(np.log2(np.where(a > 0, a, 1.0))), -126.0)
    return np.where(a > 0, 2.0 ** (e - 23.0), 0.0)


def f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


class HP:
    """the scalars of a call as the ABI receives them (float32, widened)"""

    def __init__(self, lr=0.002, b1=0.0, b2=0.99, eps=1e-8, d=0.9, gscale=0.5):
        self.lr, self.b1, self.b2, self.eps, self.d, self.gscale = (w32(x) for x in (lr, b1, b2, eps, d, gscale))

    def host_factors(self, t):
        """dg_adam_ema_step's lr / bc1 and 1 / sqrt(bc2): double arithmetic on the host, rounded to float"""
        return w32(self.lr / (1.0 - self.b1 ** t)), w32(1.0 / np.sqrt(1.0 - self.b2 ** t))


class Ref(dict):
    __getattr__ = dict.__getitem__


def adam_ref(p, g, m, v, ema, t, hp, lr_bc1=None, isb=None):
    """float64 Adam + EMA of step count t (1-based).  m / ema None: absent (m' = gg at b1 = 0).  lr_bc1 / isb: the host-made
    factors where the kernel receives them as inputs."""
    p, g, m, v, ema = (f64(a) for a in (p, g, m, v, ema))
    gg = g * hp.gscale
    m1 = hp.b1 * (m if m is not None else 0.0) + (1.0 - hp.b1) * gg
    v1 = hp.b2 * v + (1.0 - hp.b2) * gg * gg
    S = hp.lr / (1.0 - hp.b1 ** t) if lr_bc1 is None else lr_bc1
    inv = 1.0 / np.sqrt(1.0 - hp.b2 ** t) if isb is None else isb
    D = np.sqrt(v1) * inv + hp.eps
    delta = S * m1 / D
    p1 = p - delta
    e1 = None if ema is None else hp.d * ema + (1.0 - hp.d) * p1
    return Ref(gg=gg, m=m1, v=v1, S=S, D=D, delta=delta, p=p1, ema=e1, p0=p, m0=m, v0=v, ema0=ema, g=g, hp=hp, t=t,
               table=False)


def table_adam_ref(x, g, m, v, row, b1, b2, eps):
    """torch's single-tensor Adam on the schedule table's row = (step_size, bc2s, ...) as given (alpha_ref; sphere_ref's first half)"""
    x, g, m, v = (f64(a) for a in (x, g, m, v))
    b1, b2, eps, step, bc2s = w32(b1), w32(b2), w32(eps), float(row[0]), float(row[1])
    m1 = m + (1.0 - b1) * (g - m)
    v1 = v * b2 + (1.0 - b2) * g * g
    D = np.sqrt(v1) / bc2s + eps
    delta = step * m1 / D
    return Ref(gg=g, m=m1, v=v1, S=step, D=D, delta=delta, p=x - delta, ema=None, p0=x, m0=m, v0=v, ema0=None, g=g,
               hp=HP(0.0, b1, b2, eps, 1.0, 1.0), t=0, table=True)


alpha_ref = table_adam_ref

# dg_block_sum (csrc/common.h) under sphere_adam_kernel (256 threads, <= 4 elements each): a square (1 rounding), 3 additions in the
# thread (the first, onto 0, is exact), 6 xor-shuffle levels of dg_wave_sum, 4 additions over the waves' partials in thread 0
SUMSQ_PATH = 1 + 3 + 6 + 4
RENORM_EPS = w32(1e-9)                              # `1e-9f` in the kernel


def sphere_ref(latent, g, m, v, sched, k, num_step, b1, b2, eps, noise=None):
    """dg_sphere_adam at step index k: Adam from row min(k, num_step), row / sqrt(mean(row^2) + 1e-9); [B, nz] arrays"""
    r = table_adam_ref(latent, g, m, v, np.asarray(sched, dtype=np.float64)[min(k, num_step)], b1, b2, eps)
    r["scale"] = np.sqrt((r.p * r.p).mean(axis=1, keepdims=True) + RENORM_EPS)
    r["row"] = r.p / r.scale
    r["z"] = r.row if noise is None else r.row + f64(noise)
    return r


def rho(t, hp, A, P):
    """relative bound on delta without the m' term; P = 0 where the bias factors are inputs of the kernel"""
    r = float(A)
    if P:
        r += P * hp.b2 ** t / (1.0 - hp.b2 ** t)
        if hp.b1 > 0:
            r += A_BC1 + P * hp.b1 ** t / (1.0 - hp.b1 ** t)
    return r * D24


def bounds(r, A, P, gerr=None):
    """the criteria's bounds for a reference `r`.  gerr: absolute bound on the error of g where the kernel forms it itself
    (dg_adam_proj_fused's dot product; beta1 = 0): |d delta / d g| <= S gscale / D, since D grows with |g|."""
    hp = r.hp
    bv = 4.0 * u(r.v)
    if r.table:
        bm = 1.5 * u(np.maximum(np.abs(r.m0), np.abs(r.g)))
    elif hp.b1 > 0:
        big = u(np.maximum(np.abs(hp.b1 * r.m0), np.abs((1.0 - hp.b1) * r.gg)))
        bm = big + 0.5 * np.maximum(big, u(np.abs(r.m) + big))
    else:
        bm = 0.5 * u(r.gg)
    bd = rho(r.t, hp, A, P) * np.abs(r.delta)
    if r.table or hp.b1 > 0:
        bd = bd + r.S * bm / r.D
    if gerr is not None:
        ge = gerr * hp.gscale
        bv = bv + (1.0 - hp.b2) * (2.0 * np.abs(r.gg) * ge + ge * ge)
        bm = bm + ge
        bd = bd + r.S * ge / r.D
    bp = np.where(r.p0 == 0, bd, 0.5 * u(r.p) + bd)
    be = None
    if r.ema is not None:
        be = 2.0 * u(np.maximum(np.abs(hp.d * r.ema0), np.abs((1.0 - hp.d) * r.p))) + (1.0 - hp.d) * bp
    return Ref(v=bv, m=bm, delta=bd, p=bp, ema=be)


def sphere_bounds(r):
    """bounds of dg_sphere_adam's stored state: m, v as above, `row` for the renormalised latent.
    x' carries bx = 0.5 u(x') + the delta bound.  The sum of squares has only non-negative terms: relative error SUMSQ_PATH D24 from
    its own roundings plus sum(2 |x'| bx) / sum(x'^2) from its inputs; / nz and + 1e-9 round once each; the root halves all of it
    and rounds once.  row = x' / scale: |row| rel(scale) + bx / scale + one rounding."""
    b = bounds(r, A_TABLE, 0)
    bx = b.p
    ssq = (r.p * r.p).sum(axis=1, keepdims=True)
    rel = (0.5 * (SUMSQ_PATH + 2) + 1.0) * D24 + (np.abs(r.p) * bx).sum(axis=1, keepdims=True) / np.maximum(ssq, TINY)
    b["rel_scale"] = rel
    b["row"] = np.abs(r.row) * rel + bx / r.scale + 0.5 * u(r.row)
    return b


# ---- the input classes ---------------------------------------------------------------------------------------------------------
class Inputs:
    """n elements of the seven classes, interleaved: class = i % 7 (7 and 4 are coprime: every class lands on every lane of a float4
    within 28 elements), p = ema = 0 on the blocks of 28 with (i // 28) even and ~ randn on the others.  float32 arrays."""

    def __init__(self, n, seed, hp, with_m=False, cls=None, zero_half=None):
        rng = np.random.default_rng(seed)
        i = np.arange(n)
        c = i % 7 if cls is None else np.asarray(cls).reshape(-1)   # (cls / zero_half given: a layout of the caller's)
        sign = rng.choice([-1.0, 1.0], n)

        def logu(lo, hi):
            return 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)
        g = np.select([c == 0, c == 1, c == 2, c == 3, c == 4, c == 5], [0.0 * sign, 0.0 * sign, sign * logu(1e-9, 1e-6),
                      sign * logu(1e-3, 1e3), rng.standard_normal(n) * 0.1, sign * 1e-3], sign * 1e5)
        v = np.select([c == 0, c == 1, c == 2, c == 3, c == 4, c == 5], [0.0 * sign, logu(1e-6, 1e2), rng.choice([0.0, 1e-18], n),
                      0.0 * sign, rng.uniform(1e-8, 1e-2, n), 1e4 + 0.0 * sign], 1.0 + 0.0 * sign)
        zero_half = (i // 28) % 2 == 0 if zero_half is None else np.asarray(zero_half).reshape(-1)
        self.p = np.where(zero_half, 0.0, rng.standard_normal(n)).astype(np.float32)
        self.ema = np.where(zero_half, 0.0, rng.standard_normal(n)).astype(np.float32)
        self.g, self.v = (g + 0.0).astype(np.float32), np.abs(v).astype(np.float32)      # (no negative zeros)
        self.m = None
        if with_m:
            # exp_avg: of the gradient's size and either sign; every third element cancels (1 - b1) gg to 2^-9; zero where the
            # parameter never had a gradient (padding, idle) and on the first step
            gg = self.g.astype(np.float64) * hp.gscale
            m = gg * rng.uniform(-2.0, 2.0, n)
            if hp.b1 > 0:
                m = np.where(i % 3 == 0, -(1.0 - hp.b1) / hp.b1 * gg * (1.0 + 2.0 ** -9 * rng.integers(1, 8, n)), m)
            self.m = np.where(c == 3, 0.0, m).astype(np.float32)
        self.cls, self.n = c, n


def sphere_inputs(B, nz, seed, b1=0.9):
    """[B, nz] inputs of dg_sphere_adam: gradient and moments of the seven classes along each row, latent rows ~ randn at RMS 1
    (even rows) and 1e-3 (odd rows: the 1e-9 under the root is then a 1e-3 relative term)"""
    inp = Inputs(B * nz, seed, HP(0.0, b1, 0.999, 1e-8, 1.0, 1.0), with_m=True)
    rng = np.random.default_rng(seed + 77)
    lat = rng.standard_normal((B, nz)) * np.where(np.arange(B) % 2 == 0, 1.0, 1e-3)[:, None]
    sh = (B, nz)
    return Ref(latent=lat.astype(np.float32), g=inp.g.reshape(sh), m=inp.m.reshape(sh), v=inp.v.reshape(sh), cls=inp.cls.reshape(sh))


def assert_normal(r):
    """every input and intermediate of a reference is zero or a normal fp32 number (see the module docstring)"""
    hp = r.hp
    vals = [r.g, r.gg, r.gg * r.gg, (1.0 - hp.b2) * r.gg * r.gg, hp.b2 * r.v0, r.v, r.m, r.D, r.delta, r.p, r.p0]
    if r.m0 is not None:
        vals += [r.m0, hp.b1 * r.m0, (1.0 - hp.b1) * r.gg, r.g - r.m0]
    if r.ema is not None:
        vals += [r.ema0, hp.d * r.ema0, (1.0 - hp.d) * r.p, r.ema]
    for k, x in enumerate(vals):
        a = np.abs(x)
        bad = (a > 0) & (a < TINY)
        assert not bad.any(), f"intermediate {k}: {int(bad.sum())} denormal values, e.g. {float(a[bad][0])!r}"
        assert np.isfinite(a).all() and float(a.max(initial=0.0)) < 3e38


# ---- the gradients the fused kernels form ---------------------------------------------------------------------------------------
def fused_grad_ref(parts=None, g0=None, ws_src=None, ws_coef=None, ws_scale=1.0):
    """dg_adam_fused's gradient in float64: the partial rows [splits, n] + the buffer's content (accumulate) + ws_scale sum_b
    coef[b] src[b].  Returns (sum, bound), bound = (rows + 2) D24 sum |terms| over the rows + ws_n (+ 1) terms: one addition per
    term at most, the products coef src and ws_scale w."""
    terms = []
    if parts is not None:
        terms += [f64(x) for x in parts]
    if g0 is not None:
        terms.append(f64(g0))
    if ws_src is not None:
        for b in range(len(ws_src)):
            terms.append(w32(ws_scale) * (1.0 if ws_coef is None else float(ws_coef[b])) * f64(ws_src[b]))
    tot, mag = np.zeros_like(terms[0]), np.zeros_like(terms[0])
    for x in terms:
        tot, mag = tot + x, mag + np.abs(x)
    return tot, (len(terms) + 2) * D24 * mag


def proj_grad_ref(dp0, z, wscale):
    """dg_adam_proj_fused's gradient wscale dp0^T z [Np, K] on the operands exactly as stored, and the bound on the in-kernel dot
    product nb D24 sum |terms| (nb - 1 fp32 additions, one rounding for a product or the final scaling)"""
    dp0, z = f64(dp0), f64(z)
    nb = dp0.shape[0]
    return w32(wscale) * dp0.T @ z, nb * D24 * w32(wscale) * np.abs(dp0).T @ np.abs(z)


# ---- bf16 ---------------------------------------------------------------------------------------------------------------------
def bf16_rne_bits(x32):
    """uint16 bit patterns of the round-to-nearest-even bfloat16 of float32 values (no NaN among them)"""
    b = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits16):
    return (np.asarray(bits16, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


# ---- comparison and failure reports ---------------------------------------------------------------------------------------------
def failure_report(what, bad, got, want, bound, cls=None, seg=None):
    """count, the first ten (index, class, lane, got, want, bound), histograms over class, index % 4 and segment"""
    bad, got, want, bound = (np.asarray(a).reshape(-1) for a in (bad, got, want, np.broadcast_to(bound, np.shape(want))))
    idx = np.nonzero(bad)[0]
    lines = [f"{what}: {idx.size} of {bad.size} elements outside their bound"]
    for i in idx[:10].tolist():
        c = CLASSES[int(cls.reshape(-1)[i])] if cls is not None else "-"
        lines.append(f"  (index={i}, class={c}, lane={i % 4}, got={float(got[i])!r}, want={float(want[i])!r}, bound={float(bound[i]):.3g})")
    if cls is not None:
        h = np.bincount(cls.reshape(-1)[idx], minlength=len(CLASSES))
        lines.append("  by class: " + " ".join(f"{CLASSES[k]}:{n}" for k, n in enumerate(h) if n))
    lines.append("  by index % 4: " + " ".join(f"{k}:{n}" for k, n in enumerate(np.bincount(idx % 4, minlength=4)) if n))
    if seg is not None:
        lines.append("  by segment: " + " ".join(f"{k}:{n}" for k, n in enumerate(np.bincount(np.asarray(seg).reshape(-1)[idx])) if n))
    return "\n".join(lines)


def ratio_of(got, want, bound, where=None):
    """(bad mask, largest |err| / bound); a zero bound demands equality; a NaN never passes"""
    got, want = f64(got), f64(want)
    bound = np.broadcast_to(f64(bound), want.shape)
    err = np.abs(got - want)
    bad = ~(err <= bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    q = np.where(np.isnan(got), np.inf, q)
    if where is not None:
        bad, q = bad & where, np.where(where, q, 0.0)
    return bad, float(q.max(initial=0.0))


def check(what, got, r, b, cls=None, seg=None, fail=True):
    """Hold a kernel's outputs got = {p, v, m, ema} (float32 arrays; absent keys are not compared) to the reference r within the
    bounds b.  Returns {quantity: largest |err| / bound}; raises with a report (fail = False: returns the failures as text under
    the key 'failures' instead - the CPU tests ask which criterion catches a variant)."""
    out, fails = {}, []
    zero = r.p0 == 0
    items = [("v'", got.get("v"), r.v, b.v, None), ("m'", got.get("m"), r.m, b.m, None),
             ("delta", None if got.get("p") is None else -f64(got["p"]), r.delta, b.delta, zero),
             ("p'", got.get("p"), r.p, b.p, ~zero), ("ema'", got.get("ema"), r.ema, b.ema, None)]
    for name, gv, want, bound, where in items:
        if gv is None or want is None:
            continue
        bad, q = ratio_of(gv, want, bound, where)
        out[name] = q
        if bad.any():
            fails.append(failure_report(f"{what}: {name}", bad, gv, want, bound, cls, seg))
    if fails and fail:
        raise AssertionError("\n".join(fails))
    if not fail:
        out["failures"] = fails
    return out


def check_class_facts(what, got, inp, hp, has_ema):
    """what the table of classes promises bit for bit: padding (g = v = 0): p unchanged, v' == 0, ema unchanged at d = 1, no NaN;
    idle (g = 0, m = 0): p unchanged"""
    for k, a in got.items():
        assert a is None or not np.isnan(a).any(), f"{what}: NaN in {k}"
    pad, idle = inp.cls == 0, inp.cls == 1
    still = pad | idle if inp.m is None or hp.b1 == 0 else pad | (idle & (inp.m == 0))
    assert np.array_equal(got["p"][still].view(np.uint32), inp.p[still].view(np.uint32)), f"{what}: p moved where g = 0"
    assert not got["v"][pad].any(), f"{what}: v' != 0 on padding"
    if has_ema and hp.d == 1.0:
        assert np.array_equal(got["ema"][pad].view(np.uint32), inp.ema[pad].view(np.uint32)), f"{what}: ema moved on padding at d = 1"


def check_shadow(what, shadow_bits, p_got, bf16):
    """the shadow is the RNE bf16 of the kernel's own p' (uint16 bits), or its very bits in fp32 mode (uint32 bits)"""
    want = bf16_rne_bits(p_got) if bf16 else np.ascontiguousarray(p_got, dtype=np.float32).view(np.uint32)
    bad = np.asarray(shadow_bits).reshape(-1) != want.reshape(-1)
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"{what}: shadow differs from the rounded master in {int(bad.sum())} of {bad.size} elements, first at "
                             f"index {i} (lane {i % 4}): got bits {int(np.asarray(shadow_bits).reshape(-1)[i]):#x}, want "
                             f"{int(want.reshape(-1)[i]):#x}")


def scale_interval(x, row_got):
    """[lo, hi] per row that holds the row scale a kernel divided by, read back from its output where the Adam step is zero (the
    table's rows 0 and num_step: x' = x exactly): row = RN(x / scale) is within 0.5 u(row) of x / scale for every element, so the
    scale lies in the intersection of |x| / (|row| + 0.5 u) .. |x| / (|row| - 0.5 u) - with a hundred elements a fraction of an ulp"""
    x, row = np.abs(f64(x)), np.abs(f64(row_got))
    h = 0.5 * u(row)
    ok = (x > 0) & (row > h)
    lo = np.where(ok, x / np.where(ok, row + h, 1.0), 0.0).max(axis=1, keepdims=True)
    hi = np.where(ok, x / np.where(ok, row - h, 1.0), np.inf).min(axis=1, keepdims=True)
    return lo, hi


def check_sphere(what, got, r, b, cls=None, fail=True):
    """dg_sphere_adam's stored m, v and renormalised latent; where the step size is zero also the row scale itself ('scale': the
    distance of scale_interval's midpoint from the reference over rel_scale; the interval must meet the reference's)"""
    out, fails = {}, []
    if r.S == 0.0:
        lo, hi = scale_interval(r.p0, got["latent"])
        tol = b.rel_scale * r.scale
        miss = (lo > r.scale + tol) | (hi < r.scale - tol) | (lo > hi)
        out["scale"] = float((np.abs(0.5 * (lo + hi) - r.scale) / tol)[np.isfinite(hi)].max(initial=0.0))
        if miss.any():
            i = int(np.nonzero(miss.reshape(-1))[0][0])
            fails.append(f"{what}: row scale outside its bound in {int(miss.sum())} rows, first row {i}: the kernel divided by a value in "
                         f"[{float(lo.reshape(-1)[i])!r}, {float(hi.reshape(-1)[i])!r}], want {float(r.scale.reshape(-1)[i])!r} "
                         f"+- {float(tol.reshape(-1)[i]):.3g}")
    for name, gv, want, bound in (("v'", got["v"], r.v, b.v), ("m'", got["m"], r.m, b.m), ("row", got["latent"], r.row, b.row)):
        bad, q = ratio_of(gv, want, bound)
        out[name] = q
        if bad.any():
            fails.append(failure_report(f"{what}: {name}", bad, gv, want, bound, cls))
    if fails and fail:
        raise AssertionError("\n".join(fails))
    if not fail:
        out["failures"] = fails
    return out


# ---- the figures the tests print ------------------------------------------------------------------------------------------------
RATIOS = {}


def note(kernel, t, ratios):
    """keep the largest ratio per (kernel, t, quantity); format_ratios() prints the table"""
    slot = RATIOS.setdefault((kernel, t), {})
    for k, q in ratios.items():
        if k != "failures":
            slot[k] = max(slot.get(k, 0.0), q)


def format_ratios(kernel=None):
    cols = ("v'", "m'", "delta", "p'", "ema'", "row", "scale")
    lines = ["kernel | t | " + " | ".join(cols)]
    for (kn, t), slot in sorted(RATIOS.items(), key=lambda kv: (kv[0][0], kv[0][1])):
        if kernel is None or kn == kernel:
            lines.append(f"{kn} | {t} | " + " | ".join(f"{slot[c]:.3f}" if c in slot else "-" for c in cols))
    return "\n".join(lines)
