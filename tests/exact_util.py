"""Exact arithmetic for the conv / backward-data / weight-gradient kernels: integer operands, float64 references, comparators
that look at EVERY element.  Imports no GPU; tests/test_exact_util_cpu.py proves on the CPU that the comparators see the errors
a whole-tensor norm lets through, tests/test_gpu_exact.py holds the kernels to them.

Why it works.  bf16 represents every integer up to 256, an fp32 accumulator adds integers exactly in any order (split-K, atomics,
32.32 fixed point, the fp32x3 split) as long as the sums stay below 2^24.  With activations and gradients
in {-1, 0, +1}, weights in {+-1, +-2}, integer biases and power-of-two scales, the accumulator of every kernel family is EXACT, and
the float64 result of the same operation is the one right answer for each element.

The fp32x3 mode (csrc/mfma_common.h, DG_BF16X2) splits every operand into hi = bf16(x), lo = bf16(x - hi) and contracts
x_hi w_hi + x_lo w_hi + x_hi w_lo.  The small operands above have lo = 0; the WIDE operands (`wide12`, `wide9`, classes A / B / C of
`Layer` / `Head` / `Proj`) are integers of 9 to 12 bits whose pair has a non-zero lo and hi + lo == x exactly, so each of the three
term families is an integer sum of its own, still exact in fp32 (condition (c): sum |terms| < 2^22), and the float64 value of the
DOCUMENTED contraction - sum (x w - x_lo w_lo) - is the one right answer for a matrix-core kernel, the full product sum x w for a
kernel that reads the pair through dg_ld.  `x2_split` restates the pair on the host, `x2_planes` reads the two planes of a
DG_BF16X2 buffer, `assert_x2_exact` / `assert_x2_close` hold a split-storage OUTPUT to it.

The linear maps are those of oracle/dusty_oracle.py (O.pad_ring + the convolution O.down / O.up / O.head apply to it), taken
without the equal-lr scale so that a test can pass a power of two instead; `test_exact_util_cpu.py` ties them to O.down / O.up /
O.head.  The epilogue is csrc/common.h::dg_epilogue applied in float64 with the constants as that header holds them (floats).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import dusty_oracle as O

EPI_LINEAR, EPI_LRELU, EPI_MASK = 0, 1, 2
SLOPE = float(np.float32(0.2))                      # LRELU_SLOPE 0.2f
SQRT2 = float(np.float32(1.4142135623730951))       # SQRT2 1.4142135623730951f
Q_MAX = 80                                          # condition (a): largest integer pre-activation of a bf16-output case
ZERO_FRACTION_MAX = 0.10                            # condition (b): forward outputs that are exactly zero
PRODUCTS = 48                                       # non-zero products per output element the densities aim at


# ---- generators ----------------------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


def density(taps, K, products=PRODUCTS):
    """share of non-zero activations so that `taps` tap-pixels of K channels give about `products` non-zero products: 3 per
    tap-pixel for the 16-tap passes, 12 for the 4-tap passes, dense for the two-channel thin layers"""
    return min(1.0, products / float(taps * K))


def ternary(shape, dens, g):
    """activations / gradients in {-1, 0, +1}, float64"""
    nz = torch.rand(shape, generator=g, dtype=torch.float64) < dens
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return sign * nz


def weights(shape, g):
    """dense weights in {+-1, +-2}, float64"""
    mag = torch.randint(1, 3, shape, generator=g).double()
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return mag * sign


def biases(n, g):
    return torch.randint(-3, 4, (n,), generator=g).double()


# ---- wide operands: integers whose bf16 pair has a non-zero low half ---------------------------------------------------------------
PRODUCTS_C = 3                                      # class C: 9-bit x 9-bit products (<= 2^18 each) per output element
EXACT_UNITS = 2.0 ** 22                             # condition (c): sum |terms| per output element, two bits below fp32's 2^24
X2_REL = 2.0 ** -17 * (1 + 2.0 ** -4)               # |hi + lo - ref| <= X2_REL |ref| for a non-linear split-storage output


def x2_split(v):
    """the pair of the fp32x3 mode on the host: hi = bf16(v), lo = bf16(v - hi), round-to-nearest-even twice (float64 in and out;
    v must be an fp32 number, v - hi then is one too)"""
    v32 = v.float()
    assert torch.equal(v32.double(), v), "not an fp32 number"
    hi = v32.bfloat16().float()
    lo = (v32 - hi).bfloat16().float()
    return hi.double(), lo.double()


def x2_planes(raw_bf16, n):
    """(hi, lo) of the n elements of a DG_BF16X2 buffer given as its bf16 words: hi at bf16 index 2 i - i % 64, lo 64 further
    (include/dusty_gan_hip.h; tests/test_gpu_x2.py::test_layout_and_round_trip)"""
    i = torch.arange(n)
    hi_idx = 2 * i - (i % 64)
    raw = raw_bf16.double()
    return raw[hi_idx], raw[hi_idx + 64]


def wide12(shape, dens, g):
    """12-bit magnitudes in [2^11, 2^12), random sign, non-zero with probability dens: bf16 keeps 8 bits, so hi is a multiple
    of 16 and lo = x - hi in [-8, 8] is non-zero on 15 values of 16, of the opposite sign of hi on about half"""
    nz = torch.rand(shape, generator=g, dtype=torch.float64) < dens
    mag = torch.randint(2048, 4096, shape, generator=g).double()
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return sign * mag * nz


def wide9(shape, dens, g):
    """9-bit ODD magnitudes in [257, 511]: every one is an exact tie of the bf16 rounding (spacing 2), so lo = +-1 and only
    round-to-nearest-even gives the right pair"""
    nz = torch.rand(shape, generator=g, dtype=torch.float64) < dens
    mag = 257 + 2 * torch.randint(0, 128, shape, generator=g).double()
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return sign * mag * nz


def wide_mask_source(shape, g):
    """`aux` of EPI_MASK for the split-storage kernels: 12-bit values, a fifth of them exact zeros; the kernels decide the
    slope from the hi half alone, so it must hold pairs with hi > 0 > lo and with hi < 0 < lo"""
    a = wide12(shape, 0.8, g)
    hi, lo = x2_split(a)
    assert bool((a == 0).any()) and bool(((hi > 0) & (lo < 0)).any()) and bool(((hi < 0) & (lo > 0)).any())
    return a


def cast_probe(shape, seed=77):
    """operands that DO need the pair's second rounding: signed integers of 17 to 24 bits (x - hi has up to 16 bits, one in
    256 of them an exact tie of lo's rounding), for the layout / rounding check of dg_cast"""
    g = gen(seed)
    mag = torch.randint(1 << 16, 1 << 24, shape, generator=g).double()
    return mag * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)


def wide_stats(t):
    """of the non-zero elements of t: share with lo != 0, share with hi and lo of opposite signs, share that are exact ties of
    the bf16 rounding (condition (d))"""
    v = t[t != 0]
    hi, lo = x2_split(v)
    gap = ulp_of(v, torch.bfloat16)
    return float((lo != 0).double().mean()), float((hi * lo < 0).double().mean()), float((lo.abs() * 2 == gap).double().mean())


def x3_terms(fn, x, w):
    """the three term families of the fp32x3 contraction of fn (bilinear in x, w), the dropped lo lo family, and the sum of the
    three families' absolute terms per output element (condition (c))"""
    (xh, xl), (wh, wl) = x2_split(x), x2_split(w)
    assert torch.equal(xh + xl, x) and torch.equal(wh + wl, w), "hi + lo != value"
    fams = (fn(xh, wh), fn(xl, wh), fn(xh, wl))
    mass = fn(xh.abs(), wh.abs()) + fn(xl.abs(), wh.abs()) + fn(xh.abs(), wl.abs())
    return fams, fn(xl, wl), mass


def saved_activation(shape, g):
    """`aux` of EPI_MASK: small integers, a fifth of them exact zeros (the tie of `aux > 0` and of the saved 1-bit mask)"""
    a = torch.randint(-2, 3, shape, generator=g).double()
    assert bool((a == 0).any())
    return a


def pow2_rowscale(B, shift=0):
    """per-sample weights cycling through 0.5, 1, 2"""
    return torch.tensor([(0.5, 1.0, 2.0)[(b + shift) % 3] for b in range(B)], dtype=torch.float64)


# ---- the integer linear maps (float64) -----------------------------------------------------------------------------------------
def down_q(x, w, ring=True):
    """Down's convolution without scale, bias and activation: x [B,Ci,2H,2W], w [Co,Ci,4,4] -> [B,Co,H,W] (O.down)"""
    return F.conv2d(O.pad_ring(x, ring), w, None, 2, 0)


def up_q(x, w, ring=True):
    """Up's / Head's transposed convolution likewise: x [B,Ci,H,W], w [Ci,Co,4,4] -> [B,Co,2H,2W] (O.up, O.head)"""
    return F.conv_transpose2d(O.pad_ring(x, ring), w, None, 2, 3)


def adjoint_q(fn, x_shape, w, ring, e):
    """gradient of <fn(x, w), e> with respect to x (autograd of the float64 map: integers in, integers out)"""
    xr = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
    (gx,) = torch.autograd.grad(fn(xr, w, ring), xr, e)
    return gx


def wgrad_q(fn, x, w_shape, ring, e):
    """gradient of <fn(x, w), e> with respect to w, in the weight's own layout"""
    wr = torch.zeros(w_shape, dtype=torch.float64, requires_grad=True)
    (gw,) = torch.autograd.grad(fn(x, wr, ring), wr, e)
    return gw


def epilogue64(q, scale, epi, bias=None, aux=None):
    """csrc/common.h::dg_epilogue in float64; bias per channel (dim 1)"""
    v = q * scale
    if bias is not None:
        v = v + bias.view(1, -1, *([1] * (q.ndim - 2)))
    if epi == EPI_LRELU:
        v = torch.where(v > 0, v, SLOPE * v) * SQRT2
    elif epi == EPI_MASK:
        pos = (aux > 0).double()                     # (torch.where on two Python scalars would give float32)
        v = v * (pos * SQRT2 + (1.0 - pos) * (SLOPE * SQRT2))
    return v


def epilogue_f32_foldings(q, scale, epi, bias=None, aux=None):
    """The IEEE fp32 values dg_epilogue can give, one tensor per order of its two constant factors.  acc * scale + bias is exact
    here; the positive branch multiplies once (one value); the negative branch multiplies by 0.2f and by SQRT2: (0.2f v) SQRT2 as
    written, v (0.2f SQRT2) with the constants folded (EPI_MASK is written that way), (v SQRT2) 0.2f."""
    v = q * scale
    if bias is not None:
        v = v + bias.view(1, -1, *([1] * (q.ndim - 2)))
    v32 = v.float()
    assert torch.equal(v32.double(), v), "the pre-activation is not an fp32 number"
    a, s = torch.tensor(SLOPE, dtype=torch.float32), torch.tensor(SQRT2, dtype=torch.float32)
    if epi == EPI_LINEAR:
        return [v32]
    pos = (v32 > 0) if epi == EPI_LRELU else (aux > 0)
    return [torch.where(pos, v32 * s, neg) for neg in ((a * v32) * s, v32 * (a * s), (v32 * s) * a)]


def pre_activation_units(q, scale, bias=None):
    """the integer pre-activation of condition (a): (q scale + bias) / scale.  One unit of it is one product gone wrong."""
    p = q if bias is None else q + bias.view(1, -1, *([1] * (q.ndim - 2))) / scale
    assert torch.equal(p, p.round()), "not integer-valued"
    return p


# ---- neighbours in the output type ---------------------------------------------------------------------------------------------
_BITS = {torch.bfloat16: (torch.int16, 16), torch.float32: (torch.int32, 32)}


def _step(r, up):
    """the next representable number above (up) / below each element of r, in r's dtype; the two zeros count as one number"""
    it, nb = _BITS[r.dtype]
    bits = r.contiguous().view(it).to(torch.int64) & ((1 << nb) - 1)
    sign, mag = bits >> (nb - 1), bits & ((1 << (nb - 1)) - 1)
    away = (sign == 0) if up else (sign == 1)        # moving away from zero: the magnitude grows
    zero = mag == 0
    mag2 = torch.where(zero, torch.ones_like(mag), torch.where(away, mag + 1, mag - 1))
    sign2 = torch.where(zero, torch.full_like(sign, 0 if up else 1), sign)
    out = (sign2 << (nb - 1)) | mag2
    out = torch.where(out >= (1 << (nb - 1)), out - (1 << nb), out)
    return out.to(it).view(r.dtype)


def neighbours(ref64, dtype):
    """(lo, hi) as float64: the largest number of `dtype` <= ref64 and the smallest >= ref64 (equal where ref64 is representable)"""
    r = ref64.to(dtype)
    rd = r.double()
    lo = torch.where(rd <= ref64, rd, _step(r, False).double())
    hi = torch.where(rd >= ref64, rd, _step(r, True).double())
    return lo, hi


def ulp_of(ref64, dtype):
    """spacing of `dtype` at each |ref64| (the normal-number formula; zero gets the spacing at 1)"""
    p = 8 if dtype == torch.bfloat16 else 24
    a = ref64.abs()
    e = torch.floor(torch.log2(torch.where(a > 0, a, torch.ones_like(a))))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - (p - 1))


def max_ulp_error(got, ref64, dtype):
    return float(((got.double() - ref64).abs() / ulp_of(ref64, dtype)).max())


# ---- failure reports -----------------------------------------------------------------------------------------------------------
def _as4(t):
    """[B,C,Y,X] view of a result: feature maps as they are, [B,N] GEMM rows as [B,N,1,1], weight gradients [16 or 1,Ci,Co] as
    b = tap, c = co, y = ci, x = 0"""
    if t.ndim == 4:
        return t
    if t.ndim == 2:
        return t[:, :, None, None]
    if t.ndim == 3:
        return t.permute(0, 2, 1)[:, :, :, None]
    raise ValueError(t.shape)


def failure_report(bad, got, want, what=""):
    """count of wrong elements, the first ten as (b, c, y, x, got, want), histograms over y, x % 64, c % 16, b and c // 64 - a
    row, a tile edge, a 16-channel fragment, a sample segment, a 64-channel group (or one plane of it) show as one tall bar"""
    bad, got, want = _as4(bad), _as4(got), _as4(want)
    idx = bad.nonzero()
    lines = [f"{what}: {idx.shape[0]} of {bad.numel()} elements wrong (shape b,c,y,x = {tuple(bad.shape)})"]
    for b, c, y, x in idx[:10].tolist():
        lines.append(f"  (b={b}, c={c}, y={y}, x={x}, got={float(got[b, c, y, x])!r}, want={float(want[b, c, y, x])!r})")
    for name, key in (("y", idx[:, 2]), ("x % 64", idx[:, 3] % 64), ("c % 16", idx[:, 1] % 16), ("b", idx[:, 0]),
                      ("c // 64", idx[:, 1] // 64)):
        h = torch.bincount(key).tolist() if idx.shape[0] else []
        lines.append(f"  by {name}: " + " ".join(f"{k}:{n}" for k, n in enumerate(h) if n))
    return "\n".join(lines)


# ---- comparators: every element, nothing excluded ------------------------------------------------------------------------------
def assert_exact(got, ref64, what=""):
    """bit equality with ref64 cast to got's type (the two zeros are one number; a NaN never passes).  For results that are
    representable: fp32 weight gradients, EPI_LINEAR outputs with a power-of-two scale."""
    want = ref64.to(got.dtype)
    assert torch.equal(want.double(), ref64), f"{what}: the reference is not representable in {got.dtype}"
    bad = (got != want) | torch.isnan(got)
    if bool(bad.any()):
        raise AssertionError(failure_report(bad, got, want, what))


def folded_bias_slack(ref64, bias):
    """What a forward EPI_LRELU kernel may add to the criterion when it folds sqrt 2 into the scale AND the bias - the ping-pong
    conv (csrc/conv_mfma_pp.hip: fmaf(acc, scale SQRT2, bias SQRT2), then max(v, 0.2 v)) and the weight-streaming Proj kernel
    (csrc/proj_stream.hip) do, to save a multiply per element.  scale SQRT2 is exact for a power-of-two scale, the fma rounds
    once, but bias SQRT2 is a rounded float: the pre-activation carries an ABSOLUTE error of up to 2^-24 |bias| SQRT2.  It only
    matters where acc scale and bias cancel: a pre-activation that is exactly zero comes out as +-2^-23 instead of 0 (and takes
    the slope of that sign).  The slack is that bound plus the two fp32 roundings behind it (2^-23 |ref|); one product gone
    wrong moves the value by scale SQRT2 >= 0.35, six orders of magnitude more."""
    b = bias.abs().view(1, -1, *([1] * (ref64.ndim - 2)))
    return 2.0 ** -24 * SQRT2 * b + 2.0 ** -23 * ref64.abs()


def assert_faithful(got, ref64, out_dtype, foldings=None, what="", slack=None):
    """got must be one of the two numbers of `out_dtype` next to ref64 (|got - ref64| < 1 ulp; ref64 itself where representable).
    For EPI_LRELU / EPI_MASK: sqrt 2 or 0.2 sqrt 2 is applied in fp32 in one or two roundings, then rounded to bf16.
    bf16: an fp32 value within 2^-23 of ref64 rounds to one of ref64's neighbours whichever way the kernel folded the constants,
    so the criterion absorbs every legitimate order and nothing else, PROVIDED the integer pre-activation q stays small: one unit
    of q moves the true value by |v| / |q|, which leaves the neighbours once it exceeds 1.5 ulp = 1.5 * 2^-7 |v|, i.e. for
    |q| <= 80 (Q_MAX); fp32 outputs: any |q| < 2^20.
    fp32: two fp32 roundings (0.2f v, then SQRT2) can land 2 ulp from ref64 near the top of a binade, so faithfulness alone is
    not what IEEE arithmetic promises; `foldings` (epilogue_f32_foldings: the bit patterns of the three orders of the two
    constant factors) lists what it does promise, and an element may equal any of them instead - a tighter criterion than one
    ulp, and still no error of a whole product fits through it.
    slack: see folded_bias_slack - only for the kernels named there."""
    assert got.dtype == out_dtype
    lo, hi = neighbours(ref64, out_dtype)
    g = got.double()
    ok = (g == lo) | (g == hi)
    for f in foldings or ():
        ok |= got == f.to(out_dtype)
    if slack is not None:                            # a documented absolute error of the kernel's fp32 value (folded_bias_slack):
        lo2, hi2 = neighbours(ref64 - slack, out_dtype)[0], neighbours(ref64 + slack, out_dtype)[1]
        ok |= (g >= lo2) & (g <= hi2)                # any number from the neighbour below ref - slack to the one above ref + slack
    bad = ~ok
    if bool(bad.any()):
        raise AssertionError(failure_report(bad, got, ref64, what))


def assert_x2_exact(hi, lo, ref64, what=""):
    """A split-storage (DG_BF16X2) EPI_LINEAR output: BOTH planes bit for bit the pair x2_split(ref64) - the hi plane is bf16
    (ref), the lo plane bf16(ref - hi), each rounded to nearest even; ref64 must be an fp32 number (x2_split asserts it), which
    it is when the accumulator is exact and the scale a power of two.  A wrong plane, a truncated lo, a swapped pair all fail."""
    whi, wlo = x2_split(ref64)
    for name, got, want in (("hi plane", hi, whi), ("lo plane", lo, wlo)):
        bad = (got != want) | torch.isnan(got)
        if bool(bad.any()):
            raise AssertionError(failure_report(bad, got, want, f"{what} [{name}]"))


def x2_rel_error(hi, lo, ref64):
    """largest |hi + lo - ref| / |ref| over the elements with ref != 0 (what the summary records against X2_REL)"""
    nz = ref64 != 0
    return float((((hi + lo) - ref64).abs()[nz] / ref64.abs()[nz]).max()) if bool(nz.any()) else 0.0


def assert_x2_close(hi, lo, ref64, what="", slack=None):
    """A split-storage EPI_LRELU / EPI_MASK output, per element:
      |hi + lo - ref| <= 2^-17 (1 + 2^-4) |ref| (+ slack: folded_bias_slack, for the kernels named there).
    Derivation: acc scale + bias is exact; the fp32 value v is within 3 ulp (3 x 2^-23 |v| <= 2^-21 |v| = 2^-17 2^-4 |v|) of ref
    whichever way the kernel folds 0.2f and SQRT2; hi = bf16(v) leaves |v - hi| <= 2^-8 |v|, and lo = bf16(v - hi) rounds that by
    at most half of ITS spacing, 2^-9 |v - hi| <= 2^-17 |v|.
      the pair is canonical: hi == bf16(hi + lo) wherever hi + lo is not a tie of that rounding;
      ref == 0 (outside the slack set) means both planes are zero; a NaN never passes."""
    s = hi + lo
    bound = X2_REL * ref64.abs() + (0.0 if slack is None else slack)
    bad = ((s - ref64).abs() > bound) | torch.isnan(s)
    if bool(bad.any()):
        raise AssertionError(failure_report(bad, s, ref64, f"{what} [hi + lo]"))
    zero = (ref64 == 0) & (bound == 0)
    bad = zero & ((hi != 0) | (lo != 0))
    if bool(bad.any()):
        raise AssertionError(failure_report(bad, hi, ref64, f"{what} [planes of a zero]"))
    below, above = neighbours(s, torch.bfloat16)
    nearest = torch.where(s - below < above - s, below, above)
    tie = (s - below == above - s) & (below != above)
    bad = (hi != nearest) & ~tie
    if bool(bad.any()):
        raise AssertionError(failure_report(bad, hi, nearest, f"{what} [hi plane is not bf16(hi + lo)]"))


def dbias_bound(terms64):
    """per channel: (n_nz + 1) 2^-24 sum|term| + n_nz 2^-32 over the channel's n_nz non-zero terms; terms64 [B,C,Y,X]"""
    n_nz = (terms64 != 0).sum(dim=[0, 2, 3]).double()
    return (n_nz + 1) * 2.0 ** -24 * terms64.abs().sum(dim=[0, 2, 3]) + n_nz * 2.0 ** -32


def assert_dbias(db, candidates, what=""):
    """Bias gradient, per channel: |db - sum(term)| <= (n_nz + 1) 2^-24 sum|term| + n_nz 2^-32.
    Derivation: a channel's sum is formed by fp32 additions in some order (lanes, waves, workgroups).  Adding a zero is exact, so
    only the n_nz non-zero terms cost a rounding: n_nz - 1 additions, each within 2^-24 of a partial sum that never exceeds
    sum|term|, plus one rounding when the total is stored or added onto dbias, plus one for a term formed in fp32 (v * factor)
    - n_nz + 1 in all.  On the deterministic path the cross-workgroup part of the sum is in 32.32 fixed point (common.h: dg_fix1,
    resolution 2^-32 ABSOLUTE per contribution); there are at most n_nz contributions.  The two-word form of the kernels outside
    the timed path (dg_fix2, 2^-60) is finer than either.
    `candidates`: [(name, terms64 [B,C,Y,X])] - what a kernel may legitimately sum: the fp32 values before the store, or the
    values it stored (the persistent convs sum their output strip after rounding it to bf16).  ONE candidate must hold for every
    channel.  Returns (name, worst error / bound)."""
    best, passed = None, None
    for name, terms in candidates:
        want = terms.sum(dim=[0, 2, 3])
        err, bound = (db.double() - want).abs(), dbias_bound(terms)
        bad = (err > bound) | torch.isnan(db.double())
        ratio = float(torch.where(bound > 0, err / bound.clamp_min(1e-300), (err > 0).double() * float("inf")).max())
        if not bool(bad.any()):
            if passed is None or ratio < passed[1]:
                passed = (name, ratio)               # (the candidate the kernel follows most closely names what it sums)
            continue
        if best is None or int(bad.sum()) < best[0]:
            best = (int(bad.sum()), name, bad, want, err, bound)
    if passed is not None:
        return passed
    n, name, bad, want, err, bound = best
    idx = bad.nonzero().flatten()
    lines = [f"{what}: bias gradient wrong in {n} of {db.numel()} channels (closest candidate: sum of the {name})"]
    for c in idx[:10].tolist():
        lines.append(f"  (c={c}, got={float(db[c])!r}, want={float(want[c])!r}, error={float(err[c]):.3g}, bound={float(bound[c]):.3g})")
    lines.append("  by c % 16: " + " ".join(f"{k}:{m}" for k, m in enumerate(torch.bincount(idx % 16).tolist()) if m))
    raise AssertionError("\n".join(lines))


# ---- one layer's operands and references ---------------------------------------------------------------------------------------
FWD_SCALE, LIN_SCALE, BWD_SCALE = 0.5, 0.25, 0.25   # powers of two, never 1: the scaling is exercised


class Layer:
    """Integer operands of one Down / Up layer at coarse size H x W and the float64 reference of every pass the kernels run on
    it.  Down: x [B,Ci,2H,2W] -> [B,Co,H,W]; Up: x [B,Ci,H,W] -> [B,Co,2H,2W].  All tensors float64, NCHW.
    cls (the fp32x3 mode's operand classes; None: the small operands above, low halves zero):
      "A"  wide activations, gradients and mask source (12 bit), weights in {+-1, +-2}: isolates x_lo w_hi
      "B"  ternary activations and gradients, wide weights (12 bit) and mask source: isolates x_hi w_lo
      "C"  both wide (9-bit odd, PRODUCTS_C products per output): the only class in which the documented contraction
           sum (x w - x_lo w_lo) - q_fwd / q_bwd / dw(), what a matrix-core kernel must give - differs from the full product
           q_fwd_full / q_bwd_full / dw(full=True), what a kernel that reads the pairs through dg_ld must give.
    The weight gradient contracts activations with gradients, so its operands (xg, eg) are: A  wide x, sign(e) (a_lo g_hi);
    B  ternary x, e sign x 12-bit magnitudes (a_hi g_lo); C  x and e as they are (both 9-bit).
    mass_fwd / mass_bwd: sum |terms| of the three families per output element (condition (c)); lolo_fwd: the dropped family."""

    def __init__(self, which, Ci, Co, H, W, B, ring=True, seed=0, cls=None):
        self.which, self.Ci, self.Co, self.H, self.W, self.B, self.ring, self.cls = which, Ci, Co, H, W, B, ring, cls
        g = gen(1000003 * seed + Ci * 1009 + Co * 31 + H * 7 + W + 131 * B + (0 if which == "down" else 500000) + (0 if ring else 77)
                + {None: 0, "A": 11, "B": 22, "C": 33}[cls] * 10007)
        down = which == "down"
        self.fn = down_q if down else up_q
        taps_f, taps_b = (16, 4) if down else (4, 16)
        self.x_shape = (B, Ci, 2 * H, 2 * W) if down else (B, Ci, H, W)
        self.w_shape = (Co, Ci, 4, 4) if down else (Ci, Co, 4, 4)
        act = {None: ternary, "A": wide12, "B": ternary, "C": wide9}[cls]
        wgt = {None: weights, "A": weights, "B": lambda s, g_: wide12(s, 1.0, g_), "C": lambda s, g_: wide9(s, 1.0, g_)}[cls]
        prod = PRODUCTS_C if cls == "C" else PRODUCTS
        prod_e = min(prod, 12) if cls is not None and Ci <= 4 else prod   # (Down1's dense 12-bit image: keeps dW inside (c))
        self.x = act(self.x_shape, density(taps_f, Ci, prod), g)
        self.w = wgt(self.w_shape, g)
        self.b = biases(Co, g)
        fwd = lambda x, w: self.fn(x, w, ring)
        adj = lambda e, w: adjoint_q(self.fn, self.x_shape, w, ring, e)
        self.q_fwd_full = fwd(self.x, self.w)
        self.e = act(self.q_fwd_full.shape, density(taps_b, Co, prod_e), g)  # gradient w.r.t. the pre-activation
        self.prev = saved_activation(self.x_shape, g) if cls is None else wide_mask_source(self.x_shape, g)
        self.rs = pow2_rowscale(B)
        self.q_bwd_full = adjoint_q(self.fn, self.x_shape, self.w, ring, self.e)
        self.base = torch.randint(-4, 5, (16, Ci, Co), generator=g).double()  # integer-valued dW to accumulate onto
        self.xg, self.eg = self.x, self.e
        if cls is None:
            self.q_fwd, self.q_bwd = self.q_fwd_full, self.q_bwd_full
            return
        if cls == "A":
            self.eg = self.e.sign()
        elif cls == "B":
            self.eg = self.e * torch.randint(2048, 4096, self.e.shape, generator=g).double()
        fams, self.lolo_fwd, self.mass_fwd = x3_terms(fwd, self.x, self.w)
        self.q_fwd = self.q_fwd_full - self.lolo_fwd
        assert torch.equal(fams[0] + fams[1] + fams[2], self.q_fwd)
        fams, self.lolo_bwd, self.mass_bwd = x3_terms(adj, self.e, self.w)
        self.q_bwd = self.q_bwd_full - self.lolo_bwd

    # forward passes
    def fwd_lrelu(self, full=False):
        return epilogue64(self.q_fwd_full if full else self.q_fwd, FWD_SCALE, EPI_LRELU, self.b)

    def fwd_linear(self, full=False):
        return epilogue64(self.q_fwd_full if full else self.q_fwd, LIN_SCALE, EPI_LINEAR, self.b)

    def bwd_mask(self, full=False):
        return epilogue64(self.q_bwd_full if full else self.q_bwd, BWD_SCALE, EPI_MASK, None, self.prev)

    def dw_mass(self):
        """condition (c) for the weight gradient: sum |terms| of the three families per element of dW, in units of its
        smallest term (rowscale down to 0.5 of an integer product: the largest rowscale 2 over the unit 0.5)"""
        wg = lambda x, e: wgrad_q(self.fn, x, self.w_shape, self.ring, e)
        return x3_terms(wg, self.xg, self.eg)[2] * 4

    def units(self):
        """the integer pre-activations of the three passes (condition (a))"""
        return (pre_activation_units(self.q_fwd, FWD_SCALE, self.b), pre_activation_units(self.q_fwd, LIN_SCALE, self.b),
                pre_activation_units(self.q_bwd, BWD_SCALE))

    def dw(self, scale, rowscale=None, g_mod=0, x=None, full=False):
        """weight gradient in the kernels' layout [tap][ci][co]: scale * sum_b rowscale[b] x_b (x) e_(b % g_mod), of the
        operands (xg, eg); class C: without the x_lo e_lo family unless `full`"""
        x = self.xg if x is None else x
        e = self.eg if not g_mod else self.eg[torch.arange(x.shape[0]) % g_mod]
        if rowscale is not None:
            e = e * rowscale.view(-1, 1, 1, 1)
        gw = wgrad_q(self.fn, x, self.w_shape, self.ring, e)
        if self.cls == "C" and not full:
            gw = gw - wgrad_q(self.fn, x2_split(x)[1], self.w_shape, self.ring, x2_split(e)[1])
        gw = gw * scale
        perm = (2, 3, 1, 0) if self.which == "down" else (2, 3, 0, 1)       # -> [ky][kx][ci][co]
        return gw.permute(*perm).reshape(16, self.Ci, self.Co)


@functools.lru_cache(maxsize=4)
def layer(which, Ci, Co, H, W, B, ring=True, cls=None):
    return Layer(which, Ci, Co, H, W, B, ring, cls=cls)


# ---- the cases of tests/test_gpu_exact.py (conditions (a) and (b) are asserted for each on the CPU) ---------------------------------
DIRECT_SHAPES = [(6, 4, 8, 16, 2), (5, 3, 4, 6, 3), (5, 3, 2, 6, 3)]
MFMA_SHAPES = [(64, 64, 3, 64, 3), (64, 128, 4, 128, 2), (128, 64, 2, 64, 1)]
PERSIST_SHAPES = [(128, 256, 4, 64, 8), (256, 128, 4, 128, 2), (128, 128, 2, 512, 2), (64, 128, 2, 256, 2), (512, 128, 2, 128, 2),
                  (128, 256, 3, 128, 4)]
DOWN1_SHAPES = [(2, 64, 3), (4, 128, 2)]            # (Hc, Wc, B), Ci = 2 -> Co = 64
HEAD_SHAPES = [(3, 192), (4, 256)]                  # (Hc, Wc), 64 channels -> nh = 1, 2, 3 heads
PROJ_SHAPES = [(B, N) for B in (8, 17, 32) for N in (1024, 4096)]   # K = 512


def layer_cases():
    """every (which, Ci, Co, H, W, B, ring) the GPU file builds a Layer for"""
    out = []
    for which in ("down", "up"):
        out += [(which,) + s + (ring,) for s in DIRECT_SHAPES for ring in (True, False)]
        out += [(which,) + s + (True,) for s in MFMA_SHAPES + PERSIST_SHAPES]
        out += [("down", 2, 64, hc, wc, b, True) for hc, wc, b in DOWN1_SHAPES] if which == "down" else []
    return out


# ---- the cases of tests/test_gpu_x2_exact.py (conditions (b), (c), (d) are asserted for each on the CPU) ---------------------------
CLASSES = ("A", "B", "C")
X2_SHAPES = [(256, 128, 4, 128, 2), (128, 128, 2, 512, 1), (128, 256, 4, 64, 8), (64, 128, 2, 256, 1), (64, 128, 4, 64, 8),
             (512, 128, 2, 128, 2),                # tests/test_gpu_x2.py::X2_CASES, the ping-pong conv's tile flavours
             (128, 64, 4, 128, 2),                  # Up into 64 channels (Up only)
             (128, 256, 3, 128, 4)]                 # PERSIST_SHAPES: an odd row count


def x2_layer_cases():
    """(which, Ci, Co, H, W, B) of the split-storage conv / weight-gradient tests"""
    return [(which,) + s for which in ("down", "up") for s in X2_SHAPES if which == "up" or s[1] != 64]


def assert_wide_conditions(cls, operands, masses, forward_outputs=(), lolo=None):
    """conditions (b), (c), (d) on the REFERENCE of one wide case.  operands: the wide tensors; masses: sum |terms| per output
    element of every pass; forward_outputs: forward results; lolo: class C's dropped family of the forward pass"""
    for m in masses:
        assert float(m.max()) < EXACT_UNITS, ("(c)", cls, float(m.max()))
    for out in forward_outputs:
        assert float((out == 0).double().mean()) <= ZERO_FRACTION_MAX
    for t in operands:
        nz, opp, ties = wide_stats(t)
        if cls == "C":
            assert ties == 1.0 and nz == 1.0, ("(d)", ties)
        else:
            assert nz >= 0.90 and opp >= 0.40, ("(d)", nz, opp)
    if lolo is not None:
        assert float((lolo != 0).double().mean()) >= 0.5, ("(d) lo lo", float((lolo != 0).double().mean()))


# ---- float64 emulation of the fp32x3 kernels, and the faults an almost-right one makes ---------------------------------------------
def trunc_bf16(v):
    """v (an fp32 number in float64) cut to bf16 toward zero - what a conversion without rounding gives"""
    return (v.float().contiguous().view(torch.int32) & -65536).view(torch.float32).double()


def x3_contract(fn, x, w, lo_of=None):
    """x_hi w_hi + x_lo w_hi + x_hi w_lo in float64 (fn bilinear); lo_of: how the input's low half is made (default x2_split's)"""
    (xh, xl), (wh, wl) = x2_split(x), x2_split(w)
    if lo_of is not None:
        xl = lo_of(x - xh)
    return fn(xh, wh) + fn(xl, wh) + fn(xh, wl)


def x2_store(v64, lo_of=None):
    """the pair a split-storage epilogue stores for the value v64: its fp32 rounding, split"""
    v = v64.float().double()
    hi, lo = x2_split(v)
    return hi, (lo if lo_of is None else lo_of(v - hi))


X3_FAULTS = ["seam_xlo_whi_dropped", "last_pixel_hi_hi_only", "output_lo_truncated", "input_lo_truncated", "lo_lo_added",
             "xhi_wlo_missing_one_k_group", "planes_exchanged_one_group"]


def x3_fault_down(name, x, w, epilogue):
    """(hi, lo) planes of a Down layer's split-storage output, `epilogue`(q) -> float64 values, with one fault:
    seam_xlo_whi_dropped         x_lo w_hi missing for the one W tap that wraps (kx = 0 at output column 0), that column only
    last_pixel_hi_hi_only        the last pixel of the last sample from x_hi w_hi alone
    output_lo_truncated          the output's lo cut toward zero instead of rounded to nearest even
    input_lo_truncated           the input's lo likewise
    lo_lo_added                  the full product: another contraction than the documented one
    xhi_wlo_missing_one_k_group  x_hi w_lo missing for input channels 64 .. 127
    planes_exchanged_one_group   hi and lo planes exchanged in output channels 64 .. 127"""
    fn = lambda a, b_: down_q(a, b_, True)
    (xh, xl), (wh, wl) = x2_split(x), x2_split(w)
    q = x3_contract(fn, x, w)
    if name == "seam_xlo_whi_dropped":
        wz = torch.zeros_like(wh)
        wz[:, :, :, 0] = wh[:, :, :, 0]
        q[:, :, :, 0] -= fn(xl, wz)[:, :, :, 0]
    elif name == "last_pixel_hi_hi_only":
        q[-1, :, -1, -1] = fn(xh[-1:], wh)[0, :, -1, -1]
    elif name == "input_lo_truncated":
        q = x3_contract(fn, x, w, trunc_bf16)
    elif name == "lo_lo_added":
        q = q + fn(xl, wl)
    elif name == "xhi_wlo_missing_one_k_group":
        q = q - fn(xh[:, 64:128], wl[:, 64:128])
    hi, lo = x2_store(epilogue(q), trunc_bf16 if name == "output_lo_truncated" else None)
    if name == "planes_exchanged_one_group":
        hi, lo = hi.clone(), lo.clone()
        hi[:, 64:128], lo[:, 64:128] = lo[:, 64:128].clone(), hi[:, 64:128].clone()
    return hi, lo


class Head:
    """Head (O.head): 64 channels -> nh planar fp32 maps with per-head scales passed as powers of two (DgConv.nscale), B = 2"""

    def __init__(self, nh, Hc, Wc, B=2, C0=64, cls=None):
        """cls "A": 12-bit feature map, head gradient and mask source, weights {+-1, +-2}; "B": ternary map and gradient, 12-bit
        weights and mask source (12 products per forward output: dW = sum over B Hc Wc pixels stays inside condition (c)).
        Every kernel of the Head either reads the pairs through dg_ld or, on thin_up_mfma<X2>, meets lo = 0 on one side, so
        the full product is the reference; the weight gradient's operands are (xg, eg) as in Layer."""
        g = gen(9000 + 100 * nh + Hc + Wc + {None: 0, "A": 11, "B": 22}[cls] * 10007)
        self.nh, self.Hc, self.Wc, self.B, self.C0, self.cls = nh, Hc, Wc, B, C0, cls
        act = wide12 if cls == "A" else ternary
        self.x = act((B, C0, Hc, Wc), density(4, C0, PRODUCTS if cls is None else 12), g)
        self.w = wide12((C0, nh, 4, 4), 1.0, g) if cls == "B" else weights((C0, nh, 4, 4), g)
        self.b = biases(nh, g)
        self.nscale = torch.tensor([0.5, 0.25, 0.125][:nh], dtype=torch.float64)
        self.q_fwd = up_q(self.x, self.w, True)
        self.e = act(self.q_fwd.shape, 1.0, g)                               # dense: nh * 16 products
        self.prev = saved_activation(self.x.shape, g) if cls is None else wide_mask_source(self.x.shape, g)
        self.q_bwd = adjoint_q(up_q, self.x.shape, self.w, True, self.e)
        self.xg, self.eg = self.x, self.e
        if cls == "A":
            self.eg = self.e.sign()
        elif cls == "B":
            self.eg = self.e * torch.randint(2048, 4096, self.e.shape, generator=g).double()

    def fwd(self):
        return self.q_fwd * self.nscale.view(1, -1, 1, 1) + self.b.view(1, -1, 1, 1)

    def bwd_mask(self):
        return epilogue64(self.q_bwd, BWD_SCALE, EPI_MASK, None, self.prev)

    def dw(self, rowscale=None):
        e = self.eg if rowscale is None else self.eg * rowscale.view(-1, 1, 1, 1)
        gw = wgrad_q(up_q, self.xg, self.w.shape, True, e)
        return gw.permute(2, 3, 0, 1).reshape(16, self.C0, self.nh)

    def masses(self):
        """condition (c): sum |terms| per element of the forward, the backward-data and (x 4: rowscale 2 over the unit 0.5)
        the weight-gradient pass"""
        wg = lambda x, e: wgrad_q(up_q, x, self.w.shape, True, e)
        return (up_q(self.x.abs(), self.w.abs(), True), adjoint_q(up_q, self.x.shape, self.w.abs(), True, self.e.abs()),
                wg(self.xg.abs(), self.eg.abs()) * 4)


@functools.lru_cache(maxsize=4)
def head(nh, Hc, Wc, cls=None):
    return Head(nh, Hc, Wc, cls=cls)


class Proj:
    """Proj as a GEMM (MODE_GEMM): out[b, n] = epi(scale * sum_k z[b, k] w[n, k] + bias[n % C]), K = 512"""

    def __init__(self, B, N, K=512, C=64, cls=None):
        """cls as in Layer.  q / dw(): the documented contraction (class C: without the lo lo family); the weight gradient
        dW[n][k] = sum_b e[b, n] z[b, k] contracts (eg, zg): A  sign(e), wide z; B  e sign x 12-bit magnitudes, ternary z."""
        g = gen(7000 + B + N + {None: 0, "A": 11, "B": 22, "C": 33}[cls] * 10007)
        self.B, self.N, self.K, self.C, self.cls = B, N, K, C, cls
        act = {None: ternary, "A": wide12, "B": ternary, "C": wide9}[cls]
        self.z = act((B, K), density(1, K, PRODUCTS_C if cls == "C" else PRODUCTS), g)
        self.w = {None: weights, "A": weights, "B": lambda s, g_: wide12(s, 1.0, g_), "C": lambda s, g_: wide9(s, 1.0, g_)}[cls]((N, K), g)
        self.b = biases(C, g)
        self.q = self.z @ self.w.t()
        self.e = act((B, N), 0.5, g)
        self.zg, self.eg = self.z, self.e
        if cls is None:
            return
        if cls == "A":
            self.eg = self.e.sign()
        elif cls == "B":
            self.eg = self.e * torch.randint(2048, 4096, self.e.shape, generator=g).double()
        mm = lambda z, w: z @ w.t()
        _, lolo, self.mass = x3_terms(mm, self.z, self.w)
        self.q = self.q - lolo
        self.lolo = lolo
        self.dw_mass = x3_terms(lambda e, z: e.t() @ z, self.eg, self.zg)[2]

    def _bias(self):
        return self.b.repeat(self.N // self.C)

    def fwd(self, epi):
        scale = FWD_SCALE if epi == EPI_LRELU else LIN_SCALE
        return epilogue64(self.q, scale, epi, self._bias())

    def units(self, epi):
        return pre_activation_units(self.q, FWD_SCALE if epi == EPI_LRELU else LIN_SCALE, self._bias())

    def dw(self, scale):
        """[N][K]: scale * sum_b e[b, n] z[b, k]"""
        gw = self.eg.t() @ self.zg
        if self.cls == "C":
            gw = gw - x2_split(self.eg)[1].t() @ x2_split(self.zg)[1]
        return gw * scale


@functools.lru_cache(maxsize=2)
def proj(B, N, cls=None):
    return Proj(B, N, cls=cls)


# ---- CPU mutants: the errors an almost-right kernel makes ----------------------------------------------------------------------
def tap_term_down(x, w, ring, ky, kx):
    """the contribution of tap (ky, kx) to Down's convolution, [B,Co,H,W]"""
    wz = torch.zeros_like(w)
    wz[:, :, ky, kx] = w[:, :, ky, kx]
    return down_q(x, wz, ring)


def mutant_tap_dropped(q, x, w, ring, b, y, x0, ky, kx, channels=slice(None), pixels=1):
    """`pixels` pixels from (b, y, x0) on miss tap (ky, kx) in `channels`"""
    m = q.clone()
    m[b, channels, y, x0:x0 + pixels] -= tap_term_down(x[b:b + 1], w, ring, ky, kx)[0, channels, y, x0:x0 + pixels]
    return m


def mutant_neighbour_column(q, b, y, x0):
    m = q.clone()
    m[b, :, y, x0] = q[b, :, y, x0 + 1]
    return m


def mutant_channels_swapped(q, b, y, x0, c0, c1):
    assert c0 // 16 == c1 // 16
    m = q.clone()
    m[b, c0, y, x0], m[b, c1, y, x0] = q[b, c1, y, x0], q[b, c0, y, x0]
    return m


def mutant_wrong_sample_segment(q, b, b_from, y, x0, n=64):
    m = q.clone()
    m[b, :, y, x0:x0 + n] = q[b_from, :, y, x0:x0 + n]
    return m


def mutant_adjoint_extra_tap_dropped(q_bwd, e, w, b, x0, n=64, last=False):
    """Down's backward-data (MODE_UP, adj = 1) on the reflect H axis: fine row P == 1 also receives e's row 0 through w[ky = 0]
    (dg_tap1d's tap i == 2; P == Nf - 2 receives the last row through ky = 3, i == 3).  The mutant drops it in columns
    x0 .. x0 + n of sample b.  The padded row 0 reaches no other row, so the term is the adjoint of that row and tap alone."""
    ky, row = (3, e.shape[2] - 1) if last else (0, 0)
    ez, wz = torch.zeros_like(e), torch.zeros_like(w)
    ez[:, :, row] = e[:, :, row]
    wz[:, :, ky] = w[:, :, ky]
    term = adjoint_q(down_q, q_bwd.shape, wz, True, ez)
    P = q_bwd.shape[2] - 2 if last else 1
    assert not bool(term[:, :, [r for r in range(q_bwd.shape[2]) if r != P]].any())
    m = q_bwd.clone()
    m[b, :, P, x0:x0 + n] -= term[b, :, P, x0:x0 + n]
    return m


def mutant_slope_flipped(out, v, aux_or_v, b, c, y, x0):
    """one element takes the other leaky-relu slope: out = v * (sel > 0 ? SQRT2 : SLOPE SQRT2) with the decision inverted"""
    m = out.clone()
    m[b, c, y, x0] = v[b, c, y, x0] * (SLOPE * SQRT2 if aux_or_v[b, c, y, x0] > 0 else SQRT2)
    return m


def mutant_split_k_partial_missing(dw, lay, scale, tap, b):
    """weight gradient: the partial sum over sample b is missing from one tap"""
    gw = wgrad_q(lay.fn, lay.x[b:b + 1], lay.w_shape, lay.ring, lay.e[b:b + 1]) * scale
    perm = (2, 3, 1, 0) if lay.which == "down" else (2, 3, 0, 1)
    part = gw.permute(*perm).reshape(16, lay.Ci, lay.Co)
    m = dw.clone()
    m[tap] -= part[tap]
    return m
