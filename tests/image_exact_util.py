"""Exact arithmetic for the image end of the discriminator: BlurVH, DiffAugment, R1's turn-around at the image and the per-sample
sums between them (csrc/blur_aug.hip, csrc/diffaug.h, the HeadGradAug gather of csrc/head_post.hip).  Imports no GPU;
tests/test_image_exact_cpu.py proves on the CPU that the data below makes every kernel value exact and that the comparators see
the defects a whole-tensor norm lets through, tests/test_gpu_image_exact.py holds the kernels to them.

Why it works.  BlurVH's taps are 1/4 and 1/2, DiffAugment's factors are 0.5 u^2 and 1 + 0.5 u^2 - dyadic for u in {0, +-0.5, +-1} -
and the contrast mean divides by H W, a power of two in every case that runs contrast.  With integer images in [-8, 8] and integer
gradients in [-4, 4] every value a kernel forms is a dyadic rational with fewer than 24 significant bits: exact in fp32 in ANY
order, with or without multiply-add contraction.  So an fp32 output must equal the float64 reference bit for bit, a bf16 output must
be its round-to-nearest-even, and every per-sample sum must be equal - also through the accumulator arena's 32.32 fixed point
(csrc/common.h), which holds every multiple of 2^-32 below 2^31.  `assert_exact_inputs` checks the premise case by case.

The references are the oracle's own maps (O.blur_vh, O.diff_augment) on float64 inputs and autograd of them.  The second half of
the file restates the same operations index by index with ONE switchable defect each (the mutants): the CPU test shows that the
restatements without a defect equal the oracle and that each defect is reported by a named case.
"""
import functools
import itertools

import torch

from oracle import dusty_oracle as O
from tests import exact_util as X

# No case can produce it: every output is smaller in magnitude (|image| <= 8, |gradient| <= 4, at most a few taps each), and
# assert_exact_inputs checks the sums.  (The 7.0 of the other GPU files is an ordinary BlurVH output of integer images.)
SENTINEL = -1024.0
GUARD = 64                                           # sentinel elements in front of and behind what a kernel owns
U_CYCLE = (0.0, 0.5, -0.5, 1.0, -1.0)
OSCALE, S_DEPTH = 0.25, 0.25                         # powers of two, never 1: the scaling is exercised
POLICIES = {
    "default": ("brightness", "saturation", "contrast", "translation", "cutout"),
    "none": (),
    "translation": ("translation",),
    "no-translation": ("brightness", "contrast", "cutout"),
    "no-contrast": ("brightness", "translation", "cutout"),   # for H W not a power of two: the contrast mean is not exact there
}


def is_pow2(n):
    return n > 0 and n & (n - 1) == 0


def policies_for(H, W):
    """contrast only where its mean is exact; the odd shapes keep the box (6 x 12 and 5 x 7 are the only odd cut_h) and the shift"""
    return ["default", "none", "translation", "no-translation"] if is_pow2(H * W) else ["none", "translation", "no-contrast"]


# ---- generators ----------------------------------------------------------------------------------------------------------------
def images(shape, g):
    return torch.randint(-8, 9, shape, generator=g).double()


def gradients(shape, g):
    return torch.randint(-4, 5, shape, generator=g).double()


def _ranges(H, W):
    sh, sw = O.translation_shift(H, W)
    ch, cw = O.cutout_size(H, W)
    return range(-sh, sh + 1), range(-sw, sw + 1), range(0, H + (1 - ch % 2)), range(0, W + (1 - cw % 2))


def _draws(rows):
    t = torch.tensor(rows, dtype=torch.long).view(-1, 4)
    return {"t_h": t[:, 0].clone(), "t_w": t[:, 1].clone(), "o_x": t[:, 2].clone(), "o_y": t[:, 3].clone()}


def all_draws(H, W):
    """every (t_h, t_w, o_x, o_y) O.draw_augment_params can produce at H x W, as one batch (8 x 16: 3 3 9 17 = 1377)"""
    return _draws(list(itertools.product(*_ranges(H, W))))


def extra_draws(H, W):
    """outside what is ever drawn, defined by the reference formula all the same: column shifts of a period and more, every row
    shifted out"""
    ox, oy = H // 2, W // 2
    return _draws([(0, tw, ox, oy) for tw in (W - 1, -(W - 1), W, -W - 3)] + [(th, 1, ox, oy) for th in (H, -H, H + 3, -(H + 3))])


def some_draws(H, W, g, n_random=8):
    """the sixteen corners of the drawable range, the out-of-range extras, a few random draws"""
    rs = _ranges(H, W)
    rows = list(itertools.product(*[(r[0], r[-1]) for r in rs]))
    rows += [tuple(int(r[int(torch.randint(0, len(r), (1,), generator=g))]) for r in rs) for _ in range(n_random)]
    d, e = _draws(rows), extra_draws(H, W)
    return {k: torch.cat([d[k], e[k]]) for k in d}


def with_factors(rp):
    """u_b, u_c cycling through U_CYCLE so that every pair of the two occurs within 25 samples"""
    B = rp["t_h"].shape[0]
    i = torch.arange(B)
    u = torch.tensor(U_CYCLE, dtype=torch.float64)
    out = dict(rp)
    out["u_b"], out["u_c"], out["u_s"] = u[i % 5], u[(i + i // 5) % 5], torch.zeros(B, dtype=torch.float64)
    return out


# ---- float64 references: the oracle's maps and autograd of them ------------------------------------------------------------------
def blur64(x, ring):
    """O.blur_vh of x [B,1,H,W] in the kernels' layout [B,H,W,2]"""
    return O.blur_vh(x, ring=bool(ring)).permute(0, 2, 3, 1).contiguous()


def blur_adj64(d, ring):
    """BlurVH^T of d [B,H,W,2] -> [B,1,H,W] (autograd of O.blur_vh, as exact_util.adjoint_q)"""
    B, H, W, _ = d.shape
    return X.adjoint_q(lambda x, w, r: O.blur_vh(x, ring=r), (B, 1, H, W), None, bool(ring), d.permute(0, 3, 1, 2).contiguous())


def aug64(x, rp, policy):
    return O.diff_augment(x, rp, POLICIES[policy])


def aug_adj64(e, rp, policy):
    """DiffAugment^T of e: the gradient of <A(x), e> with respect to x (A is affine: any x serves)"""
    xr = torch.zeros_like(e, requires_grad=True)
    (gx,) = torch.autograd.grad(aug64(xr, rp, policy), xr, e)
    return gx


def window_mask(rp, policy, H, W):
    """[B,H,W] bool: the pixels of the AUGMENTED image that come from the source image - neither cut out nor shifted in from
    outside.  Written from the reference's definition (clamped box indices, rows y + t_h inside the image), not from diffaug.h."""
    B = rp["t_h"].shape[0]
    m = torch.ones(B, H, W, dtype=torch.bool)
    ys = torch.arange(H)
    if "translation" in POLICIES[policy]:
        src = ys[None, :] + rp["t_h"][:, None]
        m &= ((src >= 0) & (src < H))[:, :, None]
    if "cutout" in POLICIES[policy]:
        ch, cw = O.cutout_size(H, W)
        for b in range(B):
            r = (torch.arange(ch) + int(rp["o_x"][b]) - ch // 2).clamp(0, H - 1)
            c = (torch.arange(cw) + int(rp["o_y"][b]) - cw // 2).clamp(0, W - 1)
            m[b, r[:, None], c[None, :]] = False
    return m


def window_sum64(e, rp, policy):
    """the contrast pivot's gradient: the sum of e [B,1,H,W] over window_mask"""
    return (e[:, 0] * window_mask(rp, policy, e.shape[2], e.shape[3])).sum(dim=[1, 2])


# ---- one shape's operands and references (cached: the CPU and the GPU file build the same objects) -------------------------------
class Blur:
    """BlurVH at H x W: integer image x [B,1,H,W], integer upstream d [B,H,W,2]"""

    def __init__(self, H, W, B=3):
        g = X.gen(424243 + 4099 * H + W)
        self.H, self.W, self.B = H, W, B
        self.x = images((B, 1, H, W), g)
        self.d = gradients((B, H, W, 2), g)

    @functools.lru_cache(maxsize=None)
    def fwd(self, ring):
        return blur64(self.x, ring)

    @functools.lru_cache(maxsize=None)
    def adj(self, ring):
        return blur_adj64(self.d, ring)

    def ssq(self, ring):
        return self.adj(ring).pow(2).sum(dim=[1, 2, 3])

    @functools.lru_cache(maxsize=None)
    def tangent(self, ring):
        """R1's turn-around: BlurVH(OSCALE BlurVH^T(d))"""
        return blur64(OSCALE * self.adj(ring), ring)


@functools.lru_cache(maxsize=None)
def blur(H, W, B=3):
    return Blur(H, W, B)


class Aug:
    """DiffAugment at H x W: draws `all` (exhaustive + the out-of-range extras) or `some`; integer image x and upstream e
    [B,1,H,W].  which = 1: the second source set of the fused forward - other images, the draws in reverse order."""

    def __init__(self, H, W, draws, which=0):
        g = X.gen(77003 + 4099 * H + W + 1000003 * which)
        self.H, self.W = H, W
        if draws == "all":
            d, e = all_draws(H, W), extra_draws(H, W)
            rp = {k: torch.cat([d[k], e[k]]) for k in d}
        else:
            rp = some_draws(H, W, X.gen(5 + H + W))
        rp = with_factors(rp)
        if which:
            rp = {k: v.flip(0).contiguous() for k, v in rp.items()}
        self.rp, self.B = rp, rp["t_h"].shape[0]
        self.x = images((self.B, 1, H, W), g)
        self.e = gradients((self.B, 1, H, W), g)
        self.xsum = self.x.sum(dim=[1, 2, 3])

    @functools.lru_cache(maxsize=None)
    def y(self, policy):
        return aug64(self.x, self.rp, policy)

    @functools.lru_cache(maxsize=None)
    def gx(self, policy, of="e"):
        """A^T(e), or A^T(BlurVH^T(d)) of the chain (of = "chain": d = the gradients of blur(H, W, B), ring columns)"""
        return aug_adj64(self.upstream(of), self.rp, policy)

    def upstream(self, of="e"):
        return self.e if of == "e" else blur(self.H, self.W, self.B).adj(True)

    @functools.lru_cache(maxsize=None)
    def gsum(self, policy, of="e"):
        return window_sum64(self.upstream(of), self.rp, policy)

    @functools.lru_cache(maxsize=None)
    def fused(self, policy, ring):
        """BlurVH(A(x)), [B,H,W,2]"""
        return blur64(self.y(policy), ring)


@functools.lru_cache(maxsize=None)
def aug(H, W, draws, which=0):
    return Aug(H, W, draws, which)


# ---- the case table: (family, H, W, draws) - what tests/test_gpu_image_exact.py runs and tests/test_image_exact_cpu.py vouches for --
BLUR_SCALAR = [(2, 5), (3, 7), (6, 10), (4, 4)]                          # W % 4 != 0 or W < 8: blur_fwd_kernel / blur_bwd_kernel
BLUR_QUAD = [(2, 8), (3, 12), (8, 16), (4, 1028), (4, 2048), (64, 1024)]  # 257 quads: a second, partial trip; 512: two full trips
BLUR_FWD = BLUR_SCALAR + BLUR_QUAD
BLUR_ADJ = BLUR_FWD + [(6, 16), (5, 8)]                                  # with 8 x 16 and 2 x 8: 4, 2, 1 and 2 rows per block
BLUR_R1SUM = [(2, 512), (3, 1024), (8, 128)]                             # dg_blur_bwd_r1: H W % 1024 == 0
TANGENT = [(4, 8), (8, 16), (4, 2048), (16, 64)]                         # 4 rows: one band, both halo rows outside the image
AUGSUM = [(8, 16, "all"), (6, 16, "all"), (5, 8, "all"), (2, 8, "all")]
AUG = [(8, 16, "all"), (4, 32, "all"), (2, 512, "some"), (16, 64, "some"), (5, 7, "some"), (6, 12, "some")]
FUSED = [(8, 16, "all"), (4, 8, "some"), (4, 2048, "some"), (16, 64, "some")]
HEAD = [(8, 16, "all"), (16, 64, "some")]                                # also the chain cases
SUM_N = [1, 7, 1024, 1025, 8192]
MEAN_N = [8, 512]                                                        # the rider mean: one trip and two of its 256-thread loop


def blur_batch(H, W):
    return 2 if H * W >= 65536 else 3


def _cases():
    out = [("blur", H, W, None) for H, W in dict.fromkeys(BLUR_ADJ + BLUR_R1SUM + TANGENT)]
    out += [("aug", H, W, d) for H, W, d in dict.fromkeys(AUG + FUSED + HEAD)]
    out += [("augsum", H, W, d) for H, W, d in AUGSUM]
    out += [("sum", 1, n, None) for n in SUM_N]
    return out


CASES = _cases()


def case_id(c):
    return "-".join(str(v) for v in c if v is not None)


def sum_rows(n, B=3):
    """dg_sample_sum's input [B, n] (an odd n misaligns the second row: the scalar path)"""
    return images((B, n), X.gen(31 + n))


def mean_src(n):
    return gradients((n,), X.gen(97 + n))


# ---- the exactness condition -------------------------------------------------------------------------------------------------
def _f32(t, what):
    assert torch.equal(t.float().double(), t), f"{what}: not exact in fp32"
    assert not bool((t == SENTINEL).any()), f"{what}: a value equals the sentinel"


def _bf16(t, what):
    assert torch.equal(t.bfloat16().double(), t), f"{what}: not exact in bf16"


def sum_is_exact(terms):
    """a per-row sum of `terms` [R, ...]: whatever the order and the tree, a partial sum is the sum of a SUBSET of the row's terms,
    so it lies between the sum of the negative terms and the sum of the positive ones and is a multiple of the terms' common unit.
    True when that keeps it below 2^24 units (fp32 adds exactly), the unit at or above 2^-32 and the magnitude below 2^31 (the
    arena's 32.32 window, csrc/common.h)."""
    t = terms.flatten(1)
    if not bool((t != 0).any()):
        return True
    unit = 2.0 ** -40
    while bool(torch.equal((t / (unit * 2)), (t / (unit * 2)).round())):
        unit *= 2
    worst = float(torch.maximum(t.clamp_min(0).sum(dim=1), (-t).clamp_min(0).sum(dim=1)).max())
    return unit >= 2.0 ** -32 and worst / unit < 2 ** 24 and worst < 2 ** 31 and torch.equal(t.sum(dim=1).float().double(), t.sum(dim=1))


def _sum_ok(terms, what):
    assert sum_is_exact(terms), f"{what}: a partial sum may not be exact"
    assert not bool((terms.flatten(1).sum(dim=1) == SENTINEL).any()), f"{what}: a sum equals the sentinel"


DBIAS_SAMPLES = 25                                    # every pair of (u_b, u_c)


def dbias_samples(a, policy, of="e"):
    """how many leading samples of a head case the bias-gradient launch takes: the most, up to DBIAS_SAMPLES, for which the sum over
    ALL their pixels is exact in any order (under contrast the pivot term (1 - cc) gsum / (H W) makes the unit fine: few samples
    at 16 x 64, all 25 at 8 x 16; without contrast the terms are integers)"""
    gx = a.gx(policy, of)
    for n in range(min(DBIAS_SAMPLES, a.B), 0, -1):
        if sum_is_exact(gx[:n].reshape(1, -1)):
            return n
    return 0


def _blur_partials(x, ring):
    """every value BlurVH's forward can form on the way to its two outputs, whatever the order of its three terms"""
    c = x
    u = torch.cat([x[:, :, 1:2], x[:, :, :-1]], dim=2)
    d = torch.cat([x[:, :, 1:], x[:, :, -2:-1]], dim=2)
    if ring:
        l, r = torch.roll(x, 1, 3), torch.roll(x, -1, 3)
    else:
        l = torch.cat([x[:, :, :, 1:2], x[:, :, :, :-1]], dim=3)
        r = torch.cat([x[:, :, :, 1:], x[:, :, :, -2:-1]], dim=3)
    out = []
    for a, b in ((u, d), (l, r)):
        out += [0.25 * a, 0.5 * c, 0.25 * b, 0.25 * a + 0.5 * c, 0.5 * c + 0.25 * b, 0.25 * a + 0.25 * b, 0.25 * a + 0.5 * c + 0.25 * b]
    return out


def _adj_partials_ok(d, what):
    """BlurVH's adjoint adds up to eight terms 0.25 d or 0.5 d per pixel: every partial sum is a multiple of 1/4 of magnitude at most
    2.5 max|d| - eleven significant bits for |d| <= 4, whatever the order"""
    assert torch.equal(d, d.round()) and float(d.abs().max()) * 2.5 * 4 < 2 ** 11, what


def assert_exact_inputs(case):
    """The premise of `bit for bit`: the reference and each intermediate of it, in the kernels' own order (csrc/diffaug.h,
    csrc/blur_aug.hip), survives .float().double() unchanged; the sums stay inside fp32's integers and the arena's window."""
    family, H, W, draws = case
    what = case_id(case)
    if family == "sum":
        x = sum_rows(W)
        _sum_ok(x, what + " sum")
        _sum_ok(x * x, what + " sum of squares")
        return
    if family == "blur":
        k = blur(H, W, blur_batch(H, W))
        _adj_partials_ok(k.d, what)
        _bf16(k.d, what + " d")
        for ring in (True, False):
            for p in _blur_partials(k.x, ring):
                _f32(p, what + " forward partial")
            _bf16(k.fwd(ring), what + " forward")
            g = k.adj(ring)
            _f32(g, what + " adjoint")
            _f32(OSCALE * g, what + " scaled adjoint")
            _f32(g * g, what + " g^2")
            _sum_ok(g * g, what + " ssq")
            _sum_ok(g, what + " gsum (any window: bounded by the sum of |g|)")
            if (H, W) in TANGENT:
                for p in _blur_partials(OSCALE * g, ring):
                    _f32(p, what + " tangent partial")
                _f32(k.ssq(ring).sum() / 4, what + " batch mean")
        for n in MEAN_N:
            _sum_ok(mean_src(n)[None], what + " rider")
        return
    a = aug(H, W, draws)
    sets = [a] + ([aug(H, W, draws, 1)] if (H, W, draws) in FUSED else [])
    HW = float(H * W)
    for s in sets:
        _sum_ok(s.x, what + " xsum")
        for policy in policies_for(H, W):
            P = POLICIES[policy]
            ub, uc = s.rp["u_b"].view(-1, 1, 1, 1), s.rp["u_c"].view(-1, 1, 1, 1)
            br = 0.5 * ub * ub if "brightness" in P else torch.zeros_like(ub)
            cc = 1 + 0.5 * uc * uc if "contrast" in P else torch.ones_like(uc)
            steps = [br, cc, s.x + br]
            if "contrast" in P:
                assert is_pow2(H * W) and H * W <= 2 ** 13, what
                mean = s.xsum.view(-1, 1, 1, 1) / HW + br
                steps += [s.xsum / HW, mean, (s.x + br) - mean, cc * ((s.x + br) - mean), mean + cc * ((s.x + br) - mean)]
            for t in steps + [s.y(policy)]:
                _f32(t, what + " " + policy + " forward")
            for of in (("e", "chain") if s is a and (H, W, draws) in HEAD else ("e",)):
                up, gsum, gx = s.upstream(of), s.gsum(policy, of), s.gx(policy, of)
                _sum_ok(up, what + " gsum")
                gm = (1 - cc.view(-1)) * gsum / HW
                g2 = (gx - gm.view(-1, 1, 1, 1)) / cc                       # the gathered gradient before the contrast factor
                for t in (gsum, (1 - cc.view(-1)) * gsum, gm, g2, cc * g2, gx, S_DEPTH * gx):
                    _f32(t, what + " " + policy + " adjoint " + of)
            if s is a and (H, W, draws) not in FUSED:
                continue
            for ring in (True, False):
                for p in _blur_partials(s.y(policy), ring):
                    _f32(p, what + " " + policy + " fused partial")
    if family == "augsum":
        k = blur(H, W, a.B)
        _adj_partials_ok(k.d, what)
        for ring in (True, False):
            _f32(k.adj(ring), what)
            _sum_ok(k.adj(ring), what + " window sum")
    if (H, W, draws) in HEAD:
        _adj_partials_ok(blur(H, W, a.B).d, what)


# ---- comparators -------------------------------------------------------------------------------------------------------------
def as4(t):
    """[B,C,Y,X] for the report: BlurVH's maps [B,H,W,2] channel first, per-sample sums [B] as [B,1,1,1]"""
    if t.ndim == 4 and t.shape[3] == 2 and t.shape[1] != 1:
        return t.permute(0, 3, 1, 2)
    if t.ndim == 1:
        return t.view(-1, 1, 1, 1)
    return X._as4(t)


def failure_report(bad, got, want, what=""):
    """exact_util.failure_report plus the histograms that name this file's defects: x % 4 (a quad's edge) and x itself (a border
    column, the wrap at W - 1, a trip of the 256-thread loop)"""
    bad, got, want = as4(bad), as4(got), as4(want)
    idx = bad.nonzero()
    lines = [X.failure_report(bad, got, want, what)]
    for name, key in (("x % 4", idx[:, 3] % 4), ("x", idx[:, 3])):
        h = torch.bincount(key).tolist() if idx.shape[0] else []
        shown = [(k, n) for k, n in enumerate(h) if n]
        lines.append(f"  by {name}: " + " ".join(f"{k}:{n}" for k, n in shown[:40]) + (" ..." if len(shown) > 40 else ""))
    return "\n".join(lines)


def assert_exact(got, ref64, what=""):
    """exact_util.assert_exact's criterion - bit equality with the representable reference, a NaN never passes - with this file's
    report; returns the number of elements compared"""
    want = ref64.to(got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(want.double(), ref64), f"{what}: the reference is not representable in {got.dtype}"
    bad = (got != want) | torch.isnan(got)
    if bool(bad.any()):
        raise AssertionError(failure_report(bad, got, want, what))
    return got.numel()


def assert_rne(got_bf16, ref64, what=""):
    """a bf16 output must be the round-to-nearest-even of the reference (itself an fp32 number: one rounding)"""
    assert got_bf16.dtype == torch.bfloat16 and got_bf16.shape == ref64.shape, (what, got_bf16.dtype, got_bf16.shape)
    assert torch.equal(ref64.float().double(), ref64), f"{what}: the reference is not an fp32 number"
    want = ref64.float().bfloat16()
    bad = (got_bf16 != want) | torch.isnan(got_bf16)
    if bool(bad.any()):
        raise AssertionError(failure_report(bad, got_bf16, want, what))
    return got_bf16.numel()


def line(family, case, n):
    print(f"[image-exact] {family} {case}: {n} elements, all exact")


# ---- restatements, index by index, with one switchable defect each (the mutants) -----------------------------------------------
def blur_fwd_r(x, ring, defect=None):
    """BlurVH of x [B,1,H,W] -> [B,H,W,2] as blur_fwd_kernel indexes it.
    defects: replicate (mutant 1), ring_clamp (3, forward half), second_trip (12)"""
    x = x[:, 0]
    H, W = x.shape[1:]
    ys, xs = torch.arange(H), torch.arange(W)
    yu, yd = ys - 1, ys + 1
    yu[0], yd[-1] = (0, H - 1) if defect == "replicate" else (1, H - 2)
    xl, xr = xs - 1, xs + 1
    if ring:
        xl[0], xr[-1] = (0, W - 1) if defect == "ring_clamp" else (W - 1, 0)
    else:
        xl[0], xr[-1] = 1, W - 2
    v = 0.25 * x[:, yu] + 0.5 * x + 0.25 * x[:, yd]
    h = 0.25 * x[:, :, xl] + 0.5 * x + 0.25 * x[:, :, xr]
    out = torch.stack([v, h], dim=3)
    if defect == "second_trip":
        out[:, :, 1024:] = SENTINEL
    return out


def blur_adj_r(d, ring, defect=None):
    """BlurVH^T of d [B,H,W,2] -> [B,1,H,W] as blur_bwd_kernel adds it up.
    defects: no_double_row, no_double_col (mutant 2), ring_clamp (3, adjoint half)"""
    D0, D1 = d[..., 0], d[..., 1]
    H, W = D0.shape[1:]
    v = 0.5 * D0
    v[:, 1:] += 0.25 * D0[:, :-1]
    v[:, :-1] += 0.25 * D0[:, 1:]
    if defect != "no_double_row":
        v[:, 1] += 0.25 * D0[:, 0]
        v[:, H - 2] += 0.25 * D0[:, H - 1]
    h = 0.5 * D1
    if ring:
        left, right = torch.roll(D1, 1, 2), torch.roll(D1, -1, 2)
        if defect == "ring_clamp":
            left[:, :, 0], right[:, :, W - 1] = D1[:, :, 0], D1[:, :, W - 1]
        h = h + 0.25 * left + 0.25 * right
    else:
        h[:, :, 1:] += 0.25 * D1[:, :, :-1]
        h[:, :, :-1] += 0.25 * D1[:, :, 1:]
        if defect != "no_double_col":
            h[:, :, 1] += 0.25 * D1[:, :, 0]
            h[:, :, W - 2] += 0.25 * D1[:, :, W - 1]
    return (v + h)[:, None]


def _factors(rp, P, defect):
    ub, uc = rp["u_b"].double(), rp["u_c"].double()
    sq = (lambda u: u) if defect == "factor_u" else (lambda u: u * u)
    br = 0.5 * sq(ub) if "brightness" in P else torch.zeros_like(ub)
    cc = 1 + 0.5 * sq(uc) if "contrast" in P else torch.ones_like(uc)
    return br, cc


def _box(rp, H, W, defect):
    ch, cw = O.cutout_size(H, W)
    r0 = rp["o_x"] - ((ch + 1) // 2 if defect == "cut_half_up" else ch // 2) + (1 if defect == "cut_row" else 0)
    cl = rp["o_y"] - cw // 2 + (1 if defect == "cut_col" else 0)
    ys, xs = torch.arange(H)[None, :, None], torch.arange(W)[None, None, :]
    r0, cl = r0[:, None, None], cl[:, None, None]
    return (ys >= r0) & (ys < r0 + ch) & (xs >= cl) & (xs < cl + cw)


def aug_fwd_r(x, rp, policy, defect=None):
    """DiffAugment of x [B,1,H,W] as diffaug_fwd_kernel gathers it (csrc/diffaug.h).
    defects: mod_W (mutant 4), cut_row / cut_col / cut_half_up (6), row_clamp (7), pivot_no_br (8), factor_u (9)"""
    P = POLICIES[policy]
    B, _, H, W = x.shape
    br, cc = _factors(rp, P, defect)
    br, cc = br.view(-1, 1, 1), cc.view(-1, 1, 1)
    v = x[:, 0] + br
    if "contrast" in P:
        mean = x[:, 0].sum(dim=[1, 2], keepdim=True) / float(H * W) + (0 if defect == "pivot_no_br" else br)
        v = mean + cc * (v - mean)
    ys, xs = torch.arange(H)[None, :, None], torch.arange(W)[None, None, :]
    bi = torch.arange(B)[:, None, None]
    if "translation" in P:
        sy = ys + rp["t_h"][:, None, None]
        ok = torch.ones_like(sy, dtype=torch.bool) if defect == "row_clamp" else (sy >= 0) & (sy < H)
        sx = (xs + rp["t_w"][:, None, None]) % (W if defect == "mod_W" else W - 1)
        v = v[bi, sy.clamp(0, H - 1), sx] * ok
    if "cutout" in P:
        v = v * ~_box(rp, H, W, defect)
    return v[:, None]


def window_sum_r(e, rp, policy, defect=None):
    """the adjoint's window sum as diffaug_bwd_sum_kernel / blur_bwd4_kernel add it.
    defects: window_incl_cut, window_band_twice (mutant 11)"""
    P = POLICIES[policy]
    B, _, H, W = e.shape
    w = torch.ones(B, H, W, dtype=torch.float64)
    if "translation" in P:
        sy = torch.arange(H)[None, :] + rp["t_h"][:, None]
        w = w * ((sy >= 0) & (sy < H))[:, :, None]
    if "cutout" in P and defect != "window_incl_cut":
        w = w * ~_box(rp, H, W, None)
    if defect == "window_band_twice":
        w[:, :4] *= 2
    return (e[:, 0] * w).sum(dim=[1, 2])


def aug_adj_r(e, rp, policy, defect=None, gsum=None):
    """DiffAugment^T of e [B,1,H,W] in scatter form: every pixel of the augmented image inside the window sends its gradient to
    its source pixel - columns 0 and W - 1 to the SAME one under translation.
    defects: shared_col (mutant 5: the contribution of column W - 1 forgotten), and window_sum_r's through the pivot term"""
    P = POLICIES[policy]
    B, _, H, W = e.shape
    _, cc = _factors(rp, P, None)
    ys, xs = torch.arange(H)[None, :, None], torch.arange(W)[None, None, :]
    bi = torch.arange(B)[:, None, None].expand(B, H, W)
    sy, sx = ys.expand(B, H, W), xs.expand(B, H, W)
    ok = torch.ones(B, H, W, dtype=torch.bool)
    if "translation" in P:
        sy = ys + rp["t_h"][:, None, None]
        ok = ((sy >= 0) & (sy < H)).expand(B, H, W).clone()
        sx = ((xs + rp["t_w"][:, None, None]) % (W - 1)).expand(B, H, W)
        sy = sy.clamp(0, H - 1).expand(B, H, W)
        if defect == "shared_col":
            ok[:, :, W - 1] = False
    if "cutout" in P:
        ok = ok & ~_box(rp, H, W, None)
    g2 = torch.zeros(B, H, W, dtype=torch.float64)
    g2.index_put_((bi[ok], sy[ok], sx[ok]), e[:, 0][ok], accumulate=True)
    if gsum is None:
        gsum = window_sum_r(e, rp, policy, defect)
    gm = (1 - cc) * gsum / float(H * W)
    return (cc.view(-1, 1, 1) * g2 + gm.view(-1, 1, 1))[:, None]


def bf16_truncated(ref64):
    """mutant 10: the fp32 value's upper 16 bits instead of its round-to-nearest-even"""
    bits = ref64.float().contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).bfloat16()
