"""tests/exact_util.py on the CPU: the integer references are integers and are the oracle's maps, the densities keep every case
inside the two conditions the criteria need, the neighbour function is right at the edges - and the written proof of the gap:
every mutant an almost-right kernel produces fails the per-element comparators, while the local ones pass the whole-tensor
norm of tests/test_gpu_ops.py::test_down_fwd_bwd_wgrad on the same shape."""
import math

import pytest
import torch

from oracle import dusty_oracle as O
from tests import exact_util as X
from tests.golden_util import rel_l2

BF, F32 = torch.bfloat16, torch.float32
TOLBF = 2e-2          # tests/test_gpu_ops.py: the bf16 tolerance of test_down_fwd_bwd_wgrad
SHAPE = (256, 128, 4, 128, 2)   # (Ci, Co, H, W, B): the Down case of the issue's table


def _integer(t, unit):
    return torch.equal(t / unit, (t / unit).round())


# ---- the references ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.layer_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_layer_references_are_integers_within_both_conditions(case):
    lay = X.Layer(*case)
    for q in (lay.q_fwd, lay.q_bwd, lay.dw(1.0), lay.dw(0.5, lay.rs) * 4):
        assert _integer(q, 1.0)
    assert _integer(lay.fwd_linear(), X.LIN_SCALE) and _integer(lay.q_fwd * X.FWD_SCALE + lay.b.view(1, -1, 1, 1), X.FWD_SCALE)
    assert float(lay.dw(1.0).abs().max()) < 2 ** 22
    # (a) the integer pre-activation of every pass stays within Q_MAX (asserted for every case; the bf16 ones need it)
    for name, p in zip(("lrelu", "linear", "backward"), lay.units()):
        assert float(p.abs().max()) <= X.Q_MAX, (name, float(p.abs().max()))
    # (b) forward outputs: some exact zeros (they pin `v > 0` and the saved mask on ties), at most 10 %
    for out in (lay.fwd_lrelu(), lay.fwd_linear()):
        z = float((out == 0).double().mean())
        assert 0 < z <= X.ZERO_FRACTION_MAX, z
    assert bool((lay.prev == 0).any()) and bool((lay.prev > 0).any()) and bool((lay.prev < 0).any())
    # bf16 holds every operand, and every EPI_LINEAR output, exactly
    for t in (lay.x, lay.w, lay.e, lay.prev, lay.fwd_linear(), lay.q_bwd * X.BWD_SCALE):
        assert torch.equal(t.bfloat16().double(), t)


@pytest.mark.parametrize("nh", [1, 2, 3])
@pytest.mark.parametrize("Hc,Wc", X.HEAD_SHAPES)
def test_head_references(nh, Hc, Wc):
    h = X.Head(nh, Hc, Wc)
    assert _integer(h.fwd(), 0.125) and _integer(h.q_bwd, 1.0) and _integer(h.dw(), 1.0)
    assert float(h.q_fwd.abs().max()) <= X.Q_MAX and float(h.q_bwd.abs().max()) <= X.Q_MAX
    assert 0 < float((h.fwd() == 0).double().mean()) <= X.ZERO_FRACTION_MAX
    # O.head of the same operands: bias unscaled, equal-lr scale on the input
    for k in range(nh):
        w = h.w[:, k:k + 1]
        want = O.head(h.x, w, h.b[k:k + 1], True)
        got = h.q_fwd[:, k:k + 1] * O.equal_lr_scale(w) + h.b[k]
        assert float((got - want).abs().max()) < 1e-12


@pytest.mark.parametrize("B,N", X.PROJ_SHAPES)
def test_proj_references(B, N):
    p = X.Proj(B, N)
    for epi in (X.EPI_LRELU, X.EPI_LINEAR):
        assert float(p.units(epi).abs().max()) <= X.Q_MAX
        assert 0 < float((p.fwd(epi) == 0).double().mean()) <= X.ZERO_FRACTION_MAX
    assert _integer(p.dw(0.5), 0.5)


@pytest.mark.parametrize("ring", [True, False])
def test_integer_maps_are_the_oracles(ring):
    """O.down / O.up = leaky-relu epilogue of (equal-lr scale) x down_q / up_q + bias; the adjoint and the weight gradient are
    autograd's of O.down / O.up.  Checked in float64 with the oracle's own scale (no power of two: this compares maps)."""
    g = X.gen(5)
    for which, fn, ofn in (("down", X.down_q, O.down), ("up", X.up_q, O.up)):
        lay = X.Layer(which, 5, 3, 4, 6, 3, ring)
        s = O.equal_lr_scale(lay.w)
        xr, wr = lay.x.clone().requires_grad_(), lay.w.clone().requires_grad_()
        bias = lay.b + 0.3                            # (no pre-activation within rounding of zero: the slopes cannot differ)
        y = ofn(xr, wr, bias, ring)
        v = lay.q_fwd * s + bias.view(1, -1, 1, 1)
        want = torch.where(v > 0, v, O.LRELU_SLOPE * v) * O.LRELU_GAIN
        assert float((y.detach() - want).abs().max()) < 1e-12
        gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        gx, gw = torch.autograd.grad(y, [xr, wr], gy)
        e = gy * (O.LRELU_SLOPE + (1.0 - O.LRELU_SLOPE) * (v > 0).double()) * O.LRELU_GAIN          # gradient w.r.t. the pre-activation
        assert float((X.adjoint_q(fn, lay.x_shape, lay.w, ring, e) * s - gx).abs().max()) < 1e-12
        assert float((X.wgrad_q(fn, lay.x, lay.w_shape, ring, e) * s - gw).abs().max()) < 1e-12 * float(gw.abs().max())


def test_epilogue_is_dg_epilogue_with_float_constants():
    q = torch.tensor([[[[-3.0, 0.0, 5.0]]]], dtype=torch.float64)
    b = torch.tensor([1.0], dtype=torch.float64)
    s2, a = float(torch.tensor(math.sqrt(2.0)).float()), float(torch.tensor(0.2).float())
    assert X.SQRT2 == s2 and X.SLOPE == a
    assert X.epilogue64(q, 0.5, X.EPI_LINEAR, b).flatten().tolist() == [-0.5, 1.0, 3.5]
    assert X.epilogue64(q, 0.5, X.EPI_LRELU, b).flatten().tolist() == [-0.5 * a * s2, 1.0 * s2, 3.5 * s2]
    aux = torch.tensor([[[[1.0, 0.0, -2.0]]]], dtype=torch.float64)
    assert X.epilogue64(q, 0.5, X.EPI_MASK, None, aux).flatten().tolist() == [-1.5 * s2, 0.0, 2.5 * (a * s2)]
    # a zero pre-activation takes the negative branch's formula and stays zero; a zero in aux takes the 0.2 slope
    f = X.epilogue_f32_foldings(q, 0.5, X.EPI_LRELU, b)
    assert len(f) == 3 and all(t.dtype == F32 for t in f) and all(float(t.flatten()[1]) == float(torch.tensor(s2).float()) for t in f)


# ---- the neighbour function ----------------------------------------------------------------------------------------------------
def test_bf16_neighbours_at_binade_edges_zero_and_negative_values():
    def nb(v, dtype=BF):
        lo, hi = X.neighbours(torch.tensor([v], dtype=torch.float64), dtype)
        return float(lo), float(hi)
    assert nb(1.0) == (1.0, 1.0) and nb(-1.0) == (-1.0, -1.0) and nb(0.0) == (0.0, 0.0)
    assert nb(1.0 + 1e-9) == (1.0, 1.0 + 2.0 ** -7)               # just above a power of two: the upper binade's spacing
    assert nb(1.0 - 1e-9) == (1.0 - 2.0 ** -8, 1.0)               # just below: the lower binade's (half as wide)
    assert nb(-1.0 - 1e-9) == (-1.0 - 2.0 ** -7, -1.0) and nb(-1.0 + 1e-9) == (-1.0, -1.0 + 2.0 ** -8)
    assert nb(2.0 - 2.0 ** -7 + 1e-9) == (2.0 - 2.0 ** -7, 2.0)    # the top of a binade
    assert nb(255.7) == (255.0, 256.0) and nb(-256.5) == (-258.0, -256.0)
    tiny = 2.0 ** -133                                            # bf16's smallest subnormal
    assert nb(1e-45) == (0.0, tiny) and nb(-1e-45) == (-tiny, 0.0)
    assert nb(1.0 + 1e-9, F32) == (1.0, 1.0 + 2.0 ** -23) and nb(-3.0 + 1e-9, F32) == (-3.0, -3.0 + 2.0 ** -22)
    # round-to-nearest lands on one of the two, for every value
    g = X.gen(1)
    v = (torch.randn(20000, generator=g, dtype=torch.float64) * 40).clamp(-300, 300)
    lo, hi = X.neighbours(v, BF)
    r = v.bfloat16().double()
    assert bool(((r == lo) | (r == hi)).all()) and bool((lo <= v).all()) and bool((v <= hi).all())
    assert bool(((hi - lo) <= X.ulp_of(v, BF)).all())
    step = torch.tensor([1.0, -1.0, 0.0, 2.0], dtype=BF)
    assert X._step(step, True).tolist() == [1.0 + 2.0 ** -7, -1.0 + 2.0 ** -8, tiny, 2.0 + 2.0 ** -6]
    assert X._step(step, False).tolist() == [1.0 - 2.0 ** -8, -1.0 - 2.0 ** -7, -tiny, 2.0 - 2.0 ** -7]


def test_comparators_accept_the_honest_roundings_and_nothing_else():
    lay = X.layer("down", *SHAPE)
    ref = lay.fwd_lrelu()
    fold = X.epilogue_f32_foldings(lay.q_fwd, X.FWD_SCALE, X.EPI_LRELU, lay.b)
    for f in fold:                                   # each fp32 order of the constants, stored as fp32 and as bf16
        X.assert_faithful(f, ref, F32, fold)
        X.assert_faithful(f.bfloat16(), ref, BF)
    X.assert_faithful(ref.bfloat16(), ref, BF)
    X.assert_exact(lay.fwd_linear().bfloat16(), lay.fwd_linear())
    lo, hi = X.neighbours(ref, BF)
    two_away = X._step(hi.bfloat16(), True)          # the next number after the upper neighbour: 1 ulp or more from ref
    with pytest.raises(AssertionError):
        X.assert_faithful(torch.where(hi > lo, two_away, hi.bfloat16()), ref, BF)
    nan = ref.bfloat16().clone()
    nan[1, 5, 2, 77] = float("nan")
    with pytest.raises(AssertionError, match=r"1 of \d+ elements wrong[\s\S]*b=1, c=5, y=2, x=77"):
        X.assert_faithful(nan, ref, BF)
    # condition (a) is what makes the criterion sharp: at |q| <= Q_MAX one unit of q always leaves the neighbours
    p = lay.units()[0]
    off = X.epilogue64(lay.q_fwd + 1, X.FWD_SCALE, X.EPI_LRELU, lay.b).bfloat16()
    lo, hi = X.neighbours(ref, BF)
    assert bool(((off.double() != lo) & (off.double() != hi)).all()) and float(p.abs().max()) <= X.Q_MAX


def test_failure_report_shows_the_pattern():
    lay = X.layer("down", *SHAPE)
    ref = lay.fwd_linear()
    got = ref.clone()
    got[1, 32:48, 3, 64:80] += 1.0                   # one 16 x 16 fragment: row 3, columns 64..79, channels 32..47, sample 1
    with pytest.raises(AssertionError) as ei:
        X.assert_exact(got.bfloat16(), ref, "fragment")
    msg = str(ei.value)
    assert "fragment: 256 of" in msg and "(b=1, c=32, y=3, x=64, got=" in msg and msg.count("(b=") == 10
    assert "by y: 3:256" in msg and "by b: 1:256" in msg
    assert "by x % 64: " + " ".join(f"{k}:16" for k in range(16)) in msg
    assert "by c % 16: " + " ".join(f"{k}:16" for k in range(16)) in msg


def test_dbias_comparator():
    lay = X.layer("down", *SHAPE)
    terms = lay.bwd_mask() * lay.rs.view(-1, 1, 1, 1)
    want = terms.sum(dim=[0, 2, 3])
    name, ratio = X.assert_dbias(want.float(), [("reference", terms)])
    assert name == "reference" and ratio < 1.0
    # fp32 summation in the worst plain order (one long running sum) stays inside the bound
    seq = torch.zeros(lay.Ci, dtype=F32)
    flat = terms.permute(1, 0, 2, 3).reshape(lay.Ci, -1).float()
    for k in range(0, flat.shape[1], 1):
        seq = seq + flat[:, k]
    X.assert_dbias(seq, [("reference", terms)])
    # one workgroup's partial (one sample's row of 128 pixels) missing from ONE channel: passes 5e-2 rel-L2, fails here
    miss = want.clone()
    miss[37] -= terms[0, 37, 2, :128].sum()
    assert rel_l2(miss, want) < 5e-2
    with pytest.raises(AssertionError, match=r"wrong in 1 of 256 channels[\s\S]*\(c=37,"):
        X.assert_dbias(miss.float(), [("reference", terms)])
    # a channel without non-zero terms must come out exactly zero
    z = torch.zeros(1, 2, 1, 4, dtype=torch.float64)
    z[0, 1, 0, 2] = 3.0
    X.assert_dbias(torch.tensor([0.0, 3.0]), [("t", z)])
    with pytest.raises(AssertionError):
        X.assert_dbias(torch.tensor([1e-30, 3.0]), [("t", z)])


# ---- sensitivity: the mutants ----------------------------------------------------------------------------------------------------
def _first_live_tap(x, b, y, x0, ring=True):
    """a tap of Down's output pixel (b, y, x0) under which some input channel is non-zero"""
    xp = O.pad_ring(x[b:b + 1], ring)[0]
    for ky in range(4):
        for kx in range(4):
            if bool(xp[:, 2 * y + ky, 2 * x0 + kx].any()):
                return ky, kx
    raise AssertionError("no live tap")


def _normal_recipe():
    """operands and output of tests/test_gpu_ops.py::test_down_fwd_bwd_wgrad for SHAPE in bf16 (same seed, same draws)"""
    Ci, Co, H, W, B = SHAPE
    g = torch.Generator().manual_seed(Ci * 1000 + Co + H)
    x = torch.randn(B, Ci, 2 * H, 2 * W, generator=g).bfloat16().double()
    w = torch.randn(Co, Ci, 4, 4, generator=g).bfloat16().double()
    b = torch.randn(Co, generator=g).double()
    return x, w, b, 1.0 / math.sqrt(Ci * 16)


def _lrelu(q, s, b):
    return X.epilogue64(q, s, X.EPI_LRELU, b)


LOCAL = ["tap_one_pixel", "tap_one_fragment", "channels_swapped", "slope_flipped"]
WIDE = ["neighbour_column", "wrong_sample_segment"]


def _forward_mutant(name, q, x, w, pos):
    b, y, x0 = pos
    if name == "tap_one_pixel":
        return X.mutant_tap_dropped(q, x, w, True, b, y, x0, *_first_live_tap(x, b, y, x0))
    if name == "tap_one_fragment":                   # 16 pixels x 16 channels of one MFMA fragment miss a tap
        return X.mutant_tap_dropped(q, x, w, True, b, y, x0, 1, 2, channels=slice(32, 48), pixels=16)
    if name == "channels_swapped":
        return X.mutant_channels_swapped(q, b, y, x0, 33, 38)
    if name == "neighbour_column":
        return X.mutant_neighbour_column(q, b, y, x0)
    if name == "wrong_sample_segment":
        return X.mutant_wrong_sample_segment(q, b, 1 - b, y, 64)
    raise KeyError(name)


@pytest.mark.parametrize("name", LOCAL + WIDE)
def test_forward_mutants_fail_the_comparators_and_local_ones_pass_rel_l2(name):
    lay = X.layer("down", *SHAPE)
    pos = (1, 2, 80)
    ref_lin, ref_act = lay.fwd_linear(), lay.fwd_lrelu()
    if name == "slope_flipped":
        v = lay.q_fwd * X.FWD_SCALE + lay.b.view(1, -1, 1, 1)
        c = int((v[1, :, 2, 80] < 0).nonzero()[0])
        mut_act, mut_lin = X.mutant_slope_flipped(ref_act, v, v, 1, c, 2, 80), None
    else:
        qm = _forward_mutant(name, lay.q_fwd, lay.x, lay.w, pos)
        assert not torch.equal(qm, lay.q_fwd)
        mut_lin = X.epilogue64(qm, X.LIN_SCALE, X.EPI_LINEAR, lay.b)
        mut_act = _lrelu(qm, X.FWD_SCALE, lay.b)
    fold = X.epilogue_f32_foldings(lay.q_fwd, X.FWD_SCALE, X.EPI_LRELU, lay.b)
    with pytest.raises(AssertionError, match="elements wrong"):
        X.assert_faithful(mut_act.bfloat16(), ref_act, BF)
    with pytest.raises(AssertionError, match="elements wrong"):
        X.assert_faithful(mut_act.float(), ref_act, F32, fold)
    if mut_lin is not None:
        with pytest.raises(AssertionError, match="elements wrong"):
            X.assert_exact(mut_lin.bfloat16(), ref_lin)
    # the same mutant under today's recipe and norm
    x, w, b, s = _normal_recipe()
    q = X.down_q(x, w, True)
    y = _lrelu(q, s, b)
    if name == "slope_flipped":
        v = q * s + b.view(1, -1, 1, 1)
        ym = X.mutant_slope_flipped(y, v, v, 1, int(v[1, :, 2, 80].argmin()), 2, 80)   # the most negative channel: the worst flip
    else:
        ym = _lrelu(_forward_mutant(name, q, x, w, pos), s, b)
    r = rel_l2(ym.bfloat16().double(), y)
    print(f"mutant {name}: rel-L2 under test_down_fwd_bwd_wgrad's recipe = {r:.4g} (tolerance {TOLBF})")
    if name in LOCAL:
        assert 1e-4 < r < TOLBF, r                   # today's norm lets it through


@pytest.mark.parametrize("last", [False, True], ids=["P==1", "P==Nf-2"])
def test_adjoint_extra_tap_mutant_fails(last):
    lay = X.layer("down", *SHAPE)
    qm = X.mutant_adjoint_extra_tap_dropped(lay.q_bwd, lay.e, lay.w, 1, 64, last=last)
    assert not torch.equal(qm, lay.q_bwd)
    mut = X.epilogue64(qm, X.BWD_SCALE, X.EPI_MASK, None, lay.prev)
    with pytest.raises(AssertionError, match=r"by y: %d:\d+\n" % (2 * SHAPE[2] - 2 if last else 1)):
        X.assert_faithful(mut.bfloat16(), lay.bwd_mask(), BF)
    # the bias gradient sees it too
    terms = lay.bwd_mask() * lay.rs.view(-1, 1, 1, 1)
    with pytest.raises(AssertionError):
        X.assert_dbias((mut * lay.rs.view(-1, 1, 1, 1)).sum(dim=[0, 2, 3]).float(), [("reference", terms)])


def test_masked_slope_flip_mutant_fails():
    lay = X.layer("down", *SHAPE)
    v = lay.q_bwd * X.BWD_SCALE
    c = int((v[0, :, 3, 9] != 0).nonzero()[0])
    mut = X.mutant_slope_flipped(lay.bwd_mask(), v, lay.prev, 0, c, 3, 9)
    with pytest.raises(AssertionError, match=r"1 of \d+ elements wrong"):
        X.assert_faithful(mut.bfloat16(), lay.bwd_mask(), BF)


@pytest.mark.parametrize("which", ["down", "up"])
def test_split_k_partial_mutant_fails(which):
    lay = X.layer(which, *SHAPE)
    dw = lay.dw(0.5, lay.rs)
    X.assert_exact(dw.float(), dw)
    mut = X.mutant_split_k_partial_missing(dw, lay, 0.5, 6, 1)
    with pytest.raises(AssertionError, match=r"by b: 6:\d+"):         # weight gradients report the tap as b
        X.assert_exact(mut.float(), dw)
    r = rel_l2(mut, dw)
    print(f"mutant split-K partial ({which}): rel-L2 = {r:.4g}")


def test_folded_bias_slack_admits_the_folded_epilogue_and_no_product_error():
    """The ping-pong conv's forward epilogue, emulated in IEEE fp32: fmaf(acc, scale SQRT2, fl(bias SQRT2)), max(v, 0.2f v), bf16.
    Against the plain criterion it fails at ties only (true value 0, got +-2^-23); with X.folded_bias_slack it passes; the same
    epilogue on q + 1 (one product wrong) fails at every element either way."""
    lay = X.layer("down", *SHAPE)
    ref = lay.fwd_lrelu()
    s2, a = torch.tensor(X.SQRT2, dtype=F32), torch.tensor(X.SLOPE, dtype=F32)
    bias_f = (lay.b.float() * s2).double().view(1, -1, 1, 1)              # fl(bias SQRT2)

    def folded(q):
        v = (q * (X.FWD_SCALE * X.SQRT2) + bias_f).float()              # exact in double, rounded once: the fma
        return torch.maximum(v, a * v).bfloat16()
    got = folded(lay.q_fwd)
    slack = X.folded_bias_slack(ref, lay.b)
    X.assert_faithful(got, ref, BF, None, "folded", slack)
    lo, hi = X.neighbours(ref, BF)
    bad = (got.double() != lo) & (got.double() != hi)
    assert bool(bad.any()) and bool((ref[bad] == 0).all()) and float(got[bad].abs().max()) <= 2.0 ** -22
    with pytest.raises(AssertionError, match="want=0.0"):
        X.assert_faithful(got, ref, BF)
    off = folded(lay.q_fwd + 1)
    lo2, hi2 = X.neighbours(ref - slack, BF)[0], X.neighbours(ref + slack, BF)[1]
    assert bool(((off.double() < lo2) | (off.double() > hi2)).all())


# ---- the fp32x3 mode: wide operands, the pair, the split-storage comparators ------------------------------------------------------
def test_x2_split_is_round_to_nearest_even_twice_and_the_generators_do_what_they_are_for():
    v = torch.tensor([257.0, 259.0, -257.0, 511.0, 2049.0, 4095.0, 1.0 + 2.0 ** -9, 3.0, 0.0], dtype=torch.float64)
    hi, lo = X.x2_split(v)
    assert hi.tolist() == [256.0, 260.0, -256.0, 512.0, 2048.0, 4096.0, 1.0, 3.0, 0.0]      # ties to even, both ways
    assert lo.tolist() == [1.0, -1.0, -1.0, -1.0, 1.0, -1.0, 2.0 ** -9, 0.0, 0.0]
    t = torch.tensor([1.0 + 2.0 ** -9 + 2.0 ** -17 + 2.0 ** -23], dtype=torch.float64)    # v - hi needs rounding: lo is bf16 of it
    hi, lo = X.x2_split(t)
    assert float(hi) == 1.0 and float(lo) == 2.0 ** -9 + 2.0 ** -16    # (cut toward zero: 2^-9)
    g = X.gen(3)
    a = X.wide12((200000,), 0.5, g)
    nz, opp, _ = X.wide_stats(a)
    print(f"12-bit class: lo != 0 on {nz:.1%}, opposite signs on {opp:.1%}, max |lo| {float(X.x2_split(a)[1].abs().max()):g}")
    assert nz >= 0.90 and opp >= 0.40 and float(X.x2_split(a)[1].abs().max()) <= 8
    assert 0.45 < float((a != 0).double().mean()) < 0.55 and float(a.abs()[a != 0].min()) >= 2048 and float(a.abs().max()) < 4096
    c = X.wide9((200000,), 1.0, g)
    nz, _, ties = X.wide_stats(c)
    assert nz == 1.0 and ties == 1.0 and float(c.abs().min()) >= 257 and float(c.abs().max()) <= 511
    assert bool((X.x2_split(c)[1].abs() == 1).all())
    for t in (a, c):
        hi, lo = X.x2_split(t)
        assert torch.equal(hi + lo, t)
    # the planes of a DG_BF16X2 buffer: hi at 2 i - i % 64, lo 64 further
    raw = torch.arange(512).float()
    hi, lo = X.x2_planes(raw, 256)
    assert hi[:3].tolist() == [0.0, 1.0, 2.0] and float(hi[64]) == 128.0 and float(lo[0]) == 64.0 and float(lo[65]) == 193.0
    aux = X.wide_mask_source((4, 64, 8, 8), g)
    assert 0.15 < float((aux == 0).double().mean()) < 0.25


def _layer_conditions(lay):
    cls = lay.cls
    wide = {"A": (lay.x, lay.e, lay.prev), "B": (lay.w, lay.prev), "C": (lay.x, lay.w, lay.e)}[cls]
    X.assert_wide_conditions(cls, wide, (lay.mass_fwd, lay.mass_bwd, lay.dw_mass()), (lay.fwd_lrelu(), lay.fwd_linear()),
                             lay.lolo_fwd if cls == "C" else None)
    nz, opp, _ = X.wide_stats(lay.prev)
    assert nz >= 0.90 and opp >= 0.40 and 0.1 < float((lay.prev == 0).double().mean()) < 0.3
    if cls == "B":
        X.assert_wide_conditions("B", (lay.eg,), ())
    # every result the comparators take bit for bit is an fp32 number, every operand 16 bits of hi + lo
    for t in (lay.fwd_linear(), lay.q_bwd * X.BWD_SCALE, lay.dw(0.25, lay.rs), lay.fwd_linear(full=True)):
        assert torch.equal(t.float().double(), t)
    for t in (lay.x, lay.w, lay.e, lay.prev, lay.xg, lay.eg):
        hi, lo = X.x2_split(t)
        assert torch.equal(hi + lo, t)
    if cls == "C":
        assert not torch.equal(lay.q_fwd, lay.q_fwd_full) and not torch.equal(lay.q_bwd, lay.q_bwd_full)
        assert not torch.equal(lay.dw(1.0), lay.dw(1.0, full=True)) or float(lay.dw(1.0).abs().max()) == 0
    else:
        assert torch.equal(lay.q_fwd, lay.q_fwd_full) and torch.equal(lay.q_bwd, lay.q_bwd_full)
    return float(max(lay.mass_fwd.max(), lay.mass_bwd.max())), float(lay.dw_mass().max())


WIDE_LAYER_CASES = ([(w,) + s for w in ("down", "up") for s in X.MFMA_SHAPES] + X.x2_layer_cases())


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("case", WIDE_LAYER_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_wide_layer_references_stay_exact_and_carry_low_halves(case, cls):
    """conditions (b), (c), (d) for every layer tests/test_gpu_x2_exact.py launches, on the reference alone"""
    m, mw = _layer_conditions(X.Layer(*case, True, cls=cls))
    print(f"class {cls} {case}: sum |terms| <= 2^{math.log2(m):.1f} (conv passes), 2^{math.log2(max(mw, 1)):.1f} (dW) units")


@pytest.mark.parametrize("cls", ["A", "B"])
@pytest.mark.parametrize("Hc,Wc,B", X.DOWN1_SHAPES)
def test_wide_down1_references(Hc, Wc, B, cls):
    _layer_conditions(X.Layer("down", 2, 64, Hc, Wc, B, True, cls=cls))


@pytest.mark.parametrize("cls", ["A", "B"])
@pytest.mark.parametrize("nh", [1, 2, 3])
@pytest.mark.parametrize("Hc,Wc", X.HEAD_SHAPES)
def test_wide_head_references(nh, Hc, Wc, cls):
    h = X.Head(nh, Hc, Wc, cls=cls)
    X.assert_wide_conditions(cls, {"A": (h.x, h.e, h.prev), "B": (h.w, h.prev, h.eg)}[cls], h.masses(), (h.fwd(),))
    for t in (h.fwd(), h.q_bwd * X.BWD_SCALE, h.dw(X.pow2_rowscale(h.B, 1)) * 0.5):
        assert torch.equal(t.float().double(), t)


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("B,N", X.PROJ_SHAPES)
def test_wide_proj_references(B, N, cls):
    p = X.Proj(B, N, cls=cls)
    wide = {"A": (p.z, p.e), "B": (p.w, p.eg), "C": (p.z, p.w, p.e)}[cls]
    X.assert_wide_conditions(cls, wide, (p.mass, p.dw_mass), (p.fwd(X.EPI_LRELU), p.fwd(X.EPI_LINEAR)), p.lolo if cls == "C" else None)
    assert torch.equal(p.dw(0.5).float().double(), p.dw(0.5))


def _epi(lay, epi):
    if epi == X.EPI_LINEAR:
        return lambda q: X.epilogue64(q, X.LIN_SCALE, X.EPI_LINEAR, lay.b)
    return lambda q: X.epilogue64(q, X.FWD_SCALE, X.EPI_LRELU, lay.b)


@pytest.mark.parametrize("cls", X.CLASSES)
def test_emulated_fp32x3_kernel_passes_every_new_comparator(cls):
    """float64 emulation of the three-term contraction with x2_split outputs, on the wide integer data"""
    lay = X.layer("down", *SHAPE, True, cls)
    fn = lambda a, b: X.down_q(a, b, True)
    q = X.x3_contract(fn, lay.x, lay.w)
    assert torch.equal(q, lay.q_fwd)
    hi, lo = X.x2_store(_epi(lay, X.EPI_LINEAR)(q))
    X.assert_x2_exact(hi, lo, lay.fwd_linear())
    hi, lo = X.x2_store(_epi(lay, X.EPI_LRELU)(q))
    X.assert_x2_close(hi, lo, lay.fwd_lrelu())
    assert X.x2_rel_error(hi, lo, lay.fwd_lrelu()) <= X.X2_REL
    # each order of the two constants in fp32, then the pair
    for f in X.epilogue_f32_foldings(lay.q_fwd, X.FWD_SCALE, X.EPI_LRELU, lay.b):
        X.assert_x2_close(*X.x2_split(f.double()), lay.fwd_lrelu())
    # backward-data with the wide mask source, and the weight gradient (fp32 output: the existing comparators)
    qb = X.x3_contract(lambda e, w: X.adjoint_q(X.down_q, lay.x_shape, w, True, e), lay.e, lay.w)
    assert torch.equal(qb, lay.q_bwd)
    hi, lo = X.x2_store(X.epilogue64(qb, X.BWD_SCALE, X.EPI_MASK, None, lay.prev))
    X.assert_x2_close(hi, lo, lay.bwd_mask())
    # the slope follows the hi half alone: same decision as the value itself
    assert torch.equal(X.x2_split(lay.prev)[0] > 0, lay.prev > 0)
    fold = X.epilogue_f32_foldings(lay.q_fwd, X.FWD_SCALE, X.EPI_LRELU, lay.b)
    X.assert_faithful(fold[0], lay.fwd_lrelu(), F32, fold)
    X.assert_exact(lay.dw(0.5, lay.rs).float(), lay.dw(0.5, lay.rs))
    # a non-canonical pair and a non-zero pair for a zero fail
    ref = lay.fwd_lrelu()
    hi, lo = X.x2_split(ref.float().double())
    step = X.ulp_of(hi, BF) * (ref != 0)
    with pytest.raises(AssertionError, match="hi plane is not bf16"):
        X.assert_x2_close(hi + step, lo - step, ref)
    z = torch.zeros(1, 64, 1, 1, dtype=torch.float64)
    with pytest.raises(AssertionError, match="planes of a zero"):
        X.assert_x2_close(z + 1, z - 1, z)


FAULT_CLASS = {"seam_xlo_whi_dropped": "A", "last_pixel_hi_hi_only": "A", "output_lo_truncated": "A", "lo_lo_added": "C",
               "xhi_wlo_missing_one_k_group": "B", "planes_exchanged_one_group": "A"}
FAULT_BAR = {"seam_xlo_whi_dropped": r"by x % 64: 0:\d+\n", "last_pixel_hi_hi_only": r"by y: 3:\d+\n  by x % 64: 63:\d+\n",
             "planes_exchanged_one_group": r"by c // 64: 1:\d+$"}


@pytest.mark.parametrize("name", [n for n in X.X3_FAULTS if n != "input_lo_truncated"])
def test_fp32x3_faults_fail_the_new_comparators(name):
    """each fault the rel-L2 bound of tests/test_gpu_x2.py lets through, on the class of wide data that isolates its term"""
    cls = FAULT_CLASS[name]
    lay = X.layer("down", *SHAPE, True, cls)
    hi, lo = X.x3_fault_down(name, lay.x, lay.w, _epi(lay, X.EPI_LINEAR))
    with pytest.raises(AssertionError, match="elements wrong") as ei:
        X.assert_x2_exact(hi, lo, lay.fwd_linear())
    if name in FAULT_BAR:
        import re
        assert re.search(FAULT_BAR[name], str(ei.value)), str(ei.value)
    if name == "output_lo_truncated":
        assert "[lo plane]" in str(ei.value)
        return                                       # (a cut lo is within 2^-16 |v|: the bit-for-bit linear pass is what holds it)
    hi, lo = X.x3_fault_down(name, lay.x, lay.w, _epi(lay, X.EPI_LRELU))
    with pytest.raises(AssertionError, match="elements wrong"):
        X.assert_x2_close(hi, lo, lay.fwd_lrelu())
    if name != "planes_exchanged_one_group":         # the fp32-output comparators (register split) see the accumulator faults too
        v = hi + lo
        q = X.x3_contract(lambda a, b: X.down_q(a, b, True), lay.x, lay.w)
        assert not torch.equal(v, X.x2_store(_epi(lay, X.EPI_LRELU)(q))[0] + X.x2_store(_epi(lay, X.EPI_LRELU)(q))[1])


def test_input_lo_truncation_needs_operands_of_more_than_16_bits():
    """On the wide integer data hi + lo == x, so x - hi is a bf16 number and cutting it is no fault at all: the contraction
    cannot see this one.  What holds it is the plane check in front of every launch (packed planes == x2_split) on operands that
    do need the second rounding - 24-bit integers here, as tests/test_gpu_x2_exact.py casts them."""
    lay = X.layer("down", *SHAPE, True, "A")
    hi, lo = X.x3_fault_down("input_lo_truncated", lay.x, lay.w, _epi(lay, X.EPI_LINEAR))
    X.assert_x2_exact(hi, lo, lay.fwd_linear())
    v = X.cast_probe((64, 2, 1, 64))
    whi, wlo = X.x2_split(v)
    assert bool((whi + wlo != v).any())
    cut = X.trunc_bf16(v - whi)
    assert bool((cut != wlo).any())
    with pytest.raises(AssertionError, match=r"\[lo plane\]"):
        X.assert_x2_exact(whi, cut, v)
    X.assert_x2_exact(whi, wlo, v)


def test_which_fp32x3_faults_the_rel_l2_bound_accepts():
    """The written-down justification of tests/test_gpu_x2_exact.py: every fault, under tests/test_gpu_x2.py::test_down_layer's
    recipe (randn data, its first case, Down 256 -> 128, 8 x 256 input, B = 2) and bound (rel-L2 <= 1e-4 against the full
    product) - which it accepts, and that each of them fails the per-element comparators (the tests above)."""
    Ci, Co, H, W, B = SHAPE
    g = torch.Generator().manual_seed(Ci * 1000 + Co + H)
    x = torch.randn(B, Ci, 2 * H, 2 * W, generator=g).double()
    w = torch.randn(Co, Ci, 4, 4, generator=g).double()
    b = torch.randn(Co, generator=g).double()
    s = 1.0 / math.sqrt(Ci * 16)
    epi = lambda q: X.epilogue64(q, s, X.EPI_LRELU, b)
    full = epi(X.down_q(x, w, True))
    hi, lo = X.x2_store(epi(X.x3_contract(lambda a, b_: X.down_q(a, b_, True), x, w)))
    own = rel_l2(hi + lo, full)
    rows = [("none (the contraction itself)", own, True)]
    for name in X.X3_FAULTS:
        hi, lo = X.x3_fault_down(name, x, w, epi)
        r = rel_l2(hi + lo, full)
        rows.append((name, r, r < 1e-4))
    print("\nfault                              rel-L2      test_gpu_x2.py (<= 1e-4)   per-element comparators")
    for name, r, ok in rows:
        verdict = "pass" if name.startswith("none") else ("reject (by the plane check on 24-bit operands)" if name == "input_lo_truncated" else "reject")
        print(f"{name:34s} {r:10.3g}  {'accepts' if ok else 'rejects':26s} {verdict}")
    got = dict((n, ok) for n, _, ok in rows)
    assert own < 1e-5
    for name in ("seam_xlo_whi_dropped", "last_pixel_hi_hi_only", "output_lo_truncated", "input_lo_truncated", "lo_lo_added"):
        assert got[name], name                       # the bound lets every fault of the issue's table through
