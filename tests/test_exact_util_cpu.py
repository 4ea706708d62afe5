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
