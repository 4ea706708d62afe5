"""The fp32x3 precision mode PER ELEMENT, with low halves that are not zero (tests/exact_util.py: the wide operand classes).

Both forms of the mode - the register split (DG_FORCE_FP32X3 on fp32 storage) and split storage (DG_BF16X2) - contract
x_hi w_hi + x_lo w_hi + x_hi w_lo.  On 12-bit and 9-bit integer operands every one of the three term families is an exact fp32
sum, so the float64 value of that contraction is the one right answer: class A (wide activations / gradients) isolates x_lo w_hi,
class B (wide weights) x_hi w_lo, class C (both 9-bit) tells the documented contraction from the full product, which is what the
kernels that read a pair through dg_ld must give instead.  fp32 outputs and weight gradients: bit for bit (X.assert_exact /
X.assert_faithful with the fp32 foldings); split-storage outputs: both planes bit for bit the pair X.x2_split(ref) under
EPI_LINEAR, |hi + lo - ref| <= 2^-17 (1 + 2^-4) |ref| with a canonical pair under EPI_LRELU / EPI_MASK (X.assert_x2_close).
tests/test_exact_util_cpu.py shows which faults of a low half these catch that the rel-L2 bound of tests/test_gpu_x2.py accepts.

All launches go through engine.Ops and the C ABI; every test asserts from engine.TRACE which family / variant ran, checks the
packed operands against X.x2_split in front of the launch (a dg_cast failure is not the conv's), and prints an `[exact]` line.
"""
import pytest
import torch

from dusty_gan_amd._lib import (DG_FORCE_DIRECT, DG_FORCE_MFMA, DG_FORCE_PINGPONG, DG_FORCE_THIN, DG_FORCE_WG_DMA_NOPAIRS,
                                DG_FORCE_WG_DMA_PAIRS, DG_FORCE_WG_REGSTAGED)
from tests import exact_util as X
from tests.test_gpu_exact import (L, NAMES, check_layer, check_proj, check_wgrad, check_wgrad_group, pick_cap,  # noqa: F401
                                  trace)
from tests.test_gpu_ops import from_nhwc, nhwc, pack_down, pack_up
from tests.test_gpu_x2 import X2_CASES, run_conv_x2, to_x2

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
assert X.X2_SHAPES[:len(X2_CASES)] == X2_CASES


def planes(t):
    """(hi, lo) of a tagged DG_BF16X2 device tensor, flat float64"""
    return X.x2_planes(t.view(torch.bfloat16).cpu().float(), t.numel())


def assert_packed(t, v64, what):
    """the packed planes of `t` are the host's pair of the values v64 (flat, in t's element order)"""
    hi, lo = planes(t)
    whi, wlo = X.x2_split(v64.reshape(-1))
    assert torch.equal(hi, whi) and torch.equal(lo, wlo), f"{what}: dg_cast's planes differ from x2_split"


def put_x2(t):
    """an NCHW float64 operand as a packed pixel-major DG_BF16X2 tensor, its planes checked"""
    flat = nhwc(t)
    d = to_x2(flat)
    assert_packed(d, flat, "operand")
    return d


def test_cast_rounds_both_halves_to_nearest_even():
    """dg_cast on operands that need the second rounding (17..24-bit integers, ties among them) - the integer operands of the
    tests below have exact low halves, which a truncating cast would get right"""
    v = X.cast_probe((7 * 192,))
    whi, wlo = X.x2_split(v)
    assert bool((whi + wlo != v).any()) and bool((X.trunc_bf16(v - whi) != wlo).any())
    assert_packed(to_x2(v), v, "24-bit integers")


# ---- register split: fp32 storage, DG_FORCE_FP32X3 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("which", ["down", "up"])
@pytest.mark.parametrize("shape", X.MFMA_SHAPES, ids=str)
def test_register_split_conv(L, trace, monkeypatch, which, shape, cls):
    """conv_mfma_kernel<float, .., X3>: forward lrelu + bias, forward linear, backward-data EPI_MASK with per-sample weights
    and the bias gradient"""
    check_layer(L, trace, monkeypatch, which, shape, True, F32, DG_FORCE_MFMA, x3=True, cls=cls)


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("which", ["down", "up"])
@pytest.mark.parametrize("force", [DG_FORCE_MFMA, DG_FORCE_WG_REGSTAGED], ids=["mfma", "wg-regstaged"])
@pytest.mark.parametrize("shape", X.MFMA_SHAPES, ids=str)
def test_register_split_weight_gradient(L, trace, which, force, shape, cls):
    """wgrad_mfma_kernel<float, .., X3>: workspace and atomics, accumulating and overwriting"""
    lay = X.layer(which, *shape, True, cls)
    check_wgrad(L, trace, lay, force, F32, True, f"{NAMES[force]} fp32x3", L.DG_WGRAD_VARIANT_MFMA)


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("B,N", X.PROJ_SHAPES)
def test_register_split_proj_gemm(L, trace, B, N, cls):
    check_proj(L, trace, X.proj(B, N, cls), DG_FORCE_MFMA, F32, True)


# ---- split storage: the ping-pong conv ---------------------------------------------------------------------------------------------
def conv_x2(L, lay, what, mode, adj, x, w_nk, N, scale, epi, force, multi, **kw):
    """one split-storage launch -> ((hi, lo), dbias or None, trace record); multi: a second launch with the workgroup cap of
    pick_cap (>= 4 tiles per workgroup, uneven chunks - asserted), whose result is the one returned"""
    def check(xd, tw, auxd):
        assert_packed(xd, nhwc(x), f"{what} input")
        assert_packed(tw, w_nk.contiguous(), f"{what} weights")
        if auxd is not None:
            assert_packed(auxd, nhwc(kw["aux"]), f"{what} mask source")
    for k in ("bias", "rowscale"):
        if kw.get(k) is not None:
            kw[k] = kw[k].float()
    rec = []
    res = run_conv_x2(L, mode, adj, x, w_nk, N, scale, epi, force, planes=True, rec=rec, check=check, **kw)
    if multi:
        cap = pick_cap(rec[0][4])
        rec = []
        res = run_conv_x2(L, mode, adj, x, w_nk, N, scale, epi, force, planes=True, rec=rec, wg_cap=cap, **kw)
        r = rec[0]
        assert r[5] <= cap, r
        if cap > 1:
            assert r[4] // r[5] >= 4 and r[4] % r[5] != 0, r                  # >= 4 tiles per workgroup, uneven chunks
        else:
            assert r[5] == 1 and r[6] == r[4], r
    assert len(rec) == 1, rec
    pl, db = res if kw.get("want_db") else (res, None)
    return pl, db, rec[0]


def check_layer_x2(L, which, shape, cls, force, multi):
    """forward lrelu + bias into a split map, forward linear into one, backward-data EPI_MASK from a split mask source with
    rowscale and dbias.  The ping-pong conv is held to the documented contraction, the direct kernel (dg_ld / dg_st on the
    same buffers, split weights included) to the full product - the same numbers in classes A and B."""
    lay = X.layer(which, *shape, True, cls)
    down = which == "down"
    full = force == DG_FORCE_DIRECT
    fmode, bmode = (L.MODE_S2, L.MODE_UP) if down else (L.MODE_UP, L.MODE_S2)
    wf, wb = (pack_down if down else pack_up)(lay.w)
    fam = f"{NAMES[force]} bf16x2"
    tag = f"{which} {shape} class {cls}" + (" several tiles per workgroup" if multi else "")
    assert max(float(lay.mass_fwd.max()), float(lay.mass_bwd.max())) < X.EXACT_UNITS      # condition (c)
    if cls != "C":
        assert torch.equal(lay.q_fwd, lay.q_fwd_full) and torch.equal(lay.q_bwd, lay.q_bwd_full)
    ref = lay.fwd_lrelu(full)
    assert float((ref == 0).double().mean()) <= X.ZERO_FRACTION_MAX                         # condition (b)
    (hi, lo), _, rec = conv_x2(L, lay, tag, fmode, 0, lay.x, wf, lay.Co, X.FWD_SCALE, L.EPI_LRELU, force, multi, bias=lay.b)
    slack = X.folded_bias_slack(ref, lay.b) if rec[1] == L.DG_CONV_FAMILY_PINGPONG else None
    X.assert_x2_close(hi, lo, ref, f"{fam} forward lrelu {tag} {rec[1:7]}", slack)
    worst = X.x2_rel_error(hi, lo, ref)
    ref = lay.fwd_linear(full)
    (hi, lo), _, rec = conv_x2(L, lay, tag, fmode, 0, lay.x, wf, lay.Co, X.LIN_SCALE, L.EPI_LINEAR, force, multi, bias=lay.b)
    X.assert_x2_exact(hi, lo, ref, f"{fam} forward linear {tag} {rec[1:7]}")
    ratio = None
    if down or lay.Co >= 128:        # (Up's backward-data contracts over Co: the ping-pong conv takes it from 128 channels on)
        ref = lay.bwd_mask(full)
        (hi, lo), db, rec = conv_x2(L, lay, tag, bmode, 1, lay.e, wb, lay.Ci, X.BWD_SCALE, L.EPI_MASK, force, multi, aux=lay.prev,
                                    rowscale=lay.rs, want_db=True)
        what = f"{fam} backward-data {tag} {rec[1:7]}"
        X.assert_x2_close(hi, lo, ref, what)
        worst = max(worst, X.x2_rel_error(hi, lo, ref))
        rs4 = lay.rs.view(-1, 1, 1, 1)
        ratio = X.assert_dbias(db, [("fp32 values", ref * rs4), ("stored values", (hi + lo) * rs4)], what)
        if down and lay.Ci == 64 and force == DG_FORCE_PINGPONG and not multi:
            assert (rec[2], rec[3]) == (512, 64), rec                    # the both-parities tile (512 pixels x 64 channels)
    print(f"[exact] {fam} {tag}: linear planes exact; worst |hi + lo - ref| / |ref| {worst:.3g} (bound {X.X2_REL:.3g})" +
          ("" if ratio is None else f"; dbias error/bound {ratio[1]:.3g} (sum of the {ratio[0]})"))


X2_LAYERS = X.x2_layer_cases()


@pytest.mark.parametrize("multi", [False, True], ids=["default-launch", "several-tiles-per-workgroup"])
@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("case", X2_LAYERS, ids=lambda c: "-".join(str(v) for v in c))
def test_split_storage_pingpong_conv(L, case, cls, multi):
    """conv_pp_kernel<.., X2>: every tile flavour of tests/test_gpu_x2.py, Up into 64 channels, an odd row count"""
    check_layer_x2(L, case[0], case[1:], cls, DG_FORCE_PINGPONG, multi)


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("case", [c for c in X2_LAYERS if c[1] * c[2] <= 128 * 128], ids=lambda c: "-".join(str(v) for v in c))
def test_direct_conv_on_split_buffers(L, case, cls):
    """dg_ld / dg_st in the direct kernels: the full product (class C: NOT the matrix cores' contraction)"""
    check_layer_x2(L, case[0], case[1:], cls, DG_FORCE_DIRECT, False)


# ---- split storage: the LDS-DMA weight gradient ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("force", [DG_FORCE_WG_DMA_PAIRS, DG_FORCE_WG_DMA_NOPAIRS], ids=["tap-pairs", "single-taps"])
@pytest.mark.parametrize("case", X2_LAYERS, ids=lambda c: "-".join(str(v) for v in c))
def test_split_storage_weight_gradient(L, trace, case, force, cls):
    """wgrad_dma_kernel<.., X2>: workspace / atomics x accumulate / overwrite, per-sample weights, the sample map"""
    lay = X.layer(case[0], *case[1:], True, cls)
    check_wgrad(L, trace, lay, force, F32, False, f"{NAMES[force]} bf16x2", L.DG_WGRAD_VARIANT_DMA,
                {DG_FORCE_WG_DMA_PAIRS: 1, DG_FORCE_WG_DMA_NOPAIRS: 0}[force], put=put_x2)


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("which", ["down", "up"])
def test_split_storage_weight_gradient_group(L, trace, which, cls):
    """one `with ops.grouped():` block of three layers (dg_wgrad_group): each dW the float64 result"""
    lays = [X.Layer(which, *s, True, cls=cls) for s in ((64, 128, 4, 128, 2), (128, 64, 2, 64, 1), (64, 64, 3, 64, 3))]
    check_wgrad_group(L, trace, lays, DG_FORCE_MFMA, F32, put_x2)
    print(f"[exact] wgrad group bf16x2 {which} class {cls}: three layers exact, grouped and single")


# ---- the network's ends: thin kernels with a split map on one side -----------------------------------------------------------------
def one(trace, n0, kind):
    recs = [t for t in trace[n0:] if t[0] == kind]
    assert len(recs) == 1, trace[n0:]
    return recs[0]


@pytest.mark.parametrize("cls", ["A", "B"])
@pytest.mark.parametrize("nh", [1, 2, 3])
@pytest.mark.parametrize("Hc,Wc", X.HEAD_SHAPES)
def test_head_on_a_split_map(L, trace, nh, Hc, Wc, cls):
    """Head forward FROM a split map on thin_up_mfma<X2> with fp32 weights (class B: wide ones, so its lo fragment table is
    read): exact.  Head backward-data INTO a split map with a split mask source and the bias gradient; Head weight gradient
    from the split map."""
    from dusty_gan_amd import engine as E
    h = X.head(nh, Hc, Wc, cls)
    B, C0, HW = h.B, h.C0, 4 * Hc * Wc
    assert all(float(m.max()) < X.EXACT_UNITS for m in h.masses())                          # condition (c)
    o = E.Ops(F32)
    o.force = DG_FORCE_THIN
    xd = put_x2(h.x)
    coci = h.w.permute(2, 3, 1, 0).contiguous().to(DEV, F32)         # forward shadow [tap][n = co][k = ci]
    cico = h.w.permute(2, 3, 0, 1).contiguous().to(DEV, F32)         # backward shadow [tap][n = ci][k = co]
    bias, nscale = h.b.to(DEV, F32), h.nscale.to(DEV, F32)
    out = torch.full((B, nh, 2 * Hc, 2 * Wc), float("nan"), device=DEV)
    n0 = len(trace)
    o.conv(L.MODE_UP, 0, True, B, Hc, Wc, C0, nh, xd, (Hc * Wc * C0, C0, 1), out, (nh * HW, 1, HW), coci.data_ptr(), 1.0,
           L.EPI_LINEAR, bias=bias.data_ptr(), bias_mod=nh, out_dt=L.DG_F32, nscale=nscale)
    torch.cuda.synchronize()
    rec = one(trace, n0, "conv")
    assert rec[1] == L.DG_CONV_FAMILY_THIN and rec[8] == 2, rec      # thin_up_mfma
    X.assert_exact(out.cpu(), h.fwd(), f"thin bf16x2 head forward nh={nh} class {cls} {rec[1:9]}")
    # backward-data: planar fp32 head gradient -> split map, split mask source
    prevd = put_x2(h.prev)
    gd = h.e.to(DEV, F32).contiguous()
    rs = X.pow2_rowscale(B)
    dp = E.tag_x2(torch.full((B * Hc * Wc * C0,), float("nan"), device=DEV))
    db = torch.zeros(C0, device=DEV)
    n0 = len(trace)
    o.conv(L.MODE_S2, 1, True, B, Hc, Wc, nh, C0, gd, (nh * HW, 1, HW), dp, (Hc * Wc * C0, C0, 1), cico.data_ptr(), X.BWD_SCALE,
           L.EPI_MASK, aux=prevd, dbias=db.data_ptr(), bias_mod=C0, in_dt=L.DG_F32, rowscale=rs.to(DEV, F32))
    torch.cuda.synchronize()
    rec = one(trace, n0, "conv")
    assert rec[1] == L.DG_CONV_FAMILY_THIN and rec[8] == 0, rec      # the VALU kernel: dg_ld on the mask source, dg_st
    hi, lo = (from_nhwc(p, B, C0, Hc, Wc) for p in planes(dp))
    ref = h.bwd_mask()
    what = f"thin bf16x2 head backward-data nh={nh} class {cls} {rec[1:9]}"
    X.assert_x2_close(hi, lo, ref, what)
    rs4 = rs.view(-1, 1, 1, 1)
    ratio = X.assert_dbias(db.cpu(), [("fp32 values", ref * rs4), ("stored values", (hi + lo) * rs4)], what)
    # weight gradient: a = the split map, g = the planar fp32 gradient
    xg, eg = put_x2(h.xg), h.eg.to(DEV, F32).contiguous()
    rs = X.pow2_rowscale(B, 1)
    dw = torch.full((16, C0, nh), float("nan"), device=DEV)
    n0 = len(trace)
    o.wgrad(1, True, B, Hc, Wc, C0, nh, xg, (Hc * Wc * C0, C0, 1), eg, (nh * HW, 1, HW), dw.data_ptr(), 0.5,
            rowscale=rs.to(DEV, F32), g_dt=L.DG_F32, accumulate=0)
    torch.cuda.synchronize()
    rec = one(trace, n0, "wgrad")
    assert rec[1] == L.DG_WGRAD_VARIANT_THIN, rec
    X.assert_exact(dw.cpu(), h.dw(rs) * 0.5, f"thin bf16x2 head weight gradient nh={nh} class {cls} {rec}")
    print(f"[exact] thin bf16x2 head nh={nh} {(Hc, Wc)} class {cls}: forward and dW exact; backward-data worst "
          f"|hi + lo - ref| / |ref| {X.x2_rel_error(hi, lo, ref):.3g} (bound {X.X2_REL:.3g}); dbias error/bound {ratio[1]:.3g} "
          f"(sum of the {ratio[0]})")


@pytest.mark.parametrize("cls", ["A", "B"])
@pytest.mark.parametrize("Hc,Wc,B", X.DOWN1_SHAPES)
def test_down1_on_a_split_map(L, trace, Hc, Wc, B, cls):
    """Down1 forward INTO a split map (the VALU kernel's x2fast store); its backward-data (thin_up_mfma<X2>, N = 2) and weight
    gradient FROM a split gradient"""
    from dusty_gan_amd import engine as E
    lay = X.layer("down", 2, 64, Hc, Wc, B, True, cls)
    assert max(float(lay.mass_fwd.max()), float(lay.mass_bwd.max()), float(lay.dw_mass().max())) < X.EXACT_UNITS   # (c)
    o = E.Ops(F32)
    o.force = DG_FORCE_THIN
    wf, wb = pack_down(lay.w)
    img = nhwc(lay.x).to(DEV, F32)
    wfd, wbd, bias = wf.contiguous().to(DEV, F32), wb.contiguous().to(DEV, F32), lay.b.to(DEV, F32)
    worst = 0.0
    for epi, scale, ref in ((L.EPI_LRELU, X.FWD_SCALE, lay.fwd_lrelu(True)), (L.EPI_LINEAR, X.LIN_SCALE, lay.fwd_linear(True))):
        dst = E.tag_x2(torch.full((B * Hc * Wc * 64,), float("nan"), device=DEV))
        n0 = len(trace)
        o.conv(L.MODE_S2, 0, True, B, Hc, Wc, 2, 64, img, (4 * Hc * Wc * 2, 2, 1), dst, (Hc * Wc * 64, 64, 1), wfd.data_ptr(), scale,
               epi, bias=bias.data_ptr(), bias_mod=64)
        torch.cuda.synchronize()
        rec = one(trace, n0, "conv")
        assert rec[1] == L.DG_CONV_FAMILY_THIN and rec[8] == 0, rec
        hi, lo = (from_nhwc(p, B, 64, Hc, Wc) for p in planes(dst))
        what = f"thin bf16x2 Down1 forward epi={epi} class {cls} {rec[1:9]}"
        if epi == L.EPI_LINEAR:
            X.assert_x2_exact(hi, lo, ref, what)
        else:
            X.assert_x2_close(hi, lo, ref, what)
            worst = X.x2_rel_error(hi, lo, ref)
    ed = put_x2(lay.e)
    out = torch.full((B * 4 * Hc * Wc * 2,), float("nan"), device=DEV)
    n0 = len(trace)
    o.conv(L.MODE_UP, 1, True, B, Hc, Wc, 64, 2, ed, (Hc * Wc * 64, 64, 1), out, (4 * Hc * Wc * 2, 2, 1), wbd.data_ptr(), X.BWD_SCALE,
           L.EPI_LINEAR)
    torch.cuda.synchronize()
    rec = one(trace, n0, "conv")
    assert rec[1] == L.DG_CONV_FAMILY_THIN and rec[8] == 2, rec      # thin_up_mfma<X2>
    X.assert_exact(from_nhwc(out.cpu(), B, 2, 2 * Hc, 2 * Wc), lay.q_bwd_full * X.BWD_SCALE,
                   f"thin bf16x2 Down1 backward-data class {cls} {rec[1:9]}")
    egd = put_x2(lay.eg)
    xgd = nhwc(lay.xg).to(DEV, F32)
    for k, acc in enumerate((1, 0)):
        rs = X.pow2_rowscale(B, k)
        dw = lay.base.to(DEV, F32) if acc else torch.full((16, 2, 64), float("nan"), device=DEV)
        n0 = len(trace)
        o.wgrad(0, True, B, Hc, Wc, 2, 64, xgd, (4 * Hc * Wc * 2, 2, 1), egd, (Hc * Wc * 64, 64, 1), dw.data_ptr(), 0.5,
                rowscale=rs.to(DEV, F32), accumulate=acc)
        torch.cuda.synchronize()
        rec = one(trace, n0, "wgrad")
        assert rec[1] == L.DG_WGRAD_VARIANT_THIN, rec
        X.assert_exact(dw.cpu(), (lay.base if acc else 0) + lay.dw(0.5, rs, full=True),
                       f"thin bf16x2 Down1 weight gradient accumulate={acc} class {cls} {rec}")
    print(f"[exact] thin bf16x2 Down1 {(Hc, Wc, B)} class {cls}: linear planes, backward-data and dW exact; forward lrelu worst "
          f"|hi + lo - ref| / |ref| {worst:.3g} (bound {X.X2_REL:.3g})")
