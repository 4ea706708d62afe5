"""Every conv, backward-data and weight-gradient kernel on integer data, checked PER ELEMENT against float64 (tests/exact_util.py).

Operands are small integers and every scale a power of two, so each kernel's fp32 accumulator is exact whatever its order of
additions: an EPI_LINEAR output and a weight gradient must equal the float64 result bit for bit, an EPI_LRELU / EPI_MASK output
must be one of the two neighbours of it in the output type, a bias gradient must be within the rounding of its own additions.
A failure names the elements: count, the first ten as (b, c, y, x, got, want) and histograms over y, x % 64, c % 16 and b - a
boundary row, a tile edge, a 16-channel fragment or a sample segment shows as one tall bar (weight gradients: b = tap, c = co,
y = ci).  tests/test_exact_util_cpu.py shows on the CPU which errors these criteria catch that the rel-L2 tests let through.

All launches go through the C ABI (engine.Ops); every test asserts from engine.TRACE which kernel family / variant ran.
Each test prints the largest error it saw in ulps of the output type and the worst bias-gradient error / bound.
"""
import pytest
import torch

from dusty_gan_amd._lib import (DG_FORCE_DIRECT, DG_FORCE_LOCKSTEP, DG_FORCE_MFMA, DG_FORCE_PINGPONG, DG_FORCE_PINGPONG_SINGLE,
                                DG_FORCE_PROJ_STREAM, DG_FORCE_THIN, DG_FORCE_WG_DMA_NOPAIRS, DG_FORCE_WG_DMA_PAIRS,
                                DG_FORCE_WG_REGSTAGED)
from tests import exact_util as X
from tests.test_gpu_ops import from_nhwc, nhwc, pack_bits, pack_down, pack_up

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
NAMES = {DG_FORCE_DIRECT: "direct", DG_FORCE_MFMA: "mfma", DG_FORCE_LOCKSTEP: "lockstep", DG_FORCE_PINGPONG: "pingpong",
         DG_FORCE_PINGPONG_SINGLE: "pingpong-single", DG_FORCE_THIN: "thin", DG_FORCE_PROJ_STREAM: "proj-stream",
         DG_FORCE_WG_REGSTAGED: "wg-regstaged", DG_FORCE_WG_DMA_PAIRS: "wg-dma-pairs", DG_FORCE_WG_DMA_NOPAIRS: "wg-dma-nopairs"}


@pytest.fixture(scope="module")
def L():
    from dusty_gan_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture
def trace():
    from dusty_gan_amd import engine as E
    E.TRACE = []
    yield E.TRACE
    E.TRACE = None


def tname(dtype, x3=False):
    return "fp32x3" if x3 else ("bf16" if dtype == BF else "fp32")


def note(family, what, ulps=None, ratio=None):
    """the figures the summary records: largest error in ulps of the output type, worst bias-gradient error / bound"""
    print(f"[exact] {family} {what}:" + ("" if ulps is None else f" max error {ulps:.3f} ulp") +
          ("" if ratio is None else f" dbias error/bound {ratio[1]:.3g} (sum of the {ratio[0]})"))


def family_of(L, force):
    return {DG_FORCE_DIRECT: L.DG_CONV_FAMILY_DIRECT, DG_FORCE_MFMA: L.DG_CONV_FAMILY_MFMA, DG_FORCE_THIN: L.DG_CONV_FAMILY_THIN,
            DG_FORCE_LOCKSTEP: L.DG_CONV_FAMILY_LOCKSTEP, DG_FORCE_PINGPONG: L.DG_CONV_FAMILY_PINGPONG,
            DG_FORCE_PINGPONG_SINGLE: L.DG_CONV_FAMILY_PINGPONG, DG_FORCE_PROJ_STREAM: L.DG_CONV_FAMILY_PROJ_STREAM}[force]


def pick_cap(tiles):
    """the largest workgroup count with >= 4 tiles for every workgroup and a remainder (uneven chunks); a launch of fewer than
    9 tiles has none: one workgroup then walks them all"""
    for c in range(tiles // 4, 1, -1):
        if tiles % c:
            return c
    return 1


def conv(L, trace, monkeypatch, *, mode, adj, ring, x, w_nk, N, scale, epi, dtype, force, x3=False, bias=None, aux=None,
         rowscale=None, want_db=False, multi=False, from_bits=None):
    """One conv launch as tests/test_gpu_ops.py::run_conv makes it.  x [B,K,Hin,Win], aux NCHW float64 (cpu); w_nk [16][N][K].
    Returns (out NCHW cpu in the output type, dbias or None, the launch's TRACE record).
    multi: the persistent kernels with Ops.default_wg_cap set so that every workgroup walks >= 4 tiles in uneven chunks
    (asserted from the trace).  from_bits: EPI_MASK from the saved 1-bit mask (True) or from aux itself (False); None = as the
    engine would (bits for bf16 maps of >= 16 channels).  An EPI_LRELU launch on such maps must leave mask_out = bits of (out > 0)."""
    from dusty_gan_amd.engine import MaskBits, Ops
    B, K, Hin, Win = x.shape
    if mode == L.MODE_S2:
        Hc, Wc, Ho, Wo = Hin // 2, Win // 2, Hin // 2, Win // 2
    else:
        Hc, Wc, Ho, Wo = Hin, Win, 2 * Hin, 2 * Win
    xd = nhwc(x).to(DEV, dtype)
    wd = w_nk.contiguous().to(DEV, dtype)
    auxd = None if aux is None else nhwc(aux).to(DEV, dtype)
    biasd = None if bias is None else bias.to(DEV, F32)
    rs = None if rowscale is None else rowscale.to(DEV, F32)
    can_bits = dtype == BF and N % 16 == 0 and MaskBits.enabled
    use_bits = can_bits if from_bits is None else (from_bits and can_bits)
    if from_bits:
        assert can_bits

    def launch(cap):
        monkeypatch.setattr(Ops, "default_wg_cap", cap)
        o = Ops(dtype, x3=x3)
        o.force = force
        out = torch.full((B * Ho * Wo * N,), float("nan"), device=DEV, dtype=dtype)
        db = torch.zeros(N, device=DEV) if want_db else None
        obits = None
        if can_bits and epi == L.EPI_LRELU:
            obits = MaskBits.register(out)
            obits.fill_(0xA5)
        if epi == L.EPI_MASK and use_bits:
            auxd._dg_bits = pack_bits(auxd)
        n0 = len(trace)
        try:
            o.conv(mode, adj, ring, B, Hc, Wc, K, N, xd, (Hin * Win * K, K, 1), out, (Ho * Wo * N, N, 1), wd.data_ptr(), scale, epi,
                   bias=None if biasd is None else biasd.data_ptr(), bias_mod=N, aux=auxd,
                   dbias=None if db is None else db.data_ptr(), rowscale=rs)
            torch.cuda.synchronize()
        finally:
            if auxd is not None and hasattr(auxd, "_dg_bits"):
                del auxd._dg_bits
        rec = [t for t in trace[n0:] if t[0] == "conv"]
        assert len(rec) == 1, trace[n0:]
        if obits is not None:
            assert torch.equal(obits, pack_bits(out)), "mask_out differs from the bits of (out > 0)"
        if epi == L.EPI_MASK and dtype == BF:
            # mask_in is taken by the kernels that read bits (the ping-pong conv among them); the others read aux either way
            assert not (rec[0][9] & 2) or use_bits, rec
            assert rec[0][1] != L.DG_CONV_FAMILY_PINGPONG or bool(rec[0][9] & 2) == bool(use_bits), rec
        return out, db, rec[0]
    out, db, rec = launch(0)
    assert rec[1] == family_of(L, force), (NAMES[force], rec)
    if multi:
        cap = pick_cap(rec[4])
        out, db, rec = launch(cap)
        assert rec[1] == family_of(L, force) and rec[5] <= cap, rec
        if cap > 1:
            assert rec[4] // rec[5] >= 4 and rec[4] % rec[5] != 0, rec      # >= 4 tiles per workgroup, uneven chunks
        else:
            assert rec[5] == 1 and rec[6] == rec[4], rec                     # too few tiles for both: one workgroup walks all
    return from_nhwc(out.cpu(), B, N, Ho, Wo), None if db is None else db.cpu(), rec


def check_layer(L, trace, monkeypatch, which, shape, ring, dtype, force, x3=False, multi=False, cls=None):
    """forward EPI_LRELU + bias (faithful, mask_out), forward EPI_LINEAR (exact), backward-data EPI_MASK with zeros in aux,
    power-of-two per-sample weights and the bias gradient - for bf16 both from the saved mask bits and from aux.
    cls: one of the fp32x3 mode's wide operand classes (X.Layer; fp32 storage only) - condition (c) replaces condition (a)"""
    lay = X.layer(which, *shape, ring, cls)
    down = which == "down"
    fmode, bmode = (L.MODE_S2, L.MODE_UP) if down else (L.MODE_UP, L.MODE_S2)
    wf, wb = (pack_down if down else pack_up)(lay.w)
    fam = f"{NAMES[force]} {tname(dtype, x3)}"
    tag = f"{which} {shape} ring={ring}" + (" several tiles per workgroup" if multi else "") + (f" class {cls}" if cls else "")
    kw = dict(ring=ring, dtype=dtype, force=force, x3=x3, multi=multi)
    if cls is None:
        for p in lay.units():                               # condition (a), on the reference
            assert float(p.abs().max()) <= X.Q_MAX
    else:                                                   # condition (c): every term family an exact fp32 sum
        assert dtype == F32 and max(float(lay.mass_fwd.max()), float(lay.mass_bwd.max())) < X.EXACT_UNITS
    worst = 0.0
    # forward, leaky-relu + bias
    ref = lay.fwd_lrelu()
    assert float((ref == 0).double().mean()) <= X.ZERO_FRACTION_MAX             # condition (b)
    out, _, rec = conv(L, trace, monkeypatch, mode=fmode, adj=0, x=lay.x, w_nk=wf, N=lay.Co, scale=X.FWD_SCALE, epi=L.EPI_LRELU,
                       bias=lay.b, **kw)
    fold = X.epilogue_f32_foldings(lay.q_fwd, X.FWD_SCALE, X.EPI_LRELU, lay.b) if dtype == F32 else None
    # the ping-pong conv folds sqrt 2 into scale and bias: ties at zero come out as +-2^-23 (X.folded_bias_slack states the bound)
    slack = X.folded_bias_slack(ref, lay.b) if rec[1] == L.DG_CONV_FAMILY_PINGPONG else None
    X.assert_faithful(out, ref, dtype, fold, f"{fam} forward lrelu {tag} {rec[1:7]}", slack)
    worst = max(worst, X.max_ulp_error(out, ref, dtype))
    # forward, linear
    ref = lay.fwd_linear()
    out, _, rec = conv(L, trace, monkeypatch, mode=fmode, adj=0, x=lay.x, w_nk=wf, N=lay.Co, scale=X.LIN_SCALE, epi=L.EPI_LINEAR,
                       bias=lay.b, **kw)
    X.assert_exact(out, ref, f"{fam} forward linear {tag} {rec[1:7]}")
    # backward-data into the previous layer's mask
    ref = lay.bwd_mask()
    fold = X.epilogue_f32_foldings(lay.q_bwd, X.BWD_SCALE, X.EPI_MASK, None, lay.prev) if dtype == F32 else None
    rs4 = lay.rs.view(-1, 1, 1, 1)
    ratios = []
    if force == DG_FORCE_LOCKSTEP and dtype == F32 and lay.Ci == 64:
        # the fp32 lock-step kernel has 128-channel N tiles only (csrc/conv_mfma.hip: "wherever its geometry allows, else
        # DG_EUNSUPPORTED"): the 64-channel backward-data pass is refused, not run on another kernel
        with pytest.raises(L.DgError, match="DG_EUNSUPPORTED"):
            conv(L, trace, monkeypatch, mode=bmode, adj=1, x=lay.e, w_nk=wb, N=lay.Ci, scale=X.BWD_SCALE, epi=L.EPI_MASK,
                 aux=lay.prev, rowscale=lay.rs, want_db=True, **kw)
        note(fam, tag + " (forward passes; backward-data refused)", worst)
        return
    for bits in ((True, False) if dtype == BF and lay.Ci % 16 == 0 else (None,)):
        out, db, rec = conv(L, trace, monkeypatch, mode=bmode, adj=1, x=lay.e, w_nk=wb, N=lay.Ci, scale=X.BWD_SCALE,
                            epi=L.EPI_MASK, aux=lay.prev, rowscale=lay.rs, want_db=True, from_bits=bits, **kw)
        what = f"{fam} backward-data {tag} bits={bits} {rec[1:7]}"
        X.assert_faithful(out, ref, dtype, fold, what)
        worst = max(worst, X.max_ulp_error(out, ref, dtype))
        ratios.append(X.assert_dbias(db, [("fp32 values", ref * rs4), ("stored values", out.double() * rs4)], what))
    note(fam, tag, worst, max(ratios, key=lambda r: r[1]))


# ---- the conv families on Down / Up layers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["down", "up"])
@pytest.mark.parametrize("ring", [True, False])
@pytest.mark.parametrize("shape", X.DIRECT_SHAPES, ids=str)
def test_direct_conv(L, trace, monkeypatch, which, shape, ring):
    """the only family with the reflect W axis and its adjoint taps; H = 2 puts both adjoint extra taps on adjacent rows"""
    check_layer(L, trace, monkeypatch, which, shape, ring, F32, DG_FORCE_DIRECT)


@pytest.mark.parametrize("which", ["down", "up"])
@pytest.mark.parametrize("dtype,x3", [(F32, False), (BF, False), (F32, True)], ids=["fp32", "bf16", "fp32x3"])
@pytest.mark.parametrize("shape", X.MFMA_SHAPES, ids=str)
def test_mfma_conv_one_tile_per_workgroup(L, trace, monkeypatch, which, shape, dtype, x3):
    check_layer(L, trace, monkeypatch, which, shape, True, dtype, DG_FORCE_MFMA, x3=x3)


PERSISTENT = [(DG_FORCE_LOCKSTEP, F32), (DG_FORCE_LOCKSTEP, BF), (DG_FORCE_PINGPONG, BF), (DG_FORCE_PINGPONG_SINGLE, BF)]


@pytest.mark.parametrize("which", ["down", "up"])
@pytest.mark.parametrize("multi", [False, True], ids=["default-launch", "several-tiles-per-workgroup"])
@pytest.mark.parametrize("force,dtype", PERSISTENT, ids=[f"{NAMES[f]}-{tname(d)}" for f, d in PERSISTENT])
@pytest.mark.parametrize("shape", X.PERSIST_SHAPES, ids=str)
def test_persistent_conv(L, trace, monkeypatch, which, shape, force, dtype, multi):
    """4 sample segments per tile, two column tiles per row, the 64-channel both-parities / single-parity tiles, four N tiles in
    the adjoint pass, an odd row count; once as launched by default and once with the tile walk stretched"""
    check_layer(L, trace, monkeypatch, which, shape, True, dtype, force, multi=multi)
    if shape[0] == 64 and which == "down" and force in (DG_FORCE_PINGPONG, DG_FORCE_PINGPONG_SINGLE) and not multi:
        # Down's backward-data into 64 channels: the both-parities tile (512 pixels x 64) / the single-parity 256 x 64 tile
        bwd = [t for t in trace if t[0] == "conv" and t[7].startswith("mode1adj1")]
        want = (512, 64) if force == DG_FORCE_PINGPONG else (256, 64)
        assert bwd and all((t[2], t[3]) == want for t in bwd), (want, bwd)


# ---- the thin family ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Hc,Wc,B", X.DOWN1_SHAPES)
def test_thin_down1(L, trace, monkeypatch, dtype, Hc, Wc, B):
    """Down1 (two input channels): forward with bias + leaky-relu and linear, the linear backward-data the engine runs (N = 2:
    no mask behind the image), the weight gradient with per-sample weights - VALU kernels for fp32, matrix-core ones for bf16"""
    lay = X.layer("down", 2, 64, Hc, Wc, B, True)
    wf, wb = pack_down(lay.w)
    fam = f"thin {tname(dtype)}"
    kw = dict(ring=True, dtype=dtype, force=DG_FORCE_THIN)
    ref = lay.fwd_lrelu()
    assert all(float(p.abs().max()) <= X.Q_MAX for p in lay.units())              # condition (a)
    assert float((ref == 0).double().mean()) <= X.ZERO_FRACTION_MAX               # condition (b)
    out, _, rec = conv(L, trace, monkeypatch, mode=L.MODE_S2, adj=0, x=lay.x, w_nk=wf, N=64, scale=X.FWD_SCALE, epi=L.EPI_LRELU,
                       bias=lay.b, **kw)
    fold = X.epilogue_f32_foldings(lay.q_fwd, X.FWD_SCALE, X.EPI_LRELU, lay.b) if dtype == F32 else None
    X.assert_faithful(out, ref, dtype, fold, f"{fam} Down1 forward lrelu {rec[1:9]}")
    worst = X.max_ulp_error(out, ref, dtype)
    out, _, rec = conv(L, trace, monkeypatch, mode=L.MODE_S2, adj=0, x=lay.x, w_nk=wf, N=64, scale=X.LIN_SCALE, epi=L.EPI_LINEAR,
                       bias=lay.b, **kw)
    X.assert_exact(out, lay.fwd_linear(), f"{fam} Down1 forward linear {rec[1:9]}")
    out, _, rec = conv(L, trace, monkeypatch, mode=L.MODE_UP, adj=1, x=lay.e, w_nk=wb, N=2, scale=X.BWD_SCALE, epi=L.EPI_LINEAR,
                       **kw)
    X.assert_exact(out, lay.q_bwd * X.BWD_SCALE, f"{fam} Down1 backward-data {rec[1:9]}")
    assert (rec[8] == 2) == (dtype == BF), rec               # thin_up_mfma for bf16, the VALU kernel for fp32
    check_wgrad(L, trace, lay, DG_FORCE_THIN, dtype, False, fam,
                L.DG_WGRAD_VARIANT_THIN_MFMA if dtype == BF else L.DG_WGRAD_VARIANT_THIN)
    note(fam, f"Down1 {(Hc, Wc, B)}", worst)


def head_launches(L, trace, monkeypatch, h, dtype, pixel_major):
    """Head forward (planar fp32 output, per-head scales in DgConv.nscale) and masked backward-data with the bias gradient, from
    the planar fp32 head gradient or from its pixel-major bf16 copy (thin_s2_mfma)"""
    from dusty_gan_amd.engine import Ops
    nh, Hc, Wc, B, C0 = h.nh, h.Hc, h.Wc, h.B, h.C0
    HW = 4 * Hc * Wc
    assert max(float(h.q_fwd.abs().max()), float(h.q_bwd.abs().max())) <= X.Q_MAX  # condition (a)
    assert float((h.fwd() == 0).double().mean()) <= X.ZERO_FRACTION_MAX             # condition (b)
    o = Ops(dtype)
    o.force = DG_FORCE_THIN
    fam = f"thin {tname(dtype)}"
    xd = nhwc(h.x).to(DEV, dtype)
    coci = h.w.permute(2, 3, 1, 0).contiguous().to(DEV, dtype)       # forward shadow [tap][n = co][k = ci]
    cico = h.w.permute(2, 3, 0, 1).contiguous().to(DEV, dtype)       # backward shadow [tap][n = ci][k = co]
    bias, nscale = h.b.to(DEV, F32), h.nscale.to(DEV, F32)
    out = torch.full((B, nh, 2 * Hc, 2 * Wc), float("nan"), device=DEV)
    n0 = len(trace)
    o.conv(L.MODE_UP, 0, True, B, Hc, Wc, C0, nh, xd, (Hc * Wc * C0, C0, 1), out, (nh * HW, 1, HW), coci.data_ptr(), 1.0,
           L.EPI_LINEAR, bias=bias.data_ptr(), bias_mod=nh, out_dt=L.DG_F32, nscale=nscale)
    torch.cuda.synchronize()
    rec = [t for t in trace[n0:] if t[0] == "conv"][0]
    assert rec[1] == L.DG_CONV_FAMILY_THIN and (rec[8] == 2) == (dtype == BF), rec
    X.assert_exact(out.cpu(), h.fwd(), f"{fam} head forward nh={nh} {rec[1:9]}")
    # backward-data
    prevd = nhwc(h.prev).to(DEV, dtype)
    if pixel_major:
        cp = 2 if nh <= 2 else 4
        g = torch.zeros(B, 2 * Hc, 2 * Wc, cp, dtype=torch.float64)
        g[..., :nh] = h.e.permute(0, 2, 3, 1)
        gd, gs, in_dt = g.to(DEV, BF).contiguous(), (HW * cp, cp, 1), None
    else:
        gd, gs, in_dt = h.e.to(DEV, F32).contiguous(), (nh * HW, 1, HW), L.DG_F32
    ref = h.bwd_mask()
    rs = X.pow2_rowscale(B)
    results = []
    for bits in ((True, False) if dtype == BF else (False,)):
        dp = torch.full((B * Hc * Wc * C0,), float("nan"), device=DEV, dtype=dtype)
        db = torch.zeros(C0, device=DEV)
        if bits:
            prevd._dg_bits = pack_bits(prevd)
        n0 = len(trace)
        try:
            o.conv(L.MODE_S2, 1, True, B, Hc, Wc, nh, C0, gd, gs, dp, (Hc * Wc * C0, C0, 1), cico.data_ptr(), X.BWD_SCALE,
                   L.EPI_MASK, aux=prevd, dbias=db.data_ptr(), bias_mod=C0, in_dt=in_dt, rowscale=rs.to(DEV, F32))
            torch.cuda.synchronize()
        finally:
            if bits:
                del prevd._dg_bits
        rec = [t for t in trace[n0:] if t[0] == "conv"][0]
        # thin_s2_mfma takes the pixel-major bf16 gradient from four coarse rows on (csrc/conv_thin.hip: conv_s2_mfma_ok)
        assert rec[1] == L.DG_CONV_FAMILY_THIN and (rec[8] == 1) == (pixel_major and Hc >= 4), rec
        got = from_nhwc(dp.cpu(), B, C0, Hc, Wc)
        what = f"{fam} head backward-data nh={nh} pixel_major={pixel_major} bits={bits} {rec[1:9]}"
        fold = X.epilogue_f32_foldings(h.q_bwd, X.BWD_SCALE, X.EPI_MASK, None, h.prev) if dtype == F32 else None
        X.assert_faithful(got, ref, dtype, fold, what)
        rs4 = rs.view(-1, 1, 1, 1)
        results.append((X.max_ulp_error(got, ref, dtype),
                        X.assert_dbias(db.cpu(), [("fp32 values", ref * rs4), ("stored values", got.double() * rs4)], what)))
    scratch = Ops._dbias_ws.get(str(gd.device))
    assert scratch is None or float(scratch.abs().max()) == 0.0     # the staging scratch is left zero
    note(fam, f"head nh={nh} {(Hc, Wc)} pixel_major={pixel_major}", max(r[0] for r in results),
         max((r[1] for r in results), key=lambda r: r[1]))


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("nh", [1, 2, 3])
@pytest.mark.parametrize("Hc,Wc", X.HEAD_SHAPES)
def test_thin_head(L, trace, monkeypatch, dtype, nh, Hc, Wc):
    h = X.head(nh, Hc, Wc)
    head_launches(L, trace, monkeypatch, h, dtype, False)
    # weight gradient from the planar fp32 head gradient, per-sample weights
    from dusty_gan_amd.engine import Ops
    o = Ops(dtype)
    o.force = DG_FORCE_THIN
    HW = 4 * Hc * Wc
    xd, gd = nhwc(h.x).to(DEV, dtype), h.e.to(DEV, F32).contiguous()
    rs = X.pow2_rowscale(h.B, 1)
    dw = torch.full((16, h.C0, nh), float("nan"), device=DEV)
    n0 = len(trace)
    o.wgrad(1, True, h.B, Hc, Wc, h.C0, nh, xd, (Hc * Wc * h.C0, h.C0, 1), gd, (nh * HW, 1, HW), dw.data_ptr(), 0.5,
            rowscale=rs.to(DEV, F32), g_dt=L.DG_F32, accumulate=0)
    torch.cuda.synchronize()
    rec = [t for t in trace[n0:] if t[0] == "wgrad"][0]
    assert rec[1] in (L.DG_WGRAD_VARIANT_THIN, L.DG_WGRAD_VARIANT_THIN_MFMA), rec
    X.assert_exact(dw.cpu(), h.dw(rs) * 0.5, f"thin {tname(dtype)} head weight gradient nh={nh} {rec}")


@pytest.mark.parametrize("nh", [1, 2, 3])
@pytest.mark.parametrize("Hc,Wc", X.HEAD_SHAPES)
def test_thin_head_pixel_major_mfma(L, trace, monkeypatch, nh, Hc, Wc):
    """the kernels of test_head_bwd_data_pixel_major_mfma / test_head_wgrad_pixel_major_mfma: backward-data and weight gradient
    from the pixel-major bf16 copy of the head gradient"""
    from dusty_gan_amd.engine import Ops
    h = X.head(nh, Hc, Wc)
    head_launches(L, trace, monkeypatch, h, BF, True)
    o = Ops(BF)
    o.force = DG_FORCE_THIN
    HW, cp = 4 * Hc * Wc, (2 if nh <= 2 else 4)
    g = torch.full((h.B, 2 * Hc, 2 * Wc, cp), 7.0, dtype=torch.float64)   # the padding channels must not leak
    g[..., :nh] = h.e.permute(0, 2, 3, 1)
    gd, xd = g.to(DEV, BF).contiguous(), nhwc(h.x).to(DEV, BF)
    rs = X.pow2_rowscale(h.B, 2)
    for use_ws in (True, False):
        o.use_ws = use_ws
        base = torch.randint(-4, 5, (16, h.C0, nh), generator=X.gen(nh)).double()
        dw = base.to(DEV, F32)
        n0 = len(trace)
        o.wgrad(1, True, h.B, Hc, Wc, h.C0, nh, xd, (Hc * Wc * h.C0, h.C0, 1), gd, (HW * cp, cp, 1), dw.data_ptr(), 0.5,
                rowscale=rs.to(DEV, F32))
        torch.cuda.synchronize()
        rec = [t for t in trace[n0:] if t[0] == "wgrad"][0]
        # thin_wgrad_up_mfma works on pairs of coarse rows: an odd row count goes to the VALU kernel
        assert rec[1] == (L.DG_WGRAD_VARIANT_THIN_MFMA if Hc % 2 == 0 else L.DG_WGRAD_VARIANT_THIN), rec
        X.assert_exact(dw.cpu(), base + h.dw(rs) * 0.5, f"thin bf16 head weight gradient (pixel-major) nh={nh} ws={use_ws} {rec}")


# ---- Proj (MODE_GEMM) --------------------------------------------------------------------------------------------------------------
PROJ_KERNELS = [(DG_FORCE_DIRECT, F32, False), (DG_FORCE_MFMA, F32, False), (DG_FORCE_MFMA, BF, False), (DG_FORCE_MFMA, F32, True),
                (DG_FORCE_PROJ_STREAM, BF, False)]


@pytest.mark.parametrize("force,dtype,x3", PROJ_KERNELS, ids=[f"{NAMES[f]}-{tname(d, x)}" for f, d, x in PROJ_KERNELS])
@pytest.mark.parametrize("B,N", X.PROJ_SHAPES)
def test_proj_gemm(L, trace, force, dtype, x3, B, N):
    """Proj forward on the direct, MFMA, fp32x3 and weight-streaming kernels (ragged batch 17), both epilogues; its weight
    gradient (wmode 2) on the kernels that have one"""
    check_proj(L, trace, X.proj(B, N), force, dtype, x3)


def check_proj(L, trace, p, force, dtype, x3):
    """p: X.Proj, small operands or one of the fp32x3 mode's wide classes (fp32 storage)"""
    from dusty_gan_amd.engine import Ops
    B, N = p.B, p.N
    fam = f"proj {NAMES[force]} {tname(dtype, x3)}" + (f" class {p.cls}" if p.cls else "")
    if p.cls is not None:
        assert dtype == F32 and max(float(p.mass.max()), float(p.dw_mass.max())) < X.EXACT_UNITS      # condition (c)
    o = Ops(dtype, x3=x3)
    o.force = force
    zd, wd, bd = p.z.to(DEV, dtype).contiguous(), p.w.to(DEV, dtype).contiguous(), p.b.to(DEV, F32)
    worst = 0.0
    for epi, code, scale in ((X.EPI_LRELU, L.EPI_LRELU, X.FWD_SCALE), (X.EPI_LINEAR, L.EPI_LINEAR, X.LIN_SCALE)):
        assert p.cls is not None or float(p.units(epi).abs().max()) <= X.Q_MAX
        out = torch.full((B, N), float("nan"), device=DEV, dtype=dtype)
        n0 = len(trace)
        o.conv(L.MODE_GEMM, 0, 1, B, 1, 1, p.K, N, zd, (p.K, 0, 1), out, (N, 0, 1), wd.data_ptr(), scale, code,
               bias=bd.data_ptr(), bias_mod=p.C)
        torch.cuda.synchronize()
        rec = [t for t in trace[n0:] if t[0] == "conv"][0]
        assert rec[1] == family_of(L, force), rec
        ref = p.fwd(epi)
        if epi == X.EPI_LINEAR:
            X.assert_exact(out.cpu(), ref, f"{fam} linear {(B, N)}")
        else:
            fold = X.epilogue_f32_foldings(p.q, scale, epi, p._bias()) if dtype == F32 else None
            slack = X.folded_bias_slack(ref, p._bias()) if force == DG_FORCE_PROJ_STREAM else None   # (sqrt 2 folded into the bias)
            X.assert_faithful(out.cpu(), ref, dtype, fold, f"{fam} lrelu {(B, N)}", slack)
            worst = X.max_ulp_error(out.cpu(), ref, dtype)
    if force != DG_FORCE_PROJ_STREAM:
        ed, zd = p.eg.to(DEV, dtype).contiguous(), p.zg.to(DEV, dtype).contiguous()
        for acc in (0, 1):
            base = torch.randint(-4, 5, (N, p.K), generator=X.gen(B)).double()
            dw = base.to(DEV, F32) if acc else torch.full((N, p.K), float("nan"), device=DEV)
            n0 = len(trace)
            o.wgrad(2, 1, 1, 1, B, N, p.K, ed, (0, N, 1), zd, (0, p.K, 1), dw.data_ptr(), 0.5, accumulate=acc)
            torch.cuda.synchronize()
            rec = [t for t in trace[n0:] if t[0] == "wgrad"][0]
            assert rec[1] == (L.DG_WGRAD_VARIANT_DIRECT if force == DG_FORCE_DIRECT else L.DG_WGRAD_VARIANT_MFMA), rec
            X.assert_exact(dw.cpu(), (base if acc else 0) + p.dw(0.5), f"{fam} weight gradient accumulate={acc} {(B, N)}")
    note(fam, f"{(B, N)}", worst)


# ---- weight gradients ----------------------------------------------------------------------------------------------------------------
def wgrad_args(lay, a, e):
    """(wmode, strides of the input and of the gradient) as tests/test_gpu_ops.py launches Down / Up weight gradients"""
    H, W, Ci, Co = lay.H, lay.W, lay.Ci, lay.Co
    if lay.which == "down":
        return 0, (4 * H * W * Ci, Ci, 1), (H * W * Co, Co, 1)
    return 1, (H * W * Ci, Ci, 1), (4 * H * W * Co, Co, 1)


def check_wgrad(L, trace, lay, force, dtype, x3, fam, variants, pairs=None, put=None):
    """dW of one layer, torch.equal against float64: workspace and atomics path, accumulate onto an integer-valued dW and
    overwrite of a NaN-filled one, per-sample weights cycling 0.5 / 1 / 2, the gradient-sample map where the kernel has it.
    put: how an operand (NCHW float64) gets onto the device (default: pixel-major in `dtype`; the split-storage tests pack it)"""
    from dusty_gan_amd.engine import Ops
    variants = variants if isinstance(variants, tuple) else (variants,)
    put = put or (lambda t: nhwc(t).to(DEV, dtype))
    xd, ed = put(lay.xg), put(lay.eg)
    if lay.cls is not None:                                 # condition (c) for the weight gradient's own contraction
        assert float(lay.dw_mass().max()) < X.EXACT_UNITS
    wmode, sa, sg = wgrad_args(lay, xd, ed)
    B, H, W, Ci, Co = lay.B, lay.H, lay.W, lay.Ci, lay.Co
    seen = set()
    for k, (use_ws, acc) in enumerate([(True, 1), (True, 0), (False, 1), (False, 0)]):
        o = Ops(dtype, x3=x3)
        o.force, o.use_ws = force, use_ws
        rs = X.pow2_rowscale(B, k)
        scale = (0.5, 0.25)[k % 2]
        dw = lay.base.to(DEV, F32) if acc else torch.full((16, Ci, Co), float("nan"), device=DEV)
        n0 = len(trace)
        o.wgrad(wmode, lay.ring, B, H, W, Ci, Co, xd, sa, ed, sg, dw.data_ptr(), scale, rowscale=rs.to(DEV, F32), accumulate=acc)
        torch.cuda.synchronize()
        rec = [t for t in trace[n0:] if t[0] == "wgrad"][0]
        assert rec[1] in variants, (fam, rec)
        if not use_ws:
            assert not rec[5], rec                          # atomics onto dW: no workspace
        if pairs is not None and rec[1] == L.DG_WGRAD_VARIANT_DMA and use_ws:
            assert rec[4] == pairs, rec
        seen.add((rec[1], bool(rec[5])))
        want = (lay.base if acc else 0) + lay.dw(scale, rs)
        X.assert_exact(dw.cpu(), want, f"{fam} weight gradient {lay.which} ws={use_ws} accumulate={acc} {rec}")
    o = Ops(dtype, x3=x3)
    o.force = force
    mapped = False
    dw = torch.zeros(16, Ci, Co, device=DEV)
    if B >= 2 and o.wgrad_takes_map(wmode, lay.ring, B, H, W, Ci, Co, xd, sa, ed, sg, dw.data_ptr()):
        g_mod = max(1, 2 * B // 3)
        rs = X.pow2_rowscale(B, 1)
        o.wgrad(wmode, lay.ring, B, H, W, Ci, Co, xd, sa, ed, sg, dw.data_ptr(), 0.5, rowscale=rs.to(DEV, F32), g_mod=g_mod)
        torch.cuda.synchronize()
        X.assert_exact(dw.cpu(), lay.dw(0.5, rs, g_mod), f"{fam} weight gradient {lay.which} g_mod={g_mod}")
        mapped = True
    print(f"[exact] {fam} weight gradient {lay.which} {(Ci, Co, H, W, B)}{f' class {lay.cls}' if lay.cls else ''}: exact; kernels (variant, workspace) {sorted(seen)}"
          f"{' + sample map' if mapped else ''}")
    return seen


WGRAD = [(DG_FORCE_DIRECT, F32, False, X.DIRECT_SHAPES), (DG_FORCE_MFMA, F32, False, X.MFMA_SHAPES),
         (DG_FORCE_MFMA, BF, False, X.MFMA_SHAPES), (DG_FORCE_MFMA, F32, True, X.MFMA_SHAPES),
         (DG_FORCE_WG_REGSTAGED, BF, False, X.MFMA_SHAPES), (DG_FORCE_WG_REGSTAGED, F32, False, X.MFMA_SHAPES),
         (DG_FORCE_WG_DMA_PAIRS, BF, False, X.MFMA_SHAPES + X.PERSIST_SHAPES),
         (DG_FORCE_WG_DMA_NOPAIRS, BF, False, X.MFMA_SHAPES + X.PERSIST_SHAPES)]
WGRAD_CASES = [(f, d, x, s) for f, d, x, shapes in WGRAD for s in shapes]


@pytest.mark.parametrize("which", ["down", "up"])
@pytest.mark.parametrize("force,dtype,x3,shape", WGRAD_CASES, ids=[f"{NAMES[f]}-{tname(d, x)}-{s}" for f, d, x, s in WGRAD_CASES])
def test_weight_gradient(L, trace, which, force, dtype, x3, shape):
    lay = X.layer(which, *shape, True)
    fam = f"{NAMES[force]} {tname(dtype, x3)}"
    if force == DG_FORCE_DIRECT:
        variants = L.DG_WGRAD_VARIANT_DIRECT
    elif force in (DG_FORCE_WG_DMA_PAIRS, DG_FORCE_WG_DMA_NOPAIRS):
        variants = L.DG_WGRAD_VARIANT_DMA
    elif force == DG_FORCE_WG_REGSTAGED or dtype == F32:
        variants = L.DG_WGRAD_VARIANT_MFMA
    else:
        variants = (L.DG_WGRAD_VARIANT_MFMA, L.DG_WGRAD_VARIANT_DMA)     # DG_FORCE_MFMA on bf16: the library's own choice of the two
    pairs = {DG_FORCE_WG_DMA_PAIRS: 1, DG_FORCE_WG_DMA_NOPAIRS: 0}.get(force)
    check_wgrad(L, trace, lay, force, dtype, x3, fam, variants, pairs)
    if force == DG_FORCE_DIRECT:                            # the reflect W axis exists only here
        check_wgrad(L, trace, X.layer(which, *shape, False), force, dtype, x3, fam + " reflect", variants)


@pytest.mark.parametrize("wmode", [0, 1])
@pytest.mark.parametrize("force", [DG_FORCE_MFMA, DG_FORCE_WG_DMA_PAIRS, DG_FORCE_WG_DMA_NOPAIRS], ids=["auto", "tap-pairs", "single-taps"])
def test_weight_gradient_group_of_three_layers(L, trace, wmode, force):
    """one `with ops.grouped():` block of three layers: each layer's dW is the float64 result, as the three single launches'"""
    which = "down" if wmode == 0 else "up"
    lays = [X.Layer(which, *s, True) for s in ((64, 128, 4, 128, 2), (128, 64, 2, 64, 1), (64, 64, 3, 64, 3))]
    check_wgrad_group(L, trace, lays, force, BF, lambda t: nhwc(t).to(DEV, BF))


def check_wgrad_group(L, trace, lays, force, dtype, put):
    """put: as in check_wgrad"""
    from dusty_gan_amd import engine as E
    data = [(put(l.xg), put(l.eg)) for l in lays]

    def run(grouped):
        o = E.Ops(dtype)
        o.force = force
        outs = [l.base.to(DEV, F32) for l in lays]
        prev, E.Ops.group_enabled = E.Ops.group_enabled, grouped
        n0 = len(trace)
        try:
            with o.grouped():
                for l, (xd, ed), dw in zip(lays, data, outs):
                    wm, sa, sg = wgrad_args(l, xd, ed)
                    o.wgrad(wm, True, l.B, l.H, l.W, l.Ci, l.Co, xd, sa, ed, sg, dw.data_ptr(), 0.5, rowscale=l.rs.to(DEV, F32),
                            defer=True)
        finally:
            E.Ops.group_enabled = prev
        E.WGRAD_WS.flush()
        torch.cuda.synchronize()
        return outs, trace[n0:]
    single, tr0 = run(False)
    group, tr1 = run(True)
    assert not [t for t in tr0 if t[0] == "wgrad_group"]
    groups = [t for t in tr1 if t[0] == "wgrad_group"]
    assert len(groups) == 1 and groups[0][1] == 3, tr1
    assert [t[1] for t in tr1 if t[0] == "wgrad"] == [L.DG_WGRAD_VARIANT_DMA] * 3, tr1
    for k, l in enumerate(lays):
        want = l.base + l.dw(0.5, l.rs)
        X.assert_exact(single[k].cpu(), want, f"single launch, layer {k}")
        X.assert_exact(group[k].cpu(), want, f"group launch, layer {k}")
