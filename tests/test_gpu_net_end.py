"""The step's network end held per element: dg_head_post_fwd / _fwd_sum / _bwd / _bwd2 (csrc/head_post.hip, head_post.h, dg_tanh),
the final conv's 16-byte kernels, dg_gan_d_step / dg_gan_g_step, dg_final_gan_bwd, dg_pl_penalty, dg_mean_acc and dg_scale
(csrc/pointwise.hip) against the float64 restatements and the criteria of tests/net_end_ref.py (derived there, proved on the CPU by
tests/test_net_end_ref_cpu.py).  Three kinds of criterion: exact (fp32 bit for bit, bf16 the RNE of the reference) wherever the
data makes the arithmetic exact or round once in a known place; bounded (|got - ref64| <= a derived bound, per element);
structural (the pixel-major copy is the RNE of the planar output, padded channels zero, up / rs are dy's slices, scratches are
left zero, guards intact, every owned element written, a refused launch writes nothing).  Every launch goes through the C ABI;
every output starts as sentinels between guards.  The last test prints the largest |got - ref| / bound per bounded output (-s).

Measured on an MI355X, largest |got - ref| / bound over every case of this file (EXP_ULPS, RCP_ULPS and LOG1P_ULPS of
tests/net_end_ref.py are borrowed figures, not measured; no run contradicted them):
    dg_tanh         t (sweep) 0.948
    head_post_fwd   t 0.979   dsum 0.087
    head_post_bwd   d0 0.730  d1 0.738  d2 0.741  dbias0 0.021  dbias1 0.069  dbias2 0.045
    head_post_bwd2  row0 0.731  row1 0.738  row2 0.727  dbias0 0.026  dbias1 0.059  dbias2 0.039
    final_bwd_data  dbias 0.102
    gan_d_step      dy 0.661  loss 0.202  mean_real 0.090  mean_fake 0.081  dfinal_b 0.131
    gan_g_step      dy 0.620  loss 0.142
    final_gan_bwd   dy 0.242  scalars 0.034  dfinal_b 0.008  dwf 0.051  dbias 0.032  dbias (part) 0.020
    pl_penalty      baseline 0.490  acc baseline 0.817  acc penalty 0.148  v 0.204
t and d0 come close to 1 by construction: just above a power of two half an ulp of the result is the whole D24 |result| the last
rounding is allowed, and the polynomial branch of dg_tanh rounds little else."""
import functools

import numpy as np
import pytest
import torch

from tests import image_exact_util as U
from tests import net_end_ref as N
from tests.gpu_guard_util import BF16, DEV, F32, MODES, Acc, Owned

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def L():
    from dusty_gan_amd import _lib
    _lib.lib()
    return _lib


def dnp(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F)).to(dtype).to(DEV)


def bits16(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def t4(x):
    """[B,C,1,X] for image_exact_util's reports; vectors stay 1-D"""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    if t.ndim <= 1:
        return t.reshape(-1)
    return t.reshape(t.shape[0], -1, 1, t.shape[-1]) if t.ndim > 2 else t.reshape(t.shape[0], 1, 1, t.shape[1])


def ex(got, ref64, what):
    """the exact criterion: U.assert_exact (fp32) / U.assert_rne (bf16)"""
    got, ref = t4(got), t4(np.asarray(ref64, dtype=np.float64))
    return U.assert_rne(got, ref, what) if got.dtype == BF16 else U.assert_exact(got, ref, what)


def bounded(kernel, output, got, want, bound, what):
    q = N.check(f"{what} {output}", np.atleast_1d(got), np.atleast_1d(want), np.atleast_1d(bound))
    N.note_ratio(kernel, output, q)
    return q


# ---- dg_head_post_fwd / dg_head_post_fwd_sum ------------------------------------------------------------------------------------------
def run_head_fwd(L, inp, training, with_sum, mode="plain", offset=False):
    lib, B, HW, arch = L.lib(), inp.B, inp.HW, inp.arch
    heads = np.stack([inp.raw, inp.h1, inp.h2][:1 + arch], axis=1)
    gout = Owned((B, 1 + arch, HW))
    gout.t.copy_(dnp(heads))
    if offset:                                                 # noise_pixel 4 bytes off a 16-byte boundary
        hold = torch.zeros(B * HW + 1, device=DEV)
        hold[1:].copy_(dnp(inp.npx).reshape(-1))
        npx = hold[1:]
        assert npx.data_ptr() % 16 == 4
    else:
        npx = dnp(inp.npx)
    nim = dnp(inp.nim)
    mask = Owned((B, arch, HW)) if arch else None
    depth = Owned((B, HW))
    acc = Acc(L, mode)
    dsum = acc.take(B) if with_sum else None
    args = (gout.ptr, npx.data_ptr(), nim.data_ptr(), arch, training, inp.tau, inp.c, B, HW, mask.ptr if arch else None, depth.ptr)
    rc = lib.dg_head_post_fwd_sum(*args, dsum.data_ptr(), None) if with_sum else lib.dg_head_post_fwd(*args, None)
    torch.cuda.synchronize()
    return rc, gout, mask, depth, acc, dsum, heads


def check_head_fwd(L, inp, training, with_sum, mode="plain", offset=False, exact_sum=False):
    B, HW, arch = inp.B, inp.HW, inp.arch
    what = f"dg_head_post_fwd{'_sum' if with_sum else ''} {inp.tier} arch={arch} HW={HW} training={training} {mode}{' offset' if offset else ''}"
    rc, gout, mask, depth, acc, dsum, heads = run_head_fwd(L, inp, training, with_sum, mode, offset)
    if with_sum and HW % 256:
        assert rc == L.DG_EUNSUPPORTED, what
        assert torch.equal(gout.done(what), torch.from_numpy(heads)), what + ": a refused launch touched gout"
        depth.done(what, written=False)
        if arch:
            mask.done(what, written=False)
        acc.done(what)
        assert not bool(dsum.cpu().any()), what
        return None
    L.check(rc, what)
    g = gout.done(what).numpy()
    ref = N.head_fwd_case(inp, training)
    assert np.array_equal(g[:, 1:].view(np.uint32), heads[:, 1:].view(np.uint32)), what + ": the logits were touched"
    t = g[:, 0]
    if inp.tier == "sat":
        N.same_values(what + " t", t, np.round(ref.t))
    else:
        bounded("head_post_fwd", "t", t, ref.t, ref.bt, what)
    n = t.size
    if arch:
        mk = mask.done(what)
        n += ex(mk[:, 0], ref.mp, what + " pixel mask")
        if arch == 2:
            n += ex(mk[:, 1], ref.mi, what + " image mask")
    d = depth.done(what).numpy()
    N.same_values(what + " depth", d, N.depth_of(t, ref.m, inp.c))
    if with_sum:
        acc.done(what)
        got = dsum.cpu().numpy()
        want = N.f64(d).sum(axis=1)
        if exact_sum:
            n += ex(dsum.cpu(), want, what + " dsum")
        else:
            quad = HW % 1024 == 0 and not offset
            adds = N.head_sum_adds(HW, quad)
            bounded("head_post_fwd_sum", "dsum", got, want, N.sum_bound(adds, np.abs(N.f64(d)).sum(axis=1)) + adds * 2.0 ** -33, what)
    return g, (mask.t.cpu() if arch else None), d, (dsum.cpu() if with_sum else None), n


@pytest.mark.parametrize("tier", N.TIERS)
@pytest.mark.parametrize("arch", [0, 1, 2])
@pytest.mark.parametrize("HW", N.HEAD_FWD_HW)
def test_head_post_fwd(L, HW, arch, tier):
    inp = N.head_inputs(tier, arch, 3, HW)
    assert N.excluded_pixels(inp) == 0
    n = 0
    for training in (1, 0):
        a = check_head_fwd(L, inp, training, False)
        b = check_head_fwd(L, inp, training, True)
        n += a[4] + (b[4] if b else 0)
        if b:                                                  # every form returns the same bits
            assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
        if HW == 1024:
            c = check_head_fwd(L, inp, training, True, offset=True)
            assert np.array_equal(c[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(c[2].view(np.uint32), b[2].view(np.uint32))
            assert arch == 0 or torch.equal(c[1], b[1])
    U.line("head_post_fwd", f"{tier} arch={arch} HW={HW}", n)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("arch", [0, 1, 2])
@pytest.mark.parametrize("HW", [3072, 8192])
def test_head_post_fwd_sum_of_dyadic_depths_is_exact(L, HW, arch, mode):
    """tanh of 0, +-16, +-90 is exactly 0, +-1: every depth is -1, 0, 1 or drop_const and the per-sample sum, with 3 and 2
    contributors, is exact through float atomics and through the arena's 32.32 fixed point"""
    inp = N.head_inputs("sat", arch, 3, HW)
    r = check_head_fwd(L, inp, 1, True, mode, exact_sum=True)
    U.line("head_post_fwd_sum", f"sat arch={arch} HW={HW} {mode}", r[4])


def test_dg_tanh_sweep(L):
    """8192 points geometric in [2^-24, 16] with both neighbourhoods of the seam, and their negatives, through both forms"""
    x = N.tanh_sweep()
    inp = N.head_inputs("random", 0, 1, x.size)
    inp["raw"] = x[None].copy()
    want, bound = np.tanh(N.f64(x)), N.tanh_bound(x)
    for with_sum in (False, True):
        rc, gout, _, depth, acc, dsum, _ = run_head_fwd(L, inp, 1, with_sum)
        L.check(rc)
        t = gout.done("sweep").numpy().reshape(-1)
        bounded("dg_tanh", "t (sweep)", t, want, bound, f"sweep sum={with_sum}")
        assert np.array_equal(depth.done("sweep").numpy().reshape(-1).view(np.uint32), t.view(np.uint32))
        seam = np.abs(N.f64(x[:8192]) - 0.25) <= 2.0 ** -22
        assert seam.sum() == 9
        assert np.all(np.diff(t[:8192][seam]) >= 0) and np.all(np.diff(t[8192:][seam]) <= 0), \
            f"dg_tanh is not monotone across its seam: {t[:8192][seam]!r}"


# ---- dg_head_post_bwd ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def bwd_case(case):
    inp = N.head_case_inputs(case)
    return inp, N.head_bwd_case(inp)


def run_head_bwd(L, inp, cp, planar, with_ws, nb=None):
    lib, HW, arch = L.lib(), inp.HW, inp.arch
    B = inp.B if nb is None else nb
    gout = dnp(np.stack([inp.t, inp.h1, inp.h2][:1 + arch], axis=1)[:B])
    mask = dnp(np.stack([inp.mp, inp.mi][:max(arch, 1)], axis=1)[:B])
    npx, nim, go = dnp(inp.npx[:B]), dnp(inp.nim[:B]), dnp(inp.go[:B])
    draw = Owned((B, 1 + arch, HW)) if planar else None
    pm = Owned((B, HW, cp), BF16) if cp else None
    db = Owned((3,), fill=0.0)
    ws = torch.zeros(B * 1024, device=DEV) if with_ws else None
    keep = (gout, mask, npx, nim, go)

    def launch():
        rc = lib.dg_head_post_bwd(gout.data_ptr(), npx.data_ptr(), nim.data_ptr(), mask.data_ptr(), go.data_ptr(), arch, inp.tau, inp.c,
                                  B, HW, N.S_DEPTH, N.S_CONF, draw.ptr if planar else None, db.ptr, pm.ptr if cp else None, cp,
                                  L.ptr(ws), None)
        torch.cuda.synchronize()
        return rc
    return launch, draw, pm, db, ws, keep


@pytest.mark.parametrize("case", N.HEAD_BWD, ids=N.case_id)
def test_head_post_bwd(L, case):
    tier, arch, B, HW = case
    inp, r = bwd_case(case)
    assert N.excluded_pixels(inp) == 0
    scales = (N.S_DEPTH, N.S_CONF, N.S_CONF)
    quad = HW % 4 == 0
    with_ws = HW >= 4096
    adds, hb = N.head_bwd_adds(B, HW, quad)
    cps = (2, 4, 3) if HW == 21 else (2, 4) if B == 3 else (4,)
    n = 0
    for cp in cps:
        pm_given = None
        for planar in (True, False):
            what = f"dg_head_post_bwd {N.case_id(case)} cp={cp} planar={'given' if planar else 'null'}"
            launch, draw, pm, db, ws, keep = run_head_bwd(L, inp, cp, planar, with_ws)
            rc = launch()
            if not planar and (not quad or cp == 3):           # the scalar form always writes the planar copy
                assert rc == L.DG_EUNSUPPORTED, what
                pm.done(what, written=False)
                assert not bool(db.done(what).any()), what
                continue
            L.check(rc, what)
            pmb = bits16(pm.done(what))
            dbv = db.done(what).numpy()
            if planar:
                pl = draw.done(what).numpy()
                for ch in range(1 + arch):
                    got = N.f64(pl[:, ch]) / scales[ch]        # (a power of two: the unscaled row, exactly)
                    if tier == "grid" and ch == 0:
                        n += ex(pl[:, ch], scales[ch] * r.d[ch], what + " planar d0")
                    else:
                        bounded("head_post_bwd", f"d{ch}", got, r.d[ch], r.b[ch], what)
                        n += got.size
                probs = N.pm_problems(pmb, pl, 1 + arch)
                assert not probs, what + ": " + "; ".join(probs)
                pm_given = pmb
            else:                                              # the same arithmetic without the planar stores: the same bits
                assert np.array_equal(pmb, pm_given), what + ": the pixel-major copy differs from the launch with a planar copy"
            n += pmb.size
            for ch in range(3):
                if ch > arch:
                    assert dbv[ch] == 0.0, what + f": dbias[{ch}] of an absent head is {dbv[ch]!r}"
                    continue
                bsum = r.b[ch].sum() + N.sum_bound(adds, np.abs(r.d[ch]).sum()) + hb * B * 2.0 ** -32
                bounded("head_post_bwd", f"dbias{ch}", dbv[ch], r.d[ch].sum(), bsum, what)
            if with_ws:
                assert not bool(ws.any()), what + ": bias_ws is not left zero"
                first = dbv.copy()
                db.t.zero_()
                L.check(launch(), what)
                again = db.done(what).numpy()
                assert not bool(ws.any()) and np.array_equal(first.view(np.uint32), again.view(np.uint32)), \
                    what + f": two launches through bias_ws give {first!r} and {again!r}"
    if tier == "grid" and arch == 0:                           # the bias sum, exact over the samples whose total is exact in any order
        nb = N.exact_prefix(r.d[0])
        assert nb >= 1
        for ws_on in ((False, True) if with_ws else (False,)):
            launch, draw, pm, db, ws, keep = run_head_bwd(L, inp, 2, True, ws_on, nb=nb)
            L.check(launch())
            n += ex(db.done("dbias exact")[:1], r.d[0][:nb].sum().reshape(1), f"dg_head_post_bwd {N.case_id(case)} dbias over {nb} samples ws={ws_on}")
            n += ex(draw.done("dbias exact")[:, 0], N.S_DEPTH * r.d[0][:nb], "planar")
    U.line("head_post_bwd", N.case_id(case), n)


# ---- dg_head_post_bwd2 ---------------------------------------------------------------------------------------------------------------
def run_head_bwd2(L, inp, cp, with_pm=True):
    lib, B, HW, arch = L.lib(), inp.B, inp.HW, inp.arch
    gout = dnp(np.stack([inp.t, inp.h1, inp.h2][:1 + arch], axis=1))
    mask = dnp(np.stack([inp.mp, inp.mi][:max(arch, 1)], axis=1))
    npx, nim, y, th = dnp(inp.npx), dnp(inp.nim), dnp(inp.go), dnp(inp.th)
    draw = Owned((B, 1 + arch, HW))
    pm = Owned((B, HW, max(cp, 1)), BF16)
    db = Owned((3,), fill=0.0)
    rc = lib.dg_head_post_bwd2(gout.data_ptr(), npx.data_ptr(), nim.data_ptr(), mask.data_ptr(), y.data_ptr(), th.data_ptr(), arch, inp.tau,
                               inp.c, B, HW, N.S_DEPTH, N.S_CONF, draw.ptr, db.ptr, pm.ptr if with_pm else None, cp, None)
    torch.cuda.synchronize()
    return rc, draw, pm, db


@pytest.mark.parametrize("case", N.HEAD_BWD2, ids=N.case_id)
def test_head_post_bwd2(L, case):
    tier, arch, B, HW = case
    inp = N.head_case_inputs(case)
    r = N.head_bwd2_case(inp)
    scales = (N.S_DEPTH, N.S_CONF, N.S_CONF)
    total = B * HW
    hb = min(1024, -(-total // 256))
    adds = -(-total // (hb * 256)) + 6 + 4 + hb + 1
    n = 0
    for cp in (2, 4):
        what = f"dg_head_post_bwd2 {N.case_id(case)} cp={cp}"
        rc, draw, pm, db = run_head_bwd2(L, inp, cp)
        L.check(rc, what)
        pl, pmb, dbv = draw.done(what).numpy(), bits16(pm.done(what)), db.done(what).numpy()
        for ch in range(3):
            if ch > arch:
                assert dbv[ch] == 0.0
                continue
            bounded("head_post_bwd2", f"row{ch}", N.f64(pl[:, ch]) / scales[ch], r.d[ch], r.b[ch], what)
            bounded("head_post_bwd2", f"dbias{ch}", dbv[ch], r.d[ch].sum(), r.b[ch].sum() + N.sum_bound(adds, np.abs(r.d[ch]).sum()), what)
        probs = N.pm_problems(pmb, pl, 1 + arch)
        assert not probs, what + ": " + "; ".join(probs)
        n += pl.size + pmb.size
    U.line("head_post_bwd2", N.case_id(case), n)


@pytest.mark.parametrize("cp", [0, 5, 8, -1])
def test_head_post_bwd2_refuses_a_channel_count_it_cannot_pad(L, cp):
    """the element-wise store writes channels 0..3: any other cp with a pixel-major copy is DG_EINVAL, nothing launched"""
    inp = N.head_inputs("grid", 2, 3, 21)
    lib = L.lib()
    rc, draw, pm, db = run_head_bwd2(L, inp, cp)
    assert rc == L.DG_EINVAL
    draw.done("refused", written=False)
    pm.done("refused", written=False)
    assert not bool(db.done("refused").any())
    rc, draw, pm, db = run_head_bwd2(L, inp, cp, with_pm=False)       # without the copy cp is not read
    L.check(rc)
    draw.done("no copy")
    pm.done("no copy", written=False)


# ---- the final conv ------------------------------------------------------------------------------------------------------------------
def check_final(L, dt, n, C, B):
    lib = L.lib()
    T_ = BF16 if dt == "bf16" else F32
    code = L.dtype_code(T_)
    k = N.final_inputs(B, n)
    what = f"final {dt} n={n} C={C} B={B}"
    d4, wf, bias = dnp(k.d4, T_), dnp(k.wf), dnp(np.asarray([k.bias]))
    up, rs, coef = dnp(k.up), dnp(k.rs), dnp(k.coef)
    cnt = 0
    y = Owned((B,))
    L.check(lib.dg_final_fwd(d4.data_ptr(), code, wf.data_ptr(), bias.data_ptr(), N.FINAL_SCALE, B, n, y.ptr, None), what)
    cnt += ex(y.done(what), N.final_fwd_ref(k.d4, k.wf, k.bias, N.FINAL_SCALE), what + " dg_final_fwd")
    for mode in MODES:                                         # onto a preloaded y, plain and in the arena
        acc = Acc(L, mode)
        ya = acc.take(B, preload=1.5)
        L.check(lib.dg_final_fwd_acc(d4.data_ptr(), code, wf.data_ptr(), bias.data_ptr(), N.FINAL_SCALE, B, n, ya.data_ptr(), None), what)
        acc.done(what)
        cnt += ex(ya.cpu(), N.final_fwd_ref(k.d4, k.wf, k.bias, N.FINAL_SCALE) + 1.5, what + f" dg_final_fwd_acc {mode}")
    dd4, db = Owned((B, n), T_), Owned((C,), fill=0.0)
    L.check(lib.dg_final_bwd_data(d4.data_ptr(), code, wf.data_ptr(), up.data_ptr(), rs.data_ptr(), N.FINAL_SCALE, B, n, C, dd4.ptr,
                                  db.ptr, None), what)
    g = N.final_dd4_ref(k.d4, k.wf, k.up, N.FINAL_SCALE)
    cnt += ex(dd4.done(what), N.f64(g), what + " dd4")
    adds = (B if B > 256 else -(-B // 4) + 3) + -(-n // C) + 1
    want, bound = N.final_dbias_ref(g, k.rs, C, adds)
    bounded("final_bwd_data", "dbias", db.done(what).numpy(), want, bound, what)
    out = Owned((n,))
    out.t.copy_(dnp(k.out0))
    L.check(lib.dg_batch_wsum(d4.data_ptr(), code, coef.data_ptr(), N.FINAL_SCALE, B, n, out.ptr, None), what)
    cnt += ex(out.done(what), N.wsum_ref(k.d4, k.coef, N.FINAL_SCALE, k.out0), what + " dg_batch_wsum")
    return cnt


@pytest.mark.parametrize("C", N.FINAL_C)
@pytest.mark.parametrize("ni", [0, 1, 2], ids=["one-lane", "three-workgroups", "two-slabs"])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_final_conv(L, dt, ni, C):
    n = N.FINAL_N[dt][ni]
    cnt = sum(check_final(L, dt, n, C, B) for B in N.FINAL_B)
    U.line("final_conv", f"{dt} n={n} C={C}", cnt)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_final_conv_scalar_form(L, dt):
    U.line("final_conv", f"{dt} n=105 C=7", check_final(L, dt, 105, 7, 3))


# ---- dg_gan_d_step / dg_gan_g_step ------------------------------------------------------------------------------------------------------
PRE = 2.0                                                      # what the scalars' accumulators hold on entry


def run_gan(L, metric, mode_g, yr, yf, w_gan, smoothing):
    lib, B = L.lib(), yf.size
    mi = N.METRICS.index(metric)
    a, b = dnp(yr), dnp(yf)
    if mode_g:
        dy, acc = Owned((B,)), Owned((1,), fill=PRE)
        L.check(lib.dg_gan_g_step(mi, a.data_ptr(), b.data_ptr(), B, w_gan, dy.ptr, acc.ptr, None))
        w = f"dg_gan_g_step {metric} B={B}"
        return N.Ref(dy=dy.done(w), acc=acc.done(w))
    dy, up, rs, acc, dfb = Owned((2 * B,)), Owned((2 * B,)), Owned((2 * B,)), Owned((3,), fill=PRE), Owned((1,), fill=PRE)
    L.check(lib.dg_gan_d_step(mi, smoothing, a.data_ptr(), b.data_ptr(), B, w_gan, dy.ptr, up.ptr, rs.ptr, acc.ptr, dfb.ptr, None))
    w = f"dg_gan_d_step {metric} B={B}"
    return N.Ref(dy=dy.done(w), up=up.done(w), rs=rs.done(w), acc=acc.done(w), dfb=dfb.done(w))


def gan_structure(g, B, what):
    """up = [1 .. 1 | dy_fake], rs = [dy_real | 1 .. 1]: the documented slices of dy, bit for bit"""
    dy, up, rs = (g[k].numpy().view(np.uint32) for k in ("dy", "up", "rs"))
    one = np.ones(B, dtype=F).view(np.uint32)
    assert np.array_equal(up[:B], one) and np.array_equal(up[B:], dy[B:]), what + ": up is not [1 | dy_fake]"
    assert np.array_equal(rs[B:], one) and np.array_equal(rs[:B], dy[:B]), what + ": rs is not [dy_real | 1]"


@pytest.mark.parametrize("B", [1, 64, 256])
@pytest.mark.parametrize("metric", N.EXACT_METRICS)
def test_gan_step_exact(L, metric, B):
    """dyadic logits, B and w_gan powers of two: dy, up, rs, the three scalars and dfinal_b bit for bit; hinge arguments planted
    exactly on the kink, where value and derivative are 0"""
    yr, yf = N.gan_exact_logits(B)
    n = 0
    for smoothing in (1.0, 0.5):
        what = f"{metric} B={B} smoothing={smoothing}"
        r, g = N.gan_ref(metric, 0, yr, yf, 0.5, smoothing), run_gan(L, metric, 0, yr, yf, 0.5, smoothing)
        n += ex(g.dy, r.dy, what + " D dy") + ex(g.up, r.up, what + " up") + ex(g.rs, r.rs, what + " rs")
        n += ex(g.acc, PRE + np.asarray([r.mr, r.mf, r.loss]), what + " D scalars") + ex(g.dfb, PRE + np.asarray([r.sum_dy]), what + " dfinal_b")
        gan_structure(g, B, what)
    r, g = N.gan_ref(metric, 1, yr, yf, 0.5), run_gan(L, metric, 1, yr, yf, 0.5, 1.0)
    n += ex(g.dy, r.dy, f"{metric} B={B} G dy") + ex(g.acc, PRE + np.asarray([r.loss]), f"{metric} B={B} G loss")
    U.line("gan_step", f"{metric} B={B}", n)


@pytest.mark.parametrize("B", [37, 300])
@pytest.mark.parametrize("metric", N.METRICS)
def test_gan_step_bounded(L, metric, B):
    """N(0, 1.5) logits; nsgan and ragan also saturated (+-25, +-90, 20 and the float after 20: softplus's switch, the overflowing
    exponential); the relativistic metrics with every logit of a side equal"""
    kinds = ["normal"] + (["saturated"] if metric in ("nsgan", "ragan") else []) + (["equal"] if metric in ("ragan", "rahinge", "ralsgan") else [])
    for kind in kinds:
        yr, yf = N.gan_random_logits(B, kind)
        for mode_g in (0, 1):
            what = f"{metric} B={B} {kind} {'G' if mode_g else 'D'}"
            r, b = N.gan_ref(metric, mode_g, yr, yf, 0.5, 0.9), N.gan_bounds(metric, mode_g, yr, yf, 0.5, 0.9)
            g = run_gan(L, metric, mode_g, yr, yf, 0.5, 0.9)
            name = "gan_g_step" if mode_g else "gan_d_step"
            bounded(name, "dy", g.dy.numpy(), r.dy, b.dy, what)
            acc = g.acc.numpy()
            scal = [("loss", r.loss, b.loss)] if mode_g else [("mean_real", r.mr, b.mr), ("mean_fake", r.mf, b.mf), ("loss", r.loss, b.loss)]
            for i, (k, want, bd) in enumerate(scal):
                bounded(name, k, acc[i], PRE + want, bd + N.D24 * abs(PRE + want), what)
            if not mode_g:
                gan_structure(g, B, what)
                bounded(name, "dfinal_b", g.dfb.numpy(), PRE + r.sum_dy, b.sum_dy + N.D24 * abs(PRE + r.sum_dy), what)


# ---- dg_final_gan_bwd ----------------------------------------------------------------------------------------------------------------
GAN_BWD = [(0, 33, 0), (0, 33, 1), (0, 128, 0), (0, 128, 1), (1, 65, 0)]   # (mode_g, B, r1): ns = 66 (a second sweep), 256 (the table), 65


def run_final_gan(L, dt, metric, mode_g, B, r1, k, yr, yf, w_gan, n, C, part):
    lib = L.lib()
    T_ = BF16 if dt == "bf16" else F32
    ns = B if mode_g else 2 * B
    d4, wf, a, b = dnp(k.d4, T_), dnp(k.wf), dnp(yr), dnp(yf)
    dy, up, rs = Owned((ns,)), Owned((ns,)), Owned((ns,))
    acc, dfb = Owned((3,), fill=0.0), Owned((1,), fill=0.0)
    dd4, db, dwf = Owned((ns, n), T_), Owned((C,), fill=0.0), Owned((n,))
    dwf.t.copy_(dnp(k.out0))
    dbp = Owned((n,)) if part else None
    rc = lib.dg_final_gan_bwd(N.METRICS.index(metric), mode_g, 1.0, a.data_ptr(), b.data_ptr(), B, w_gan, r1, dy.ptr, up.ptr if r1 else None,
                              rs.ptr if r1 else None, acc.ptr, dfb.ptr, d4.data_ptr(), L.dtype_code(T_), wf.data_ptr(), N.FINAL_SCALE, n, C,
                              dd4.ptr, db.ptr, dwf.ptr, dbp.ptr if part else None, None)
    L.check(rc)
    w = f"dg_final_gan_bwd {dt} {metric} G={mode_g} B={B} r1={r1} part={part}"
    if part:
        item = (L.DgWgradReduce * 1)()
        item[0].ws, item[0].dw, item[0].numel, item[0].splits, item[0].accumulate = dbp.ptr, db.ptr, C, n // C, 1
        L.check(lib.dg_wgrad_reduce(item, 1, None))
        dbp.done(w)
    out = N.Ref(dy=dy.done(w), acc=acc.done(w), dfb=dfb.done(w), dd4=dd4.done(w), db=db.done(w), dwf=dwf.done(w))
    if r1:
        out["up"], out["rs"] = up.done(w), rs.done(w)
    else:
        up.done(w, written=False)
        rs.done(w, written=False)
    return out


GAN_BWD_CASES = [(m,) + c for m in N.EXACT_METRICS for c in GAN_BWD] + [("nsgan", 0, 33, 1)]


@pytest.mark.parametrize("metric,mode_g,B,r1", GAN_BWD_CASES, ids=[N.case_id(c) for c in GAN_BWD_CASES])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_final_gan_bwd(L, dt, metric, mode_g, B, r1):
    """against the float64 reference directly.  The five exact metrics on dyadic logits (w_gan = B / 64: k = w_gan / B is 2^-6 for any
    B) give dyadic dy: dy, up, rs, dd4 and dwf bit for bit; the scalars, dbias and dbias_part + dg_wgrad_reduce bounded; nsgan
    bounded, its dd4 and dwf from the kernel's own dy."""
    exact = metric != "nsgan"
    n, C = (512 * 2 + 8, 24) if dt == "bf16" else (256 * 2 + 4, 12)
    ns = B if mode_g else 2 * B
    k = N.final_inputs(ns, n, seed=5)
    yr, yf = N.gan_exact_logits(B, small=True) if exact else N.gan_random_logits(B, "saturated")
    w_gan = B / 64.0
    r, bd = N.gan_ref(metric, mode_g, yr, yf, w_gan), N.gan_bounds(metric, mode_g, yr, yf, w_gan)
    cnt, runs = 0, []
    for part in (False, True, True):
        what = f"dg_final_gan_bwd {dt} {metric} G={mode_g} B={B} r1={r1} part={part}"
        g = run_final_gan(L, dt, metric, mode_g, B, r1, k, yr, yf, w_gan, n, C, part)
        runs.append(g)
        if exact:
            cnt += ex(g.dy, r.dy, what + " dy")
        else:
            bounded("final_gan_bwd", "dy", g.dy.numpy(), r.dy, bd.dy, what)
        dy = g.dy.numpy()
        if r1:
            gan_structure(g, B, what)
        scal = [r.loss] if mode_g else [r.mr, r.mf, r.loss]
        sb = [bd.loss] if mode_g else [bd.mr, bd.mf, bd.loss]
        bounded("final_gan_bwd", "scalars", g.acc.numpy()[:len(scal)], np.asarray(scal), np.asarray(sb) + N.TINY, what)
        if not mode_g:
            bounded("final_gan_bwd", "dfinal_b", g.dfb.numpy(), r.sum_dy, bd.sum_dy, what)
        u_ = g.up.numpy() if r1 else dy                        # the kernel's own per-sample vectors (equal to the reference's where exact)
        rs_ = g.rs.numpy() if r1 else np.ones(ns, dtype=F)
        gref = N.final_dd4_ref(k.d4, k.wf, u_, N.FINAL_SCALE)
        cnt += ex(g.dd4, N.f64(gref), what + " dd4")
        if exact:
            cnt += ex(g.dwf, N.wsum_ref(k.d4, r.dy, N.FINAL_SCALE, k.out0), what + " dwf")
        else:
            terms = N.FINAL_SCALE * np.abs(N.f64(dy))[:, None] * np.abs(N.f64(k.d4))
            bounded("final_gan_bwd", "dwf", g.dwf.numpy(), N.wsum_ref(k.d4, dy, N.FINAL_SCALE, k.out0),
                    (-(-ns // 8) + 7 + 3) * N.D24 * (terms.sum(axis=0) + np.abs(N.f64(k.out0))), what)
        adds = -(-ns // 8) + 7 + n // C + 1
        want, bound = N.final_dbias_ref(gref, rs_, C, adds)
        bounded("final_gan_bwd", "dbias (part)" if part else "dbias", g.db.numpy(), want, bound, what)
    a, b = runs[1], runs[2]                                    # dbias_part + dg_wgrad_reduce: two launches agree bit for bit
    for key in ("dy", "dd4", "dwf", "db", "acc"):
        assert torch.equal(a[key].view(torch.int16 if a[key].dtype == BF16 else torch.int32),
                           b[key].view(torch.int16 if b[key].dtype == BF16 else torch.int32)), f"{key} differs between two launches"
    U.line("final_gan_bwd", f"{dt} {metric} G={mode_g} B={B} r1={r1}", cnt)


# ---- dg_pl_penalty, dg_mean_acc, dg_scale ----------------------------------------------------------------------------------------------
def run_pl(L, dz, w, ema):
    B, K = dz.shape
    d = dnp(dz)
    pe, v, acc = Owned((1,), fill=ema), Owned((B, K)), Owned((2,), fill=1.0)
    rc = L.lib().dg_pl_penalty(d.data_ptr(), B, K, w, pe.ptr, v.ptr, acc.ptr, None)
    torch.cuda.synchronize()
    return rc, pe, v, acc


@pytest.mark.parametrize("K", N.PL_K)
@pytest.mark.parametrize("B", N.PL_B)
def test_pl_penalty(L, B, K):
    dz = N.pl_inputs(B, K)
    for ema in (0.0, 0.7):
        what = f"dg_pl_penalty B={B} K={K} ema={ema}"
        r, b = N.pl_ref(dz, 2.0, N.w32(ema)), N.pl_bounds(dz, 2.0, ema)
        rc, pe, v, acc = run_pl(L, dz, 2.0, ema)
        L.check(rc, what)
        a = pe.done(what).numpy()
        bounded("pl_penalty", "baseline", a, r.a, b.a, what)
        got = acc.done(what).numpy()
        bounded("pl_penalty", "acc baseline", got[0], 1.0 + r.a, b.a + N.D24 * abs(1.0 + r.a), what)
        bounded("pl_penalty", "acc penalty", got[1], 1.0 + r.pen, b.pen + N.D24 * abs(1.0 + r.pen), what)
        vv = v.done(what).numpy()
        assert not np.isnan(vv).any(), what
        bounded("pl_penalty", "v", vv, r.v, b.v, what)
        if B >= 3:
            assert not vv[1].any(), what + ": v of the all-zero sample is not 0"
    # equal lengths with the baseline at their common value: a = ema, every deviation 0 - everything exact
    dz = np.full((B, 1), 0.75, dtype=F) * np.where(np.arange(B) % 2, -1, 1)[:, None].astype(F)
    rc, pe, v, acc = run_pl(L, dz, 2.0, 0.75)
    L.check(rc)
    ex(pe.done("pl exact"), np.asarray([0.75]), "pl_ema")
    ex(acc.done("pl exact"), np.asarray([1.75, 1.0]), "acc")
    assert not v.done("pl exact").numpy().any()


def test_pl_penalty_refuses_more_samples_than_its_table(L):
    rc, pe, v, acc = run_pl(L, N.pl_inputs(257, 8), 2.0, 0.5)
    assert rc == L.DG_EINVAL
    v.done("refused", written=False)
    assert float(pe.done("refused")) == 0.5 and acc.done("refused").tolist() == [1.0, 1.0]


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_mean_acc(L, n):
    x = N.mean_inputs(n)
    acc = Owned((1,), fill=3.0)
    L.check(L.lib().dg_mean_acc(dnp(x).data_ptr(), n, acc.ptr, None))
    ex(acc.done("mean_acc"), np.asarray([3.0 + N.f64(x).sum() / n]), f"dg_mean_acc n={n}")


@pytest.mark.parametrize("n", [1, 256, 257])
def test_scale(L, n):
    """one rounding: fl32(a x)"""
    x = np.random.default_rng(n).standard_normal(n).astype(F)
    a = F(1.0 / 3.0)
    xd, y = dnp(x), Owned((n,))
    L.check(L.lib().dg_scale(xd.data_ptr(), float(a), n, y.ptr, None))
    ex(y.done("scale"), N.f64(a * x), f"dg_scale n={n}")


def test_zz_ratio_table():
    """largest |got - ref| / bound per bounded output over every case above (each assertion already demands < 1)"""
    print("\n" + N.format_table())
    for (k, t), slot in N.RATIOS.items():
        if k == N.TABLE_KEY:
            assert all(q < 1.0 for q in slot.values()), (t, slot)
