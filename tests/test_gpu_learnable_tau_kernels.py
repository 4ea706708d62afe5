"""The learnable-temperature head kernels held per element: dg_head_post_fwd_lt / _fwd_sum_lt / _bwd_lt / _bwd_aug_lt
(csrc/head_post.hip, head_post.h) against the float64 restatement and the criteria of tests/learnable_tau_ref.py (derived there,
vouched for on the CPU by tests/test_learnable_tau_cpu.py), in the manner of tests/test_gpu_net_end.py: every launch goes through the
C ABI, every output starts as sentinels between guards, no tolerance is invented.  The last test prints the largest
|got - ref| / bound per bounded output (-s).

Measured on an MI355X, largest |got - ref| / bound over every case of this file:
    head_post_fwd_lt   t 0.964   dsum 0.070
    head_post_bwd_lt   d0 0.730  d1 0.741  d2 0.733  dbias0 0.021  dbias1 0.086  dbias2 0.031  dtau0 0.069  dtau1 0.065
(EXP_ULPS, RCP_ULPS and LOG1P_ULPS of tests/net_end_ref.py are borrowed figures, not measured; no run contradicted them.)"""
import functools

import numpy as np
import pytest
import torch

from tests import learnable_tau_ref as T
from tests import net_end_ref as N
from tests.gpu_guard_util import BF16, DEV, Acc, Owned
from tests.test_gpu_net_end import bits16, bounded, dnp, ex

pytestmark = pytest.mark.gpu
F = np.float32
KERNEL = "head_post_bwd_lt"


@pytest.fixture(scope="module")
def L():
    from dusty_gan_amd import _lib
    _lib.lib()
    return _lib


def weights(wp, wi, arch):
    return torch.tensor([wp, wi][:arch], dtype=torch.float32, device=DEV)


# ---- forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", N.TIERS)
@pytest.mark.parametrize("arch,wp,wi", [(1, -3.0, 0.0), (2, 0.0, 2.5), (2, 2.5, -3.0)])
@pytest.mark.parametrize("HW", [21, 1024, 4096])
def test_head_post_fwd_lt(L, HW, arch, wp, wi, tier):
    """t within tanh's bound, the masks and the depth exact - and, hard masks not depending on a positive slope, the very bits the
    fixed-tau entry point stores"""
    lib = L.lib()
    inp = T.lt_inputs(tier, arch, 3, HW)
    assert T.excluded_pixels_lt(inp, wp, wi) == 0
    B = inp.B
    heads = np.stack([inp.raw, inp.h1, inp.h2][:1 + arch], axis=1)
    npx, nim, w = dnp(inp.npx), dnp(inp.nim), weights(wp, wi, arch)
    n = 0
    for training in (1, 0):
        ref = N.head_fwd_case(inp, training)
        for with_sum in (False, True):
            what = f"dg_head_post_fwd{'_sum' if with_sum else ''}_lt {tier} arch={arch} HW={HW} w=({wp},{wi}) training={training}"
            outs = []
            for lt in (True, False):
                gout = Owned((B, 1 + arch, HW))
                gout.t.copy_(dnp(heads))
                mask, depth = Owned((B, arch, HW)), Owned((B, HW))
                acc = Acc(L, "plain")
                dsum = acc.take(B) if with_sum else None
                head = (gout.ptr, npx.data_ptr(), nim.data_ptr(), arch, training)
                tail = (inp.c, B, HW, mask.ptr, depth.ptr) + ((dsum.data_ptr(),) if with_sum else ()) + (None,)
                if lt:
                    rc = (lib.dg_head_post_fwd_sum_lt if with_sum else lib.dg_head_post_fwd_lt)(*head, w.data_ptr(), T.INV_MIN, *tail)
                else:
                    rc = (lib.dg_head_post_fwd_sum if with_sum else lib.dg_head_post_fwd)(*head, 1.0, *tail)
                torch.cuda.synchronize()
                if with_sum and HW % 256:
                    assert rc == L.DG_EUNSUPPORTED, what
                    depth.done(what, written=False)
                    continue
                L.check(rc, what)
                acc.done(what)
                outs.append((gout.done(what).numpy(), mask.done(what), depth.done(what).numpy(), dsum.cpu().numpy() if with_sum else None))
            if not outs:
                continue
            g, mk, d, ds = outs[0]
            assert np.array_equal(g[:, 1:].view(np.uint32), heads[:, 1:].view(np.uint32)), what + ": the logits were touched"
            bounded("head_post_fwd_lt", "t", g[:, 0], ref.t, ref.bt, what)
            n += ex(mk[:, 0], ref.mp, what + " pixel mask")
            if arch == 2:
                n += ex(mk[:, 1], ref.mi, what + " image mask")
            N.same_values(what + " depth", d, N.depth_of(g[:, 0], ref.m, inp.c))
            if with_sum:
                adds = N.head_sum_adds(HW, HW % 1024 == 0)
                bounded("head_post_fwd_lt", "dsum", ds, N.f64(d).sum(axis=1), N.sum_bound(adds, np.abs(N.f64(d)).sum(axis=1)) + adds * 2.0 ** -33,
                        what)
            g0, mk0, d0, ds0 = outs[1]
            assert np.array_equal(g.view(np.uint32), g0.view(np.uint32)) and torch.equal(mk, mk0), what + ": differs from the fixed-tau form"
            assert np.array_equal(d.view(np.uint32), d0.view(np.uint32)), what + ": depth differs from the fixed-tau form"


# ---- backward --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def bwd_case(case):
    inp = T.lt_case_inputs(case)
    return inp, T.lt_bwd_ref(inp, case[4], case[5])


def run_bwd_lt(L, inp, wp, wi, cp, planar, with_ws, inv_min=T.INV_MIN, go=None):
    lib, HW, arch, B = L.lib(), inp.HW, inp.arch, inp.B
    gout = dnp(np.stack([inp.t, inp.h1, inp.h2][:1 + arch], axis=1))
    mask = dnp(np.stack([inp.mp, inp.mi][:arch], axis=1))
    npx, nim = dnp(inp.npx), dnp(inp.nim)
    go = dnp(inp.go) if go is None else go
    w = weights(wp, wi, arch)
    draw = Owned((B, 1 + arch, HW)) if planar else None
    pm = Owned((B, HW, cp), BF16) if cp else None
    db, dt = Owned((3,), fill=0.0), Owned((2,), fill=0.0)
    ws = torch.zeros(B * 1024, device=DEV) if with_ws else None
    keep = (gout, mask, npx, nim, go, w)

    def launch():
        rc = lib.dg_head_post_bwd_lt(gout.data_ptr(), npx.data_ptr(), nim.data_ptr(), mask.data_ptr(), go.data_ptr(), arch, w.data_ptr(),
                                     inv_min, dt.ptr, inp.c, B, HW, N.S_DEPTH, N.S_CONF, draw.ptr if planar else None, db.ptr,
                                     pm.ptr if cp else None, cp, L.ptr(ws), None)
        torch.cuda.synchronize()
        return rc
    return launch, draw, pm, db, dt, ws, keep


@pytest.mark.parametrize("case", T.LT_BWD, ids=T.lt_case_id)
def test_head_post_bwd_lt(L, case):
    tier, arch, B, HW, wp, wi = case
    inp, r = bwd_case(case)
    assert T.excluded_pixels_lt(inp, wp, wi) == 0
    scales = (N.S_DEPTH, N.S_CONF, N.S_CONF)
    quad = HW % 4 == 0
    with_ws = HW >= 4096
    adds, hb = N.head_bwd_adds(B, HW, quad)
    fixed = quad and with_ws and hb > 1                        # the 32.32 slots and tickets; otherwise float atomics
    nfix = hb * B if fixed else 0
    ws_ = (wp, wi)
    n = 0
    for cp in ((2, 4) if B == 3 else (4,)):
        what = f"dg_head_post_bwd_lt {T.lt_case_id(case)} cp={cp}"
        launch, draw, pm, db, dt, ws, keep = run_bwd_lt(L, inp, wp, wi, cp, True, with_ws)
        L.check(launch(), what)
        pl = draw.done(what).numpy()
        for ch in range(1 + arch):
            got = N.f64(pl[:, ch]) / scales[ch]                # (a power of two: the unscaled row, exactly)
            bounded(KERNEL, f"d{ch}", got, r.d[ch], r.b[ch], what)
            n += got.size
        probs = N.pm_problems(bits16(pm.done(what)), pl, 1 + arch)
        assert not probs, what + ": " + "; ".join(probs)
        dbv, dtv = db.done(what).numpy(), dt.done(what).numpy()
        for ch in range(3):
            if ch > arch:
                assert dbv[ch] == 0.0, what
                continue
            bsum = r.b[ch].sum() + N.sum_bound(adds, np.abs(r.d[ch]).sum()) + nfix * 2.0 ** -33
            bounded(KERNEL, f"dbias{ch}", dbv[ch], r.d[ch].sum(), bsum, what)
        want = []
        for k in range(2):
            if k >= arch:
                assert dtv[k] == 0.0, what + f": dtau_w[{k}] of an absent sigmoid is {dtv[k]!r}"
                continue
            val, bnd = T.dtau_ref(r, k, ws_[k], adds, nfix)
            want.append((val, bnd))
            bounded(KERNEL, f"dtau{k}", dtv[k], val, bnd, what)
        if with_ws:
            assert not bool(ws.any()), what + ": bias_ws is not left zero"
        # accumulation: a second launch adds the same sums once more
        first = (dbv.copy(), dtv.copy())
        L.check(launch(), what)
        dbv2, dtv2 = db.done(what).numpy(), dt.done(what).numpy()
        for k, (val, bnd) in enumerate(want):
            bounded(KERNEL, f"dtau{k}", dtv2[k], 2.0 * val, 2.0 * bnd + 2.0 * N.D24 * abs(val), what + " second launch")
        if with_ws:
            assert not bool(ws.any()), what + ": bias_ws is not left zero"
        if fixed:                                              # two runs through the slots: the same bits
            db.t.zero_(); dt.t.zero_()
            L.check(launch(), what)
            again = (db.done(what).numpy(), dt.done(what).numpy())
            assert np.array_equal(first[0].view(np.uint32), again[0].view(np.uint32)) and \
                np.array_equal(first[1].view(np.uint32), again[1].view(np.uint32)), what + f": two runs give {first!r} and {again!r}"
        if cp == 4 and quad:                                   # the pixel-major copy alone, no dbias: the same copy, the same dtau sums
            launch2, _, pm2, db2, dt2, ws2, keep2 = run_bwd_lt(L, inp, wp, wi, cp, False, with_ws)
            L.check(launch2(), what)
            assert np.array_equal(bits16(pm2.done(what)), bits16(pm.t.cpu())), what + ": the copy without a planar output differs"
            if fixed:
                assert np.array_equal(dt2.done(what).numpy().view(np.uint32), first[1].view(np.uint32)), what
    assert n == (1 + arch) * B * HW * (2 if B == 3 else 1)      # every element of every plane was held to its bound


@pytest.mark.parametrize("arch", [1, 2])
@pytest.mark.parametrize("HW", [21, 4096])
def test_fixed_tau_entry_point_gives_the_same_bits(L, HW, arch):
    """tau_max = 2 and w = -30 for both sigmoids: softplus(w) = 9e-14 is below half an ulp of 1 / tau_max = 0.5, so the slope the
    kernel forms IS 0.5f whatever log1pf's and __expf's last bits - the float the old entry point forms from tau = 2.  draw, draw_pm
    and dbias must then be the old entry point's, bit for bit (and through the slots, dbias too)."""
    lib = L.lib()
    inp = N.head_inputs("random", arch, 3, HW, seed=arch, tau=2.0)
    cp = 2 if arch == 1 else 4
    with_ws = HW >= 4096
    launch, draw, pm, db, dt, ws, keep = run_bwd_lt(L, inp, -30.0, -30.0, cp, True, with_ws, inv_min=0.5)
    L.check(launch())
    gout, mask, npx, nim, go, w = keep
    draw0, pm0, db0 = Owned((inp.B, 1 + arch, HW)), Owned((inp.B, HW, cp), BF16), Owned((3,), fill=0.0)
    ws0 = torch.zeros(inp.B * 1024, device=DEV) if with_ws else None
    L.check(lib.dg_head_post_bwd(gout.data_ptr(), npx.data_ptr(), nim.data_ptr(), mask.data_ptr(), go.data_ptr(), arch, 2.0, inp.c,
                                 inp.B, HW, N.S_DEPTH, N.S_CONF, draw0.ptr, db0.ptr, pm0.ptr, cp, L.ptr(ws0), None))
    torch.cuda.synchronize()
    what = f"old vs _lt arch={arch} HW={HW}"
    a, b = draw.done(what).numpy(), draw0.done(what).numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what + ": draw"
    assert float(np.abs(a[:, 1:]).max()) > 0
    assert np.array_equal(bits16(pm.done(what)), bits16(pm0.done(what))), what + ": draw_pm"
    if with_ws:                                                # (float atomics arrive in any order: bits only through the slots)
        assert np.array_equal(db.done(what).numpy().view(np.uint32), db0.done(what).numpy().view(np.uint32)), what + ": dbias"
    else:
        # one block per sample forms the same partial in both launches; only the order of the B = 3 float atomics onto dbias may
        # differ: two roundings of at most D24 sum |d| each
        got, old = db.done(what).numpy(), db0.done(what).numpy()
        for ch, sc in enumerate((N.S_DEPTH, N.S_CONF, N.S_CONF)[:1 + arch]):
            assert abs(float(got[ch]) - float(old[ch])) <= 2.0 * N.D24 * float(np.abs(N.f64(a[:, ch])).sum()) / sc, (what, ch)


@pytest.mark.parametrize("B,H,W", T.LT_AUG, ids=lambda v: str(v))
@pytest.mark.parametrize("arch", [1, 2])
def test_head_post_bwd_aug_lt_equals_the_plain_form_on_the_materialised_upstream(L, arch, B, H, W):
    """DiffAugment's adjoint gather inside the launch (full policy) against dg_head_post_bwd_lt fed the upstream dg_diffaug_bwd_pre
    writes: one kernel body, the same gather function, the same grid - the same bits in every output, the temperature sums'
    included (both shapes put several blocks on a sample: the fixed-point slots)"""
    from dusty_gan_amd.utils.diff_augment import DiffAugment
    from oracle import dusty_oracle as O
    lib = L.lib()
    g = torch.Generator().manual_seed(17 + arch + W)
    HW = H * W
    inp = T.lt_inputs("random", arch, B, HW, seed=3)
    wp, wi = (2.5, -3.0) if arch == 2 else (0.0, 0.0)
    A = DiffAugment()
    gy = torch.randn(B, 1, H, W, generator=g).to(DEV)
    gsum = torch.randn(B, generator=g).to(DEV)
    rpd = DiffAugment.params_to_device(O.draw_augment_params(B, H, W, g), DEV)
    ddepth = A.backward_pre(gy, rpd, gsum).contiguous()
    args, keep_args = A._args(rpd, B, gy.device)
    cp = 2 if arch == 1 else 4
    launch, draw, pm, db, dt, ws, keep = run_bwd_lt(L, inp, wp, wi, cp, True, True, go=ddepth.view(B, HW))
    L.check(launch())
    gout, mask, npx, nim, go, w = keep
    draw1, pm1, db1, dt1 = Owned((B, 1 + arch, HW)), Owned((B, HW, cp), BF16), Owned((3,), fill=0.0), Owned((2,), fill=0.0)
    ws1 = torch.zeros(B * 1024, device=DEV)
    L.check(lib.dg_head_post_bwd_aug_lt(gout.data_ptr(), npx.data_ptr(), nim.data_ptr(), mask.data_ptr(), gy.data_ptr(), *args, A.mask,
                                        gsum.data_ptr(), arch, w.data_ptr(), T.INV_MIN, dt1.ptr, inp.c, B, H, W, N.S_DEPTH, N.S_CONF,
                                        draw1.ptr, db1.ptr, pm1.ptr, cp, ws1.data_ptr(), None))
    torch.cuda.synchronize()
    what = f"dg_head_post_bwd_aug_lt arch={arch} {B}x{H}x{W}"
    assert N.head_bwd_adds(B, HW, True)[1] > 1
    for name, x, y in (("draw", draw, draw1), ("dbias", db, db1), ("dtau_w", dt, dt1)):
        a, b = x.done(what).numpy(), y.done(what).numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{what}: {name} differs, {np.abs(a - b).max()!r} at most"
    assert np.array_equal(bits16(pm.done(what)), bits16(pm1.done(what))), what + ": draw_pm differs"
    assert float(np.abs(dt.t.cpu().numpy()[:arch]).min()) > 0 and not bool(ws1.any())
    # the plain launch itself is held to the float64 reference on this upstream
    inp2 = N.Ref(dict(inp, go=ddepth.view(B, HW).cpu().numpy()))
    r = T.lt_bwd_ref(inp2, wp, wi)
    adds, hb = N.head_bwd_adds(B, HW, True)
    for k, wk in enumerate((wp, wi)[:arch]):
        val, bnd = T.dtau_ref(r, k, wk, adds, hb * B)
        bounded(KERNEL, f"dtau{k}", dt.t.cpu().numpy()[k], val, bnd, what)


def test_lt_entry_points_refuse_bad_arguments(L):
    lib = L.lib()
    B, HW, arch = 2, 256, 2
    z = lambda *s: torch.zeros(*s, device=DEV)
    gout, npx, nim, mask, depth, go = z(B, 3, HW), z(B, HW), z(B), z(B, 2, HW), z(B, HW), z(B, HW)
    draw, db, dt, dsum = Owned((B, 3, HW)), Owned((3,), fill=0.0), Owned((2,), fill=0.0), z(B)
    w = weights(0.0, 0.0, 2)
    uf, qi = z(B), torch.zeros(B, dtype=torch.int32, device=DEV)      # DiffAugment's draws (policy 0: none is read)
    EINVAL = L.DG_EINVAL

    def fwd(wptr, inv_min, a=arch):
        return (lib.dg_head_post_fwd_lt(gout.data_ptr(), npx.data_ptr(), nim.data_ptr(), a, 1, wptr, inv_min, -1.0, B, HW, mask.data_ptr(),
                                        depth.data_ptr(), None),
                lib.dg_head_post_fwd_sum_lt(gout.data_ptr(), npx.data_ptr(), nim.data_ptr(), a, 1, wptr, inv_min, -1.0, B, HW,
                                            mask.data_ptr(), depth.data_ptr(), dsum.data_ptr(), None))

    def bwd(wptr, inv_min, dptr, a=arch):
        aug = (go.data_ptr(), uf.data_ptr(), uf.data_ptr(), qi.data_ptr(), qi.data_ptr(), qi.data_ptr(), qi.data_ptr(), 0, None)
        return (lib.dg_head_post_bwd_lt(gout.data_ptr(), npx.data_ptr(), nim.data_ptr(), mask.data_ptr(), go.data_ptr(), a, wptr, inv_min,
                                        dptr, -1.0, B, HW, 0.25, 0.5, draw.ptr, db.ptr, None, 0, None, None),
                lib.dg_head_post_bwd_aug_lt(gout.data_ptr(), npx.data_ptr(), nim.data_ptr(), mask.data_ptr(), *aug, a, wptr, inv_min,
                                            dptr, -1.0, B, 4, HW // 4, 0.25, 0.5, draw.ptr, db.ptr, None, 0, None, None))
    for bad in (fwd(None, 1.0), fwd(w.data_ptr(), 0.0), fwd(w.data_ptr(), -1.0), fwd(w.data_ptr(), float("nan")), fwd(w.data_ptr(), 1.0, 0),
                bwd(None, 1.0, dt.ptr), bwd(w.data_ptr(), 1.0, None), bwd(w.data_ptr(), 0.0, dt.ptr), bwd(w.data_ptr(), -2.0, dt.ptr),
                bwd(w.data_ptr(), 1.0, dt.ptr, 0)):
        assert bad == (EINVAL, EINVAL), bad
    torch.cuda.synchronize()
    draw.done("refused", written=False)
    assert not bool(db.done("refused").any()) and not bool(dt.done("refused").any()) and not bool(depth.any())
    assert fwd(w.data_ptr(), 1.0) == (L.DG_OK, L.DG_OK) and bwd(w.data_ptr(), 1.0, dt.ptr) == (L.DG_OK, L.DG_OK)
    torch.cuda.synchronize()


def test_zz_print_ratio_table(L):
    print("\n" + N.format_table())
