"""The image end of the discriminator held per element: BlurVH, DiffAugment, R1's turn-around, the HeadGradAug gather and the
per-sample sums (csrc/blur_aug.hip, csrc/diffaug.h, csrc/head_post.hip) against the float64 oracle on the exact data of
tests/image_exact_util.py.  fp32 outputs bit for bit, bf16 outputs the round-to-nearest-even of the reference, every sum equal -
into a plain buffer (float atomics) and into the accumulator arena (32.32 fixed point).  Every launch goes through the C ABI;
every output sits between two guards of sentinels and starts as sentinels.  tests/test_image_exact_cpu.py vouches for the inputs."""
import pytest
import torch

from tests import image_exact_util as U
from tests.gpu_guard_util import BF16, DEV, F32, MODES, Acc, Owned, dev   # (shared with tests/test_gpu_net_end.py)

pytestmark = pytest.mark.gpu
MEAN_ACC_N = 4


@pytest.fixture(scope="module")
def L():
    from dusty_gan_amd import _lib
    _lib.lib()
    return _lib


def rp_dev(rp):
    """(u_b, u_c, t_h, t_w, o_x, o_y) pointers in the C ABI's order, and the tensors that own them"""
    keep = [dev(rp[k]) for k in ("u_b", "u_c")] + [dev(rp[k], torch.int32) for k in ("t_h", "t_w", "o_x", "o_y")]
    return tuple(t.data_ptr() for t in keep), keep


def compare(got, ref64, what):
    """fp32: bit for bit; bf16: the RNE of the reference (equal to it wherever it is a bf16 number)"""
    return U.assert_rne(got, ref64, what) if got.dtype == BF16 else U.assert_exact(got, ref64, what)


def ids(shapes):
    return ["x".join(str(v) for v in s) for s in shapes]


# ---- a. BlurVH forward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [1, 0], ids=["ring", "reflect"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,W", U.BLUR_FWD, ids=ids(U.BLUR_FWD))
def test_blur_fwd(L, H, W, dtype, ring):
    lib, code = L.lib(), L.dtype_code(dtype)
    B = U.blur_batch(H, W)
    k = U.blur(H, W, B)
    x, ref = dev(k.x), k.fwd(bool(ring))
    what = f"dg_blur_fwd {H}x{W} {dtype} ring={ring}"
    out = Owned((B, H, W, 2), dtype)
    L.check(lib.dg_blur_fwd(x.data_ptr(), out.ptr, code, B, H, W, ring, None))
    n = U.assert_exact(out.done(what), ref, what)            # both types: on this data the outputs are bf16 numbers
    for mean_n in U.MEAN_N:
        src = U.mean_src(mean_n)
        sd, macc, out2 = dev(src), Owned((1,), fill=3.0), Owned((B, H, W, 2), dtype)
        rc = lib.dg_blur_fwd_mean(x.data_ptr(), out2.ptr, code, B, H, W, ring, sd.data_ptr(), mean_n, macc.ptr, None)
        if W % 4 or W < 8:
            assert rc == L.DG_EUNSUPPORTED
            out2.done(what + " refused", written=False)
            assert float(macc.done(what)) == 3.0
            continue
        L.check(rc)
        n += U.assert_exact(out2.done(what + " +mean"), ref, what + " +mean")
        n += U.assert_exact(macc.done(what + " rider"), 3.0 + src.sum().view(1) / mean_n, what + " rider")
    U.line("blur_fwd", what, n)


# ---- b. BlurVH adjoint -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [1, 0], ids=["ring", "reflect"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,W", U.BLUR_ADJ, ids=ids(U.BLUR_ADJ))
def test_blur_bwd(L, H, W, dtype, ring):
    lib, code = L.lib(), L.dtype_code(dtype)
    B = U.blur_batch(H, W)
    k = U.blur(H, W, B)
    what = f"dg_blur_bwd {H}x{W} {dtype} ring={ring}"
    d, dx = dev(k.d, dtype), Owned((B, 1, H, W))
    L.check(lib.dg_blur_bwd(d.data_ptr(), code, dx.ptr, B, H, W, ring, None))
    n = U.assert_exact(dx.done(what), k.adj(bool(ring)), what)
    if (H * W) % 1024:                                        # the R1 form refuses, and writes nothing
        dx2, ssq = Owned((B, 1, H, W)), Owned((B,), fill=0.0)
        assert lib.dg_blur_bwd_r1(d.data_ptr(), code, dx2.ptr, U.OSCALE, ssq.ptr, B, H, W, ring, None) == L.DG_EUNSUPPORTED
        dx2.done(what + " r1 refused", written=False)
        assert not bool(ssq.done(what).any())
    U.line("blur_bwd", what, n)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ring", [1, 0], ids=["ring", "reflect"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,W", U.BLUR_R1SUM, ids=ids(U.BLUR_R1SUM))
def test_blur_bwd_r1(L, H, W, dtype, ring, mode):
    lib, code = L.lib(), L.dtype_code(dtype)
    B = U.blur_batch(H, W)
    k = U.blur(H, W, B)
    what = f"dg_blur_bwd_r1 {H}x{W} {dtype} ring={ring} {mode}"
    acc = Acc(L, mode)
    d, dx, ssq = dev(k.d, dtype), Owned((B, 1, H, W)), acc.take(B)
    L.check(lib.dg_blur_bwd_r1(d.data_ptr(), code, dx.ptr, U.OSCALE, ssq.data_ptr(), B, H, W, ring, None))
    n = U.assert_exact(dx.done(what), U.OSCALE * k.adj(bool(ring)), what)
    acc.done(what)
    n += U.assert_exact(ssq.cpu(), k.ssq(bool(ring)), what + " ssq")
    U.line("blur_bwd_r1", what, n)


@pytest.mark.parametrize("ring", [1, 0], ids=["ring", "reflect"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,W,draws", U.AUGSUM, ids=ids(U.AUGSUM))
def test_blur_bwd_augsum(L, H, W, draws, dtype, ring):
    """every window (t_h, o_x, o_y) the shape can draw, and rows shifted out altogether, as one batch; 4, 2 and 1 rows per block"""
    lib, code = L.lib(), L.dtype_code(dtype)
    a = U.aug(H, W, draws)
    B = a.B
    k = U.blur(H, W, B)
    ref = k.adj(bool(ring))
    d = dev(k.d, dtype)
    args, keep = rp_dev(a.rp)
    n = 0
    for policy in U.policies_for(H, W):
        for mode in MODES:
            what = f"dg_blur_bwd_augsum {H}x{W} {dtype} ring={ring} {policy} {mode}"
            acc = Acc(L, mode)
            dx, gsum = Owned((B, 1, H, W)), acc.take(B)
            L.check(lib.dg_blur_bwd_augsum(d.data_ptr(), code, dx.ptr, args[2], args[4], args[5], L.policy_mask(U.POLICIES[policy]),
                                           gsum.data_ptr(), B, H, W, ring, None))
            n += U.assert_exact(dx.done(what), ref, what)
            acc.done(what)
            n += U.assert_exact(gsum.cpu(), U.window_sum64(ref, a.rp, policy), what + " gsum")
    U.line("blur_bwd_augsum", f"{H}x{W} {dtype} ring={ring}", n)


# ---- c. R1's turn-around ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ring", [1, 0], ids=["ring", "reflect"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,W", U.TANGENT, ids=ids(U.TANGENT))
def test_r1_tangent(L, H, W, dtype, ring, mode):
    lib, code = L.lib(), L.dtype_code(dtype)
    B = 3
    k = U.blur(H, W, B)
    d = dev(k.d, dtype)
    n = 0
    for with_mean in (True, False):
        what = f"dg_blur_r1_tangent {H}x{W} {dtype} ring={ring} {mode} mean_acc={with_mean}"
        acc = Acc(L, mode)
        out, ssq = Owned((B, H, W, 2), dtype), acc.take(B)
        macc = acc.take(1) if with_mean else None
        L.check(lib.dg_blur_r1_tangent(d.data_ptr(), code, out.ptr, U.OSCALE, ssq.data_ptr(), L.ptr(macc), MEAN_ACC_N, B, H, W, ring, None))
        n += compare(out.done(what), k.tangent(bool(ring)), what)
        acc.done(what)
        n += U.assert_exact(ssq.cpu(), k.ssq(bool(ring)), what + " ssq")
        if with_mean:
            n += U.assert_exact(macc.cpu(), k.ssq(bool(ring)).sum().view(1) / MEAN_ACC_N, what + " mean")
    U.line("r1_tangent", f"{H}x{W} {dtype} ring={ring} {mode}", n)


# ---- d. DiffAugment forward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,draws", U.AUG, ids=ids(U.AUG))
def test_diffaug_fwd(L, H, W, draws):
    lib = L.lib()
    a = U.aug(H, W, draws)
    B, x = a.B, dev(a.x)
    args, keep = rp_dev(a.rp)
    n = 0
    for policy in U.policies_for(H, W):
        mask, contrast = L.policy_mask(U.POLICIES[policy]), "contrast" in U.POLICIES[policy]
        ref = a.y(policy)
        what = f"dg_diffaug_fwd {H}x{W} {policy}"
        y, xsum = Owned((B, 1, H, W)), Owned((B,))          # the plain form zeroes xsum itself - when it needs it
        L.check(lib.dg_diffaug_fwd(x.data_ptr(), *args, mask, B, H, W, xsum.ptr, y.ptr, None))
        n += U.assert_exact(y.done(what), ref, what)
        got = xsum.done(what + " xsum", written=contrast)
        if contrast:
            n += U.assert_exact(got, a.xsum, what + " xsum")
        for mode in MODES:                                   # _acc: into a zeroed accumulator (a preloaded one: the test below)
            w2 = f"dg_diffaug_fwd_acc {H}x{W} {policy} {mode}"
            acc = Acc(L, mode)
            y, xs = Owned((B, 1, H, W)), acc.take(B)
            L.check(lib.dg_diffaug_fwd_acc(x.data_ptr(), *args, mask, B, H, W, xs.data_ptr(), y.ptr, None))
            n += U.assert_exact(y.done(w2), ref, w2)
            acc.done(w2)
            n += U.assert_exact(xs.cpu(), a.xsum if contrast else torch.zeros(B, dtype=torch.float64), w2 + " xsum")
        w3 = f"dg_diffaug_fwd_pre {H}x{W} {policy}"
        y, pre = Owned((B, 1, H, W)), dev(a.xsum)
        L.check(lib.dg_diffaug_fwd_pre(x.data_ptr(), *args, mask, B, H, W, pre.data_ptr(), y.ptr, None))
        n += U.assert_exact(y.done(w3), ref, w3)
    U.line("diffaug_fwd", f"{H}x{W} {draws}, {B} draws", n)


@pytest.mark.parametrize("mode", MODES)
def test_diffaug_fwd_acc_adds_onto_a_preloaded_sum(L, mode):
    """the contrast pivot is read from the accumulator the call added into: a preloaded H W k shifts every mean by k, exactly"""
    lib = L.lib()
    H, W, policy = 8, 16, "default"
    a = U.aug(H, W, "all")
    B, x = a.B, dev(a.x)
    args, keep = rp_dev(a.rp)
    acc = Acc(L, mode)
    y, xs = Owned((B, 1, H, W)), acc.take(B, preload=float(H * W))
    L.check(lib.dg_diffaug_fwd_acc(x.data_ptr(), *args, L.policy_mask(U.POLICIES[policy]), B, H, W, xs.data_ptr(), y.ptr, None))
    got = y.done("preloaded")
    acc.done("preloaded")
    n = U.assert_exact(xs.cpu(), a.xsum + H * W, "preloaded xsum")
    # A(x) with the mean moved by 1: y = mean + cc (v - mean) -> y + (1 - cc) on the window's pixels
    cc = (1 + 0.5 * a.rp["u_c"] ** 2).view(-1, 1, 1, 1)
    win = U.window_mask(a.rp, policy, H, W)[:, None]
    n += U.assert_exact(got, a.y(policy) + (1 - cc) * win, "preloaded")
    U.line("diffaug_fwd_acc", f"preloaded {mode}", n)


# ---- e. DiffAugment + BlurVH in one launch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", [0, 8], ids=["sums", "partials"])
@pytest.mark.parametrize("nsets", [1, 2])
@pytest.mark.parametrize("ring", [1, 0], ids=["ring", "reflect"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,W,draws", U.FUSED, ids=ids(U.FUSED))
def test_diffaug_blur_fwd(L, H, W, draws, dtype, ring, nsets, parts):
    """against O.blur_vh(O.diff_augment(x)) in float64 - not against the unfused kernels, which share csrc/diffaug.h with it"""
    lib, code = L.lib(), L.dtype_code(dtype)
    assert parts in (0, L.XSUM_PARTS)
    srcs = [U.aug(H, W, draws, s) for s in range(nsets)]
    B = srcs[0].B
    sets, keep = [], []
    for s in srcs:
        x = dev(s.x)
        if parts:                                            # any integers that sum to the sample's sum
            p = torch.randint(-50, 51, (B, parts), generator=torch.Generator().manual_seed(B + parts)).double()
            p[:, -1] = s.xsum - p[:, :-1].sum(dim=1)
            sums = dev(p)
        else:
            sums = dev(s.xsum)
        args, kp = rp_dev(s.rp)
        q = L.DgAugSet()
        q.x, q.xsum, q.xsum_parts = x.data_ptr(), sums.data_ptr(), parts
        q.u_b, q.u_c, q.t_h, q.t_w, q.o_x, q.o_y = args
        sets.append(q)
        keep += [x, sums, kp]
    arr = (L.DgAugSet * nsets)(*sets)
    n = 0
    for policy in U.policies_for(H, W):
        what = f"dg_diffaug_blur_fwd {H}x{W} {dtype} ring={ring} nsets={nsets} parts={parts} {policy}"
        out = Owned((nsets * B, H, W, 2), dtype)
        L.check(lib.dg_diffaug_blur_fwd(arr, nsets, L.policy_mask(U.POLICIES[policy]), B, H, W, ring, out.ptr, code, None))
        n += compare(out.done(what), torch.cat([s.fused(policy, bool(ring)) for s in srcs]), what)
    U.line("diffaug_blur_fwd", f"{H}x{W} {dtype} ring={ring} nsets={nsets} parts={parts}", n)


# ---- f. the way back ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,draws", U.AUG, ids=ids(U.AUG))
def test_diffaug_bwd(L, H, W, draws):
    lib = L.lib()
    a = U.aug(H, W, draws)
    B, e = a.B, dev(a.e)
    args, keep = rp_dev(a.rp)
    n = 0
    for policy in U.policies_for(H, W):
        mask, contrast = L.policy_mask(U.POLICIES[policy]), "contrast" in U.POLICIES[policy]
        ref, rsum = a.gx(policy), a.gsum(policy)
        what = f"dg_diffaug_bwd {H}x{W} {policy}"
        gx, gsum = Owned((B, 1, H, W)), Owned((B,))
        L.check(lib.dg_diffaug_bwd(e.data_ptr(), *args, mask, B, H, W, gsum.ptr, gx.ptr, None))
        n += U.assert_exact(gx.done(what), ref, what)
        got = gsum.done(what + " gsum", written=contrast)
        if contrast:
            n += U.assert_exact(got, rsum, what + " gsum")
        for mode in MODES:
            w2 = f"dg_diffaug_bwd_acc {H}x{W} {policy} {mode}"
            acc = Acc(L, mode)
            gx, gs = Owned((B, 1, H, W)), acc.take(B)
            L.check(lib.dg_diffaug_bwd_acc(e.data_ptr(), *args, mask, B, H, W, gs.data_ptr(), gx.ptr, None))
            n += U.assert_exact(gx.done(w2), ref, w2)
            acc.done(w2)
            n += U.assert_exact(gs.cpu(), rsum if contrast else torch.zeros(B, dtype=torch.float64), w2 + " gsum")
        w3 = f"dg_diffaug_bwd_pre {H}x{W} {policy}"
        gx, pre = Owned((B, 1, H, W)), dev(rsum)
        L.check(lib.dg_diffaug_bwd_pre(e.data_ptr(), *args, mask, B, H, W, pre.data_ptr(), gx.ptr, None))
        n += U.assert_exact(gx.done(w3), ref, w3)
    U.line("diffaug_bwd", f"{H}x{W} {draws}, {B} draws", n)


def _head(L, a, policy, gy, gsum, arch, cp, B, mask01, with_dbias):
    """dg_head_post_bwd_aug on the first B samples with the saved tanh plane zero (1 - t^2 == 1), logits and noise zero, tau 1,
    drop_const -1 -> (draw [B,1+arch,H,W], pm [B,H,W,cp], dbias [3] or None)"""
    lib = L.lib()
    H, W = a.H, a.W
    args, keep = rp_dev({k: v[:B] for k, v in a.rp.items()})
    gout = torch.zeros(B, 1 + arch, H, W, device=DEV)
    npx, nim = torch.zeros(B, 1, H, W, device=DEV), torch.zeros(B, device=DEV)
    mk = dev(mask01[:B]) if arch else None
    gyd, gsd = dev(gy[:B]), dev(gsum[:B])
    draw, pm = Owned((B, 1 + arch, H, W)), Owned((B, H, W, cp), BF16)
    db = Owned((3,), fill=0.0) if with_dbias else None
    L.check(lib.dg_head_post_bwd_aug(gout.data_ptr(), npx.data_ptr(), nim.data_ptr(), L.ptr(mk), gyd.data_ptr(), *args,
                                     L.policy_mask(U.POLICIES[policy]), gsd.data_ptr(), arch, 1.0, -1.0, B, H, W, U.S_DEPTH, 0.5,
                                     draw.ptr, db.ptr if db else None, pm.ptr, cp, None, None))
    what = f"dg_head_post_bwd_aug {H}x{W} {policy} arch={arch} cp={cp} B={B}"
    return draw.done(what), pm.done(what), (db.done(what) if db else None), what


def _head_checks(draw, pm, ref_depth, arch, cp, what):
    """channel 0 of the planar copy and of the pixel-major copy; the pixel-major copy's padded channels are zero"""
    n = U.assert_exact(draw[:, :1], ref_depth, what + " draw")
    n += U.assert_rne(pm[..., 0].unsqueeze(1).contiguous(), ref_depth, what + " pixel-major")
    pad = pm[..., 1 + arch:].float()
    assert not bool(pad.any()), what + ": padded channels of the pixel-major copy are not zero"
    return n + pad.numel()


@pytest.mark.parametrize("cp", [2, 4])
@pytest.mark.parametrize("arch", [0, 1])
@pytest.mark.parametrize("H,W,draws", U.HEAD, ids=ids(U.HEAD))
def test_head_post_bwd_aug(L, H, W, draws, arch, cp):
    a = U.aug(H, W, draws)
    mask01 = torch.randint(0, 2, (a.B, 1, H, W), generator=torch.Generator().manual_seed(H + W)).double()
    n = 0
    for policy in U.policies_for(H, W):
        gx = a.gx(policy)
        ref = U.S_DEPTH * gx * (mask01 if arch else 1.0)
        draw, pm, _, what = _head(L, a, policy, a.e, a.gsum(policy), arch, cp, a.B, mask01, False)
        n += _head_checks(draw, pm, ref, arch, cp, what)
        nb = U.dbias_samples(a, policy)                       # the bias gradient: over samples whose total is exact in any order
        if arch == 0 and nb:
            draw, pm, db, what = _head(L, a, policy, a.e, a.gsum(policy), 0, cp, nb, mask01, True)
            n += _head_checks(draw, pm, ref[:nb], 0, cp, what)
            n += U.assert_exact(db[:1], gx[:nb].sum().view(1), what + " dbias")
            assert not bool(db[1:].any()), what
    U.line("head_post_bwd_aug", f"{H}x{W} arch={arch} cp={cp}", n)


@pytest.mark.parametrize("H,W,draws", U.HEAD, ids=ids(U.HEAD))
def test_chain_blur_adjoint_into_the_head(L, H, W, draws):
    """bf16 d -> dg_blur_bwd_augsum -> dg_head_post_bwd_aug against A^T(BlurVH^T(d)) in float64"""
    lib = L.lib()
    a = U.aug(H, W, draws)
    B = a.B
    k = U.blur(H, W, B)
    d = dev(k.d, BF16)
    args, keep = rp_dev(a.rp)
    n = 0
    for policy in U.policies_for(H, W):
        what = f"chain {H}x{W} {policy}"
        dx, gsum = Owned((B, 1, H, W)), Owned((B,), fill=0.0)
        L.check(lib.dg_blur_bwd_augsum(d.data_ptr(), L.DG_BF16, dx.ptr, args[2], args[4], args[5], L.policy_mask(U.POLICIES[policy]),
                                       gsum.ptr, B, H, W, 1, None))
        gy, gs = dx.done(what), gsum.done(what)
        n += U.assert_exact(gy, k.adj(True), what + " dx") + U.assert_exact(gs, a.gsum(policy, "chain"), what + " gsum")
        draw, pm, _, w2 = _head(L, a, policy, gy.double(), gs.double(), 0, 2, B, None, False)
        n += _head_checks(draw, pm, U.S_DEPTH * a.gx(policy, "chain"), 0, 2, what + " " + w2)
    U.line("chain", f"{H}x{W} {draws}", n)


# ---- g. per-sample sums ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sq", [0, 1])
@pytest.mark.parametrize("n", U.SUM_N)
def test_sample_sum(L, n, sq):
    lib = L.lib()
    x = U.sum_rows(n)
    B, xd = x.shape[0], dev(x)
    ref = (x * x if sq else x).sum(dim=1)
    what = f"dg_sample_sum n={n} sq={sq}"
    out = Owned((B,))
    L.check(lib.dg_sample_sum(xd.data_ptr(), B, n, sq, out.ptr, None))
    cnt = U.assert_exact(out.done(what), ref, what)
    for mode in MODES:
        acc = Acc(L, mode)
        o = acc.take(B, preload=5.0)
        L.check(lib.dg_sample_sum_acc(xd.data_ptr(), B, n, sq, o.data_ptr(), None))
        acc.done(what)
        cnt += U.assert_exact(o.cpu(), ref + 5.0, what + " _acc " + mode)
    U.line("sample_sum", what, cnt)
