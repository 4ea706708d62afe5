"""Every kernel that evaluates csrc/diffaug.h, per element, with the per-sample gate of DiffAugment(p < 1): the three forward forms,
the forward fused with BlurVH, the three adjoint forms, the BlurVH adjoint's window sum and the head backward's on-the-fly gather
(fixed tau and learnable tau), against the float64 restatement of tests/aug_gate_ref.py on image_exact_util's exact integer data.
A batch mixes all four gate states and neighbouring samples differ; fp32 outputs bit for bit, bf16 outputs the round-to-nearest-
even of the reference, every sum equal.  Guards and sentinels as in tests/test_gpu_image_exact.py."""
import pytest
import torch

from tests import aug_gate_ref as R
from tests import image_exact_util as U
from tests.gpu_guard_util import BF16, DEV, F32, MODES, Acc, Owned, dev
from tests.test_gpu_image_exact import compare, ids, rp_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from dusty_gan_amd import _lib
    _lib.lib()
    assert _lib.DG_AUG_OFF == R.OFF
    return _lib


@pytest.mark.parametrize("H,W,draws", R.GATE_AUG, ids=ids(R.GATE_AUG))
def test_the_data_keeps_every_value_exact(H, W, draws):
    a = R.gate_aug(H, W, draws)
    st = R.gate_state(a.rp)
    assert torch.bincount(st).tolist() == [a.B // 4] * 4 and bool((st[1:] != st[:-1]).all())
    R.assert_gate_inputs(H, W, draws)


@pytest.mark.parametrize("H,W,draws", R.GATE_AUG, ids=ids(R.GATE_AUG))
def test_diffaug_fwd_gated(L, H, W, draws):
    lib = L.lib()
    a = R.gate_aug(H, W, draws)
    B, x = a.B, dev(a.x)
    args, keep = rp_dev(a.rp)
    n = 0
    for policy in U.policies_for(H, W):
        mask, contrast = L.policy_mask(U.POLICIES[policy]), "contrast" in U.POLICIES[policy]
        ref = a.y(policy)
        what = f"dg_diffaug_fwd gated {H}x{W} {policy}"
        y, xsum = Owned((B, 1, H, W)), Owned((B,))
        L.check(lib.dg_diffaug_fwd(x.data_ptr(), *args, mask, B, H, W, xsum.ptr, y.ptr, None))
        n += U.assert_exact(y.done(what), ref, what)
        xsum.done(what + " xsum", written=contrast)
        for mode in MODES:
            w2 = f"dg_diffaug_fwd_acc gated {H}x{W} {policy} {mode}"
            acc = Acc(L, mode)
            y, xs = Owned((B, 1, H, W)), acc.take(B)
            L.check(lib.dg_diffaug_fwd_acc(x.data_ptr(), *args, mask, B, H, W, xs.data_ptr(), y.ptr, None))
            n += U.assert_exact(y.done(w2), ref, w2)
            acc.done(w2)
        w3 = f"dg_diffaug_fwd_pre gated {H}x{W} {policy}"
        y, pre = Owned((B, 1, H, W)), dev(a.xsum)
        L.check(lib.dg_diffaug_fwd_pre(x.data_ptr(), *args, mask, B, H, W, pre.data_ptr(), y.ptr, None))
        n += U.assert_exact(y.done(w3), ref, w3)
    U.line("diffaug_fwd gated", f"{H}x{W} {draws}, {B} samples", n)


@pytest.mark.parametrize("ring", [1, 0], ids=["ring", "reflect"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,W,draws", R.GATE_FUSED, ids=ids(R.GATE_FUSED))
def test_diffaug_blur_fwd_gated(L, H, W, draws, dtype, ring):
    """two source sets in one launch, the second with the batch reversed: a block's set, sample and gates all change together"""
    lib, code = L.lib(), L.dtype_code(dtype)
    srcs = [R.gate_aug(H, W, draws, s) for s in range(2)]
    B = srcs[0].B
    sets, keep = [], []
    for s in srcs:
        x, sums = dev(s.x), dev(s.xsum)
        args, kp = rp_dev(s.rp)
        q = L.DgAugSet()
        q.x, q.xsum, q.xsum_parts = x.data_ptr(), sums.data_ptr(), 0
        q.u_b, q.u_c, q.t_h, q.t_w, q.o_x, q.o_y = args
        sets.append(q)
        keep += [x, sums, kp]
    arr = (L.DgAugSet * 2)(*sets)
    n = 0
    for policy in U.policies_for(H, W):
        what = f"dg_diffaug_blur_fwd gated {H}x{W} {dtype} ring={ring} {policy}"
        for t in U._blur_partials(srcs[0].y(policy), bool(ring)):
            U._f32(t, what + " partial")
        out = Owned((2 * B, H, W, 2), dtype)
        L.check(lib.dg_diffaug_blur_fwd(arr, 2, L.policy_mask(U.POLICIES[policy]), B, H, W, ring, out.ptr, code, None))
        n += compare(out.done(what), torch.cat([s.fused(policy, bool(ring)) for s in srcs]), what)
    U.line("diffaug_blur_fwd gated", f"{H}x{W} {dtype} ring={ring}", n)


@pytest.mark.parametrize("H,W,draws", R.GATE_AUG, ids=ids(R.GATE_AUG))
def test_diffaug_bwd_gated(L, H, W, draws):
    lib = L.lib()
    a = R.gate_aug(H, W, draws)
    B, e = a.B, dev(a.e)
    args, keep = rp_dev(a.rp)
    n = 0
    for policy in U.policies_for(H, W):
        mask, contrast = L.policy_mask(U.POLICIES[policy]), "contrast" in U.POLICIES[policy]
        ref, rsum = a.gx(policy), a.gsum(policy)
        what = f"dg_diffaug_bwd gated {H}x{W} {policy}"
        gx, gsum = Owned((B, 1, H, W)), Owned((B,))
        L.check(lib.dg_diffaug_bwd(e.data_ptr(), *args, mask, B, H, W, gsum.ptr, gx.ptr, None))
        n += U.assert_exact(gx.done(what), ref, what)
        got = gsum.done(what + " gsum", written=contrast)
        if contrast:
            n += U.assert_exact(got, rsum, what + " gsum")
        for mode in MODES:
            w2 = f"dg_diffaug_bwd_acc gated {H}x{W} {policy} {mode}"
            acc = Acc(L, mode)
            gx, gs = Owned((B, 1, H, W)), acc.take(B)
            L.check(lib.dg_diffaug_bwd_acc(e.data_ptr(), *args, mask, B, H, W, gs.data_ptr(), gx.ptr, None))
            n += U.assert_exact(gx.done(w2), ref, w2)
            acc.done(w2)
            n += U.assert_exact(gs.cpu(), rsum if contrast else torch.zeros(B, dtype=torch.float64), w2 + " gsum")
        w3 = f"dg_diffaug_bwd_pre gated {H}x{W} {policy}"
        gx, pre = Owned((B, 1, H, W)), dev(rsum)
        L.check(lib.dg_diffaug_bwd_pre(e.data_ptr(), *args, mask, B, H, W, pre.data_ptr(), gx.ptr, None))
        n += U.assert_exact(gx.done(w3), ref, w3)
    U.line("diffaug_bwd gated", f"{H}x{W} {draws}, {B} samples", n)


@pytest.mark.parametrize("ring", [1, 0], ids=["ring", "reflect"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,W,draws", R.GATE_AUGSUM, ids=ids(R.GATE_AUGSUM))
def test_blur_bwd_augsum_gated(L, H, W, draws, dtype, ring):
    """the three-parameter window (t_h, o_x, o_y) sees both sentinels"""
    lib, code = L.lib(), L.dtype_code(dtype)
    a = R.gate_aug(H, W, draws)
    B = a.B
    k = U.blur(H, W, B)
    U._adj_partials_ok(k.d, "augsum gated")
    ref = k.adj(bool(ring))
    U._sum_ok(ref, "augsum gated window sum")
    d = dev(k.d, dtype)
    args, keep = rp_dev(a.rp)
    n = 0
    for policy in U.policies_for(H, W):
        for mode in MODES:
            what = f"dg_blur_bwd_augsum gated {H}x{W} {dtype} ring={ring} {policy} {mode}"
            acc = Acc(L, mode)
            dx, gsum = Owned((B, 1, H, W)), acc.take(B)
            L.check(lib.dg_blur_bwd_augsum(d.data_ptr(), code, dx.ptr, args[2], args[4], args[5], L.policy_mask(U.POLICIES[policy]),
                                           gsum.data_ptr(), B, H, W, ring, None))
            n += U.assert_exact(dx.done(what), ref, what)
            acc.done(what)
            n += U.assert_exact(gsum.cpu(), R.window_sum(ref, a.rp, U.POLICIES[policy]), what + " gsum")
    U.line("blur_bwd_augsum gated", f"{H}x{W} {dtype} ring={ring}", n)


def _head(L, a, policy, arch, cp, mask01, lt):
    """dg_head_post_bwd_aug (lt: its learnable-temperature form, weight 0 and 1 / tau_max = 1) with the saved planes zero, as
    tests/test_gpu_image_exact.py runs it -> (draw [B,1+arch,H,W], pm [B,H,W,cp], what)"""
    lib = L.lib()
    H, W, B = a.H, a.W, a.B
    args, keep = rp_dev(a.rp)
    gout = torch.zeros(B, 1 + arch, H, W, device=DEV)
    npx, nim = torch.zeros(B, 1, H, W, device=DEV), torch.zeros(B, device=DEV)
    mk = dev(mask01) if arch else None
    gyd, gsd = dev(a.e), dev(a.gsum(policy))
    draw, pm = Owned((B, 1 + arch, H, W)), Owned((B, H, W, cp), BF16)
    mask = L.policy_mask(U.POLICIES[policy])
    if lt:
        w, dt = torch.zeros(2, device=DEV), Owned((2,), fill=0.0)
        ws = torch.zeros(B * 1024, device=DEV)
        L.check(lib.dg_head_post_bwd_aug_lt(gout.data_ptr(), npx.data_ptr(), nim.data_ptr(), L.ptr(mk), gyd.data_ptr(), *args, mask,
                                            gsd.data_ptr(), arch, w.data_ptr(), 1.0, dt.ptr, -1.0, B, H, W, U.S_DEPTH, 0.5, draw.ptr,
                                            None, pm.ptr, cp, ws.data_ptr(), None))
    else:
        L.check(lib.dg_head_post_bwd_aug(gout.data_ptr(), npx.data_ptr(), nim.data_ptr(), L.ptr(mk), gyd.data_ptr(), *args, mask,
                                         gsd.data_ptr(), arch, 1.0, -1.0, B, H, W, U.S_DEPTH, 0.5, draw.ptr, None, pm.ptr, cp, None,
                                         None))
    what = f"dg_head_post_bwd_aug{'_lt' if lt else ''} gated {H}x{W} {policy} arch={arch} cp={cp}"
    return draw.done(what), pm.done(what), what


# (the learnable temperature belongs to the masked generators: arch >= 1)
@pytest.mark.parametrize("arch,cp,lt", [(0, 2, False), (1, 2, False), (1, 4, False), (1, 2, True), (1, 4, True)],
                         ids=["none-cp2-tau", "dusty-cp2-tau", "dusty-cp4-tau", "dusty-cp2-lt", "dusty-cp4-lt"])
@pytest.mark.parametrize("H,W,draws", R.GATE_HEAD, ids=ids(R.GATE_HEAD))
def test_head_post_bwd_aug_gated(L, H, W, draws, arch, cp, lt):
    a = R.gate_aug(H, W, draws)
    mask01 = torch.randint(0, 2, (a.B, 1, H, W), generator=torch.Generator().manual_seed(H + W)).double()
    n = 0
    for policy in U.policies_for(H, W):
        ref = U.S_DEPTH * a.gx(policy) * (mask01 if arch else 1.0)
        draw, pm, what = _head(L, a, policy, arch, cp, mask01, lt)
        n += U.assert_exact(draw[:, :1], ref, what + " draw")
        n += U.assert_rne(pm[..., 0].unsqueeze(1).contiguous(), ref, what + " pixel-major")
    U.line("head_post_bwd_aug gated", f"{H}x{W} arch={arch} cp={cp} lt={lt}", n)


def test_without_a_sentinel_the_gated_batch_is_the_ungated_one(L):
    """the same draws with every gate on: the bits of the ungated reference (image_exact_util.aug64 at the policy)"""
    lib = L.lib()
    H, W = 8, 16
    a = R.gate_aug(H, W, "all")
    on = R.gate_state(a.rp) == 3
    rp = {k: v[on] for k, v in a.rp.items()}
    x = a.x[on]
    B = x.shape[0]
    args, keep = rp_dev(rp)
    y, xsum = Owned((B, 1, H, W)), Owned((B,))
    L.check(lib.dg_diffaug_fwd(dev(x).data_ptr(), *args, L.policy_mask(U.POLICIES["default"]), B, H, W, xsum.ptr, y.ptr, None))
    U.assert_exact(y.done("all on"), U.aug64(x, rp, "default"), "all on")
