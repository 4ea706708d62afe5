"""What tests/test_gpu_net_end.py leans on, shown without a GPU:
 (a) the float64 restatements of tests/net_end_ref.py equal autograd in float64 through the oracle (maskout, gumbel_sigmoid,
     gan_loss), the double backward for head_post_bwd2, and autograd of the reference's path-length lines for pl_penalty;
 (b) the same arithmetic in float32, on the very inputs the GPU test uses, stays inside the criteria - and the inputs keep their
     promises: no pixel excluded from the mask comparison, everything normal or zero, the exact tiers exact;
 (c) every wrong variant of the list falls outside them, at every shape of the list where it can occur."""
import numpy as np
import pytest
import torch

from oracle import dusty_oracle as O
from tests import net_end_ref as N

F = np.float32
T = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
ARCH = {0: "none", 1: "dusty1", 2: "dusty2"}


def small_inputs(arch, seed=3):
    return N.head_inputs("random", arch, 2, 40, seed=seed)


def oracle_depth(h, inp, arch, training=True):
    """O.maskout on float64 head outputs h [B,1+arch,HW] (h[:, 0] is the raw depth)"""
    out = {"depth": torch.tanh(h[:, :1]), "confidence": h[:, 1:]}
    noise = {"pixel": T(inp.npx)[:, None], "image": T(inp.nim)[:, None, None]}
    return O.maskout(out, ARCH[arch], noise, inp.tau, inp.c, training)


def heads64(inp, arch):
    return torch.stack([T(inp.raw), T(inp.h1), T(inp.h2)][:1 + arch], dim=1).requires_grad_(True)


def z64(inp):
    return (N.f64(inp.h1) + N.f64(inp.npx)) / inp.tau, (N.f64(inp.h2) + N.f64(inp.nim)[:, None]) / inp.tau


# ---- (a) the restatements equal autograd ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("arch", [0, 1, 2])
def test_a_head_fwd_equals_oracle(arch, training):
    inp = small_inputs(arch)
    out = oracle_depth(heads64(inp, arch), inp, arch, bool(training))
    depth = (out["depth"] if arch else torch.tanh(T(inp.raw))[:, None]).detach().numpy()[:, 0]
    r = N.head_fwd_ref(inp.raw, N.f64(inp.h1) + N.f64(inp.npx), N.f64(inp.h2) + N.f64(inp.nim)[:, None], inp.h2, arch, training, inp.c)
    assert np.abs(N.depth_of(r.t, r.m, inp.c) - depth).max() <= 1e-15          # (two libraries' tanh)
    if arch:
        mk = out["mask"].detach().numpy()
        assert np.array_equal(mk[:, 0], r.mp) and (arch == 1 or np.array_equal(mk[:, 1], r.mi))


@pytest.mark.parametrize("arch", [0, 1, 2])
def test_a_head_bwd_and_bwd2_equal_autograd(arch):
    inp = small_inputs(arch)
    h = heads64(inp, arch)
    depth = oracle_depth(h, inp, arch)["depth"] if arch else torch.tanh(h[:, :1])
    go, th = T(inp.go)[:, None], T(inp.th)
    (g,) = torch.autograd.grad(depth, h, go, create_graph=True)
    (g2,) = torch.autograd.grad(g, h, th)                      # the tangent of the backward along th (the Hessian is symmetric)
    z1, z2 = z64(inp)
    t = np.tanh(N.f64(inp.raw))
    mp, mi = (z1 > 0).astype(float), (z2 > 0).astype(float)
    r = N.head_bwd_ref(t, inp.go, z1, z2, mp, mi, 1.0 / inp.tau, inp.c, arch)
    r2 = N.head_bwd2_ref(t, inp.go, inp.th, z1, z2, mp, mi, 1.0 / inp.tau, inp.c, arch)
    for ch in range(1 + arch):
        for got, want in ((r.d[ch], g[:, ch]), (r2.d[ch], g2[:, ch])):
            want = want.detach().numpy()
            assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), (arch, ch)


@pytest.mark.parametrize("mode_g", [0, 1])
@pytest.mark.parametrize("metric", N.METRICS)
def test_a_gan_ref_equals_autograd(metric, mode_g):
    for B, kind, smoothing in ((37, "normal", 0.9), (5, "saturated", 1.0), (8, "equal", 0.5)):
        if kind == "saturated":
            B = 12
        smoothing = N.w32(smoothing)                            # (the float the ABI receives)
        yr, yf = N.gan_random_logits(B, kind)
        a, b = T(yr).requires_grad_(True), T(yf).requires_grad_(True)
        loss = O.gan_loss(metric, a, b, "G" if mode_g else "D", smoothing)
        gr, gf = torch.autograd.grad(loss, [a, b], allow_unused=True)
        r = N.gan_ref(metric, mode_g, yr, yf, 0.5, smoothing)
        # (torch's softplus returns x above 20 in float64 too: the saturated logits differ from log1p(exp x) by up to e^-20 there)
        tol = 2.1e-9 if kind == "saturated" and metric in ("nsgan", "ragan") else 1e-15
        assert abs(float(loss.detach()) - r.loss) <= max(tol, 1e-13 * abs(float(loss.detach())))
        want = gf if mode_g else torch.cat([gr, gf])
        assert np.abs(r.dy - 0.5 * want.numpy()).max() <= tol, (metric, mode_g, kind)
        if not mode_g:
            assert np.array_equal(r.up[:B], np.ones(B)) and np.array_equal(r.up[B:], r.dy[B:])
            assert np.array_equal(r.rs[B:], np.ones(B)) and np.array_equal(r.rs[:B], r.dy[:B])
            assert abs(r.sum_dy - r.dy.sum()) <= 1e-15


@pytest.mark.parametrize("B,K", [(1, 1), (3, 63), (5, 65), (4, 512)])
def test_a_pl_ref_equals_autograd(B, K):
    """trainers/dcgan_amp.py:294-300 of the reference, in float64: lengths, lerp(.., 0.01) with the live mean, the penalty"""
    dz64 = N.f64(N.pl_inputs(B, K))
    if B >= 3:
        dz64[1] = 1e-3                                          # (autograd's sqrt has no derivative at a zero sample)
    dz = torch.tensor(dz64, requires_grad=True)
    ema = torch.tensor(0.3, dtype=torch.float64)
    lens = torch.sqrt(dz.pow(2).sum(dim=-1))
    pl_ema = ema.lerp(lens.mean(), N.C01)
    pen = (lens - pl_ema).pow(2).mean()
    (g,) = torch.autograd.grad(pen, dz)
    r = N.pl_ref(dz64, 2.0, 0.3)
    assert abs(float(pl_ema.detach()) - r.a) <= 1e-15 * max(1.0, r.a) and abs(float(pen.detach()) - r.pen) <= 1e-15 * max(1.0, r.pen)
    assert np.abs(r.v - 2.0 * g.numpy()).max() <= 1e-14 * max(1.0, np.abs(r.v).max())


# ---- (b) float32 restatements on the GPU test's inputs stay inside; the inputs keep their promises ------------------------------------
def test_b_tanh_sweep_inside_and_monotone():
    x = N.tanh_sweep()
    assert x.size == 16384 and np.float32(0.25) in x
    for k in range(1, 5):
        assert np.float32(0.25) - k * np.float32(2.0 ** -26) in x and np.float32(0.25) + k * np.float32(2.0 ** -25) in x
    got = N.dg_tanh32(x)
    q = N.check("dg_tanh32 sweep", got, np.tanh(N.f64(x)), N.tanh_bound(x))
    assert q < 1.0
    pos = x[:8192]
    assert np.all(np.diff(pos) > 0)
    seam = np.abs(N.f64(pos) - 0.25) <= 2.0 ** -22
    assert seam.sum() == 9 and np.all(np.diff(got[:8192][seam]) >= 0), "not monotone across the seam"
    N.assert_normal([x, x * x, N.f64(x) ** 3], "tanh sweep")


@pytest.mark.parametrize("tier", N.TIERS + ("sat",))
@pytest.mark.parametrize("arch", [0, 1, 2])
@pytest.mark.parametrize("HW", N.HEAD_FWD_HW)
def test_b_head_fwd_inputs(HW, arch, tier):
    inp = N.head_inputs(tier, arch, 3, HW)
    assert N.excluded_pixels(inp) == 0
    N.assert_normal(N.head_intermediates(inp), f"{tier} {arch} {HW}")
    l1, z1, l2, z2, it = N.head_formed(inp)
    for training in (1, 0):
        r = N.head_fwd_case(inp, training)
        if arch:                                               # the float32 sigmoid decides every mask as the reference does
            one = F(1.0)
            assert np.array_equal((one / (one + np.exp(-z1)) > F(0.5)).astype(float), r.mp)
            if arch == 2 and training:
                assert np.array_equal((one / (one + np.exp(-z2)) > F(0.5)).astype(float), r.mi)
        t32 = N.dg_tanh32(inp.raw)
        assert N.check("t", t32, r.t, r.bt) < 1.0
        big = np.abs(inp.raw) >= 9
        assert np.array_equal(np.abs(t32[big]), np.ones(int(big.sum()), dtype=F))
    if tier != "random":
        assert (l1 == 0).any() or arch == 0
        assert np.array_equal(N.f64(l1), N.f64(inp.h1) + N.f64(inp.npx)), "l1 is not exact on the grid"
        assert np.array_equal(N.f64(l2), N.f64(inp.h2) + N.f64(inp.nim)[:, None])
    if tier == "sat":                                          # every depth is -1, 0, 1 or c: sums of multiples of 1/2 below 2^24
        t32 = N.dg_tanh32(inp.raw)
        assert set(np.unique(np.abs(t32))) <= {0.0, 1.0}
        assert N.exact_sum_ok(N.depth_of(t32, N.head_fwd_case(inp, 1).m, inp.c), axis=1)


@pytest.mark.parametrize("case", N.HEAD_BWD, ids=N.case_id)
def test_b_head_bwd_f32_inside(case):
    inp = N.head_case_inputs(case)
    tier, arch, B, HW = case
    assert N.excluded_pixels(inp) == 0
    N.assert_normal(N.head_intermediates(inp), N.case_id(case))
    _, z1, _, z2, it = N.head_formed(inp)
    r = N.head_bwd_case(inp)
    got = N.head_bwd32(inp.t, inp.go, z1, z2, inp.mp, inp.mi, it, inp.c, arch)
    adds, _ = N.head_bwd_adds(B, HW, HW % 4 == 0)
    for ch in range(1 + arch):
        assert N.check(f"d{ch}", got[ch], r.d[ch], r.b[ch]) < 1.0
        bsum = r.b[ch].sum() + N.sum_bound(adds, np.abs(r.d[ch]).sum()) + 2.0 ** -33 * B * 8
        assert abs(float(got[ch].sum(dtype=F)) - r.d[ch].sum()) <= bsum
    if tier == "grid":                                         # arch 0 (and every d0): exact, also after the power-of-two scale
        assert np.array_equal(N.f64(got[0]), r.d[0]) and np.array_equal(N.f64(F(N.S_DEPTH) * got[0]), N.S_DEPTH * r.d[0])


@pytest.mark.parametrize("case", N.HEAD_BWD2, ids=N.case_id)
def test_b_head_bwd2_f32_inside(case):
    inp = N.head_case_inputs(case)
    tier, arch, B, HW = case
    assert N.excluded_pixels(inp) == 0
    N.assert_normal(N.head_intermediates(inp), N.case_id(case))
    _, z1, _, z2, it = N.head_formed(inp)
    r = N.head_bwd2_case(inp)
    got = N.head_bwd2_32(inp.t, inp.go, inp.th, z1, z2, inp.mp, inp.mi, it, inp.c, arch)
    for ch in range(1 + arch):
        assert N.check(f"row {ch}", got[ch], r.d[ch], r.b[ch]) < 1.0


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_b_final_conv_data_is_exact(dt):
    for n in N.FINAL_N[dt]:
        for B in N.FINAL_B:
            k = N.final_inputs(B, n)
            if dt == "bf16":
                assert np.array_equal(N.bf16_value(N.bf16_rne_bits(k.d4)), k.d4)
            assert N.exact_sum_ok(N.f64(k.d4) * N.f64(k.wf)[None], axis=1)             # y
            assert N.exact_sum_ok(N.f64(k.coef)[:, None] * N.f64(k.d4), axis=0)        # dwf
            y = N.final_fwd_ref(k.d4, k.wf, k.bias, N.FINAL_SCALE, k.y0)
            assert np.array_equal(N.f64(y.astype(F)), y)
            o = N.wsum_ref(k.d4, k.coef, N.FINAL_SCALE, k.out0)
            assert np.array_equal(N.f64(o.astype(F)), o)
            uw = N.f64(k.up)[:, None] * (N.f64(k.wf) * N.FINAL_SCALE)[None]
            assert np.array_equal(N.f64(uw.astype(F)), uw), "u w is not exact"
            N.assert_normal([uw, N.final_dd4_ref(k.d4, k.wf, k.up, N.FINAL_SCALE)])


@pytest.mark.parametrize("metric", N.EXACT_METRICS)
def test_b_gan_exact_tier_is_exact(metric):
    """float32 in thread order (a serial sum) returns the float64 reference bit for bit; so does any other order: every sum is of
    multiples of 2^-9 far below 2^24 units"""
    cases = [(B, False, 0.5, s) for B in (1, 64, 256) for s in (1.0, 0.5)] + [(B, True, B / 64.0, 1.0) for B in (33, 65, 128)]
    for B, small, w_gan, smoothing in cases:
        yr, yf = N.gan_exact_logits(B, small)
        assert abs(float(N.f64(yr).mean()) - (0.5 if B > 1 else 0.0)) == 0 and N.exact_sum_ok(yr[None], 1) and N.exact_sum_ok(yf[None], 1)
        for mode_g in (0, 1):
            r = N.gan_ref(metric, mode_g, yr, yf, w_gan, smoothing)
            g = N.gan_ref(metric, mode_g, yr, yf, w_gan, smoothing, dtype=F)
            exact_scalar = B in (1, 64, 128, 256)               # the loss divides by B
            for k in ("dy", "up", "rs", "mr", "mf") + (("loss", "sum_dy") if exact_scalar else ()):
                if k in r:
                    assert np.array_equal(N.f64(g[k]), N.f64(r[k])), (metric, B, mode_g, k)
                    assert np.array_equal(N.f64(np.asarray(r[k]).astype(F)), N.f64(r[k])), (metric, B, mode_g, k)
            assert N.exact_sum_ok(np.asarray(r.dy)[None] * 8.0, 1)
    if metric in ("hinge", "rahinge"):                         # the planted arguments sit exactly on the kink: value and derivative 0
        yr, yf = N.gan_exact_logits(64)
        off = (float(N.f64(yf).mean()), float(N.f64(yr).mean())) if metric == "rahinge" else (0.0, 0.0)
        j = 0 if metric == "rahinge" else 1
        assert 1.0 - (float(yr[j]) - off[0]) == 0.0 and 1.0 + (float(yf[j]) - off[1]) == 0.0
        if metric == "rahinge":
            assert 1.0 + (float(yr[2]) - off[0]) == 0.0 and 1.0 - (float(yf[2]) - off[1]) == 0.0


@pytest.mark.parametrize("metric", N.EXACT_METRICS)
def test_b_final_gan_bwd_data_is_exact(metric):
    """dg_final_gan_bwd's exact cases: dy is dyadic, so u w and every partial sum of dwf's terms dy[b] d4[b][i] are exact"""
    for mode_g, B in ((0, 33), (0, 128), (1, 65)):
        yr, yf = N.gan_exact_logits(B, small=True)
        r = N.gan_ref(metric, mode_g, yr, yf, B / 64.0)
        ns = B if mode_g else 2 * B
        for n in (512 * 2 + 8, 256 * 2 + 4):
            k = N.final_inputs(ns, n, seed=5)
            assert N.exact_sum_ok(N.f64(r.dy)[:, None] * N.f64(k.d4), axis=0)
            o = N.wsum_ref(k.d4, r.dy, N.FINAL_SCALE, k.out0)
            assert np.array_equal(N.f64(o.astype(F)), o)
            for u_ in ([r.dy] if mode_g else [r.dy, r.up]):
                uw = N.f64(u_)[:, None] * (N.f64(k.wf) * N.FINAL_SCALE)[None]
                assert np.array_equal(N.f64(uw.astype(F)), uw)


@pytest.mark.parametrize("metric", N.METRICS)
def test_b_gan_f32_inside(metric):
    kinds = ["normal", "equal"] if metric not in ("nsgan", "ragan") else ["normal", "saturated", "equal"]
    if metric in ("nsgan", "wgan", "lsgan", "hinge"):
        kinds.remove("equal")
    for B in (37, 300):
        for kind in kinds:
            yr, yf = N.gan_random_logits(B, kind)
            for mode_g in (0, 1):
                r, b = N.gan_ref(metric, mode_g, yr, yf, 0.5, 0.9), N.gan_bounds(metric, mode_g, yr, yf, 0.5, 0.9)
                g = N.gan_ref(metric, mode_g, yr, yf, 0.5, 0.9, dtype=F)
                for k in b:
                    assert N.check(f"{metric} {B} {kind} G={mode_g} {k}", np.atleast_1d(g[k]), np.atleast_1d(r[k]), np.atleast_1d(b[k])) < 1.0


@pytest.mark.parametrize("K", N.PL_K)
@pytest.mark.parametrize("B", N.PL_B)
def test_b_pl_f32_inside(B, K):
    dz = N.pl_inputs(B, K)
    for ema in (0.0, 0.7):
        r, b, g = N.pl_ref(dz, 2.0, ema), N.pl_bounds(dz, 2.0, ema), N.pl_ref(dz, 2.0, ema, dtype=F)
        for k in ("a", "pen", "v", "len"):
            assert N.check(f"pl {B} {K} {k}", np.atleast_1d(g[k]), np.atleast_1d(r[k]), np.atleast_1d(b[k])) < 1.0
        assert not np.isnan(g.v).any() and (B < 3 or not g.v[1].any())
        N.assert_normal([dz, r.len, r.v, r.dl])
    # equal lengths with ema at their common value: everything exact
    dz = np.full((B, 1), 0.75, dtype=F) * np.where(np.arange(B) % 2, -1, 1)[:, None].astype(F)
    g = N.pl_ref(dz, 2.0, 0.75, dtype=F)
    assert float(g.a) == 0.75 and float(g.pen) == 0.0 and not g.v.any()


def test_b_mean_and_scale_inputs():
    for n in (1, 255, 256, 257):
        x = N.mean_inputs(n)
        assert N.exact_sum_ok(x[None], 1) and float(N.f64(x).sum()) % n == 0


# ---- (c) the wrong variants fall outside ------------------------------------------------------------------------------------------
def rejected(what, got, want, bound):
    q, rep = N.check(what, got, want, bound, fail=False)
    return q > 1.0 and bool(rep)


@pytest.mark.parametrize("case", [c for c in N.HEAD_BWD if c[2] == 3], ids=N.case_id)
def test_c_head_bwd_variants(case):
    tier, arch, B, HW = case
    inp = N.head_case_inputs(case)
    r = N.head_bwd_case(inp)
    planar = np.stack([(d * s).astype(F) for d, s in zip(r.d[:1 + arch], (N.S_DEPTH, N.S_CONF, N.S_CONF))], axis=1)
    for cp in (2, 4):
        pm = np.zeros((B, HW, cp), dtype=np.uint16)
        for ch in range(min(1 + arch, cp)):
            pm[:, :, ch] = N.bf16_rne_bits(planar[:, ch])
        assert N.pm_problems(pm, planar, 1 + arch) == []
        assert N.pm_problems(np.roll(pm, 1, axis=1), planar, 1 + arch), "a copy shifted by one pixel passes"
        assert N.pm_problems(pm[:, :, ::-1].copy(), planar, 1 + arch), "swapped channels pass"
        trunc = pm.copy()
        trunc[:, :, 0] = planar[:, 0].view(np.uint32) >> 16
        assert tier == "grid" or N.pm_problems(trunc, planar, 1 + arch), "a truncated copy passes"
    # a quad's last pixel taken from the next sample
    for ch in range(1 + arch):
        mut = r.d[ch].copy()
        mut[:, 3::4] = np.roll(r.d[ch], -1, axis=0)[:, 3::4]
        assert rejected("quad", mut, r.d[ch], r.b[ch]), (case, ch)
    # dtanh from raw instead of from t
    assert rejected("dtanh", N.head_bwd_case(inp, "dtanh_raw").d[0], r.d[0], r.b[0])
    if arch == 2:
        assert rejected("si for sp", N.head_bwd_case(inp, "si_for_sp").d[1], r.d[1], r.b[1])


@pytest.mark.parametrize("case", [c for c in N.HEAD_BWD2 if c[1] >= 1 and c[3] < 1000], ids=N.case_id)
def test_c_head_bwd2_variants(case):
    tier, arch, B, HW = case
    inp = N.head_case_inputs(case)
    r = N.head_bwd2_case(inp)
    if arch == 2:
        m = N.head_bwd2_case(inp, "no_H12")
        assert rejected("H12", m.d[1], r.d[1], r.b[1]) and rejected("H12", m.d[2], r.d[2], r.b[2])
        # a term 1e-3 of its row still counts: wherever the H12 term is that much of the row (and neither sigmoid is saturated:
        # beyond |z| = 4 the fp32 1 - s cancels and the bound grows with it) dropping it misses by more than the bound
        _, z1, _, z2, _ = N.head_formed(inp)
        miss = np.abs(m.d[1] - r.d[1])
        big = (miss > 0) & (miss >= 1e-3 * np.abs(r.d[1])) & (np.abs(z1) <= 4) & (np.abs(z2) <= 4)
        assert big.any() and bool((miss[big] > r.b[1][big]).all())
    if inp.tau != 1.0:
        m = N.head_bwd2_case(inp, "sp2_tau")
        assert rejected("sp'' tau", m.d[1], r.d[1], r.b[1])


@pytest.mark.parametrize("arch", [1, 2])
@pytest.mark.parametrize("HW", N.HEAD_FWD_HW)
def test_c_head_fwd_variants(HW, arch):
    inp = N.head_inputs("grid", arch, 3, HW)
    r = N.head_fwd_case(inp, 1)
    ge = N.head_fwd_case(inp, 1, "ge")
    assert not np.array_equal(ge.mp, r.mp), "no pixel sits at l1 = 0"
    if arch == 2:
        assert not np.array_equal(ge.mi, r.mi)
        assert not np.array_equal(N.head_fwd_case(inp, 0, "eval_noisy").mi, N.head_fwd_case(inp, 0).mi)
    if HW % 1024:                                              # (the four-pixel form runs where HW % 1024 == 0)
        return
    # a quad's last pixel from the next sample, in the depth: value-for-value comparison sees it
    d = N.depth_of(N.dg_tanh32(inp.raw), r.m, inp.c)
    mut = d.copy()
    mut[:, 3::4] = np.roll(d, -1, axis=0)[:, 3::4]
    assert rejected("depth", mut, d, 0.0)


def test_c_tanh_variants():
    x = N.tanh_sweep()
    want, bound = np.tanh(N.f64(x)), N.tanh_bound(x)
    assert rejected("seam", N.dg_tanh32(x, seam=0.5), want, bound)
    assert rejected("horner", N.dg_tanh32(x, drop_last=True), want, bound)
    for tier in N.TIERS:                                       # ... and on a head case's own raw plane (768 pixels of 3 samples)
        raw = N.head_inputs(tier, 0, 3, 768).raw
        assert rejected("seam", N.dg_tanh32(raw, seam=0.5), np.tanh(N.f64(raw)), N.tanh_bound(raw)), tier


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_c_final_conv_variants(dt):
    V = 8 if dt == "bf16" else 4
    for n in N.FINAL_N[dt]:
        for C in N.FINAL_C:
            for B in (3, 256):
                k = N.final_inputs(B, n)
                g = N.final_dd4_ref(k.d4, k.wf, k.up, N.FINAL_SCALE)
                assert (k.d4 == 0).any() and not np.array_equal(N.final_dd4_ref(k.d4, k.wf, k.up, N.FINAL_SCALE, "ge"), g)
                db, bound = N.final_dbias_ref(g, k.rs, C, -(-B // 4) + 3 + -(-n // C))
                bad, _ = N.final_dbias_ref(g, k.rs, C, 0, "ie_div_C")
                if n > C:
                    assert rejected("dbias", bad, db, bound), (n, C, B)
                if B > 64:                                     # a sample of the second sweep skipped
                    rows = np.arange(B) != 64
                    assert not np.array_equal(N.wsum_ref(k.d4, k.coef, N.FINAL_SCALE, k.out0, rows), N.wsum_ref(k.d4, k.coef, N.FINAL_SCALE, k.out0))


@pytest.mark.parametrize("metric", ["ragan", "rahinge", "ralsgan"])
def test_c_gan_cross_term_swapped(metric):
    for B, exact in ((64, True), (37, False), (300, False)):
        if exact and metric == "ragan":
            continue
        yr, yf = N.gan_exact_logits(B) if exact else N.gan_random_logits(B)
        r = N.gan_ref(metric, 0, yr, yf, 0.5)
        b = N.gan_bounds(metric, 0, yr, yf, 0.5).dy if not exact else 0.0
        assert rejected("swap", N.gan_ref(metric, 0, yr, yf, 0.5, defect="cross_swap").dy, r.dy, b), (metric, B)


def test_c_lsgan_g_target_smoothed():
    for B, exact in ((64, True), (37, False)):
        yr, yf = N.gan_exact_logits(B) if exact else N.gan_random_logits(B)
        r = N.gan_ref("lsgan", 1, yr, yf, 0.5, 0.5)
        b = N.gan_bounds("lsgan", 1, yr, yf, 0.5, 0.5).dy if not exact else 0.0
        assert rejected("target", N.gan_ref("lsgan", 1, yr, yf, 0.5, 0.5, defect="lsgan_g_smoothed").dy, r.dy, b)


@pytest.mark.parametrize("K", N.PL_K)
@pytest.mark.parametrize("B", [3, 4, 5, 256])
def test_c_pl_variants(B, K):
    dz = N.pl_inputs(B, K)
    r, b = N.pl_ref(dz, 2.0, 0.7), N.pl_bounds(dz, 2.0, 0.7)
    assert rejected("mdev", N.pl_ref(dz, 2.0, 0.7, defect="no_mdev").v, r.v, b.v)
    if K != B:
        m = N.pl_ref(dz, 2.0, 0.7, defect="mean_over_K")
        assert rejected("over K", m.v, r.v, b.v) and abs(m.pen - r.pen) > b.pen
