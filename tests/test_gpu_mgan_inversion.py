"""Multi-code GAN inversion (mGANprior) on the MI355X: dg_feat_compose / dg_feat_compose_bwd against float64, parity of
invert(num_code=4) with the reference's loop (tests/golden/mgan_inversion.npz) and with its bf16-emulating restatement
(tests/mgan_inv_util.py), one-hot consistency with the single-code path at full width, determinism and capture, batch
independence, isolation, and the evaluation command.

Figures measured on an MI355X are printed by every test before it asserts."""
import numpy as np
import pytest
import torch

from tests.golden_util import load
from tests.mgan_inv_util import CASES, IDS, fixture_case, oracle_invert_multi
from tests.test_gpu_inversion import BF16, cosine, make_G, rel_max

pytestmark = pytest.mark.gpu
DEV = "cuda"
SQRT2 = np.float32(1.4142135623730951)
F_POS, F_NEG = float(SQRT2), float(np.float32(0.2) * SQRT2)   # the two values of the EPI_MASK factor (csrc/common.h dg_epilogue)


# ------------------------------------------------------------------------------------------------ 1. the kernels
def compose_inputs(dtype, B, N, P, C, same_sign=False):
    gen = torch.Generator().manual_seed(B * 1000 + N * 100 + C)
    a = torch.randn(B * N, P, C, generator=gen)
    if same_sign:   # every code of a scan has the sign of code 0 at (p, c): the sum over codes does not cancel
        sgn = torch.sign(a.view(B, N, P, C)[:, :1]).expand(B, N, P, C).reshape(B * N, P, C)
        a = a.abs() * sgn
    a[torch.rand(B * N, P, C, generator=gen) < 0.05] = 0.0   # exact zeros: the slope's convention at zero
    g = torch.randn(B, P, C, generator=gen)
    alpha = torch.rand(B, N, C, generator=gen) * 0.5 + 0.05 if same_sign else torch.randn(B, N, C, generator=gen) * 0.5
    return a.to(dtype).to(DEV), g.to(dtype).to(DEV), alpha.to(DEV)


def run_compose(a, g, alpha, nchunk=None):
    from dusty_gan_amd import _lib as L
    lib = L.lib()
    B, N, C = alpha.shape
    P = a.shape[1]
    dt = L.dtype_code(a.dtype)
    out = torch.full_like(g, float("nan"))
    dpre = torch.full_like(a, float("nan"))
    dalpha = torch.full_like(alpha, float("nan"))
    es = a.element_size()
    nchunk = max(1, min(64, P, (P * C * es) // 65536)) if nchunk is None else nchunk
    parts = torch.zeros(B * N * nchunk * C, device=DEV)
    tickets = torch.zeros(B * N, dtype=torch.int32, device=DEV)
    L.check(lib.dg_feat_compose(L.ptr(a), L.ptr(alpha), L.ptr(out), dt, B, N, P, C, L.stream_ptr()), "dg_feat_compose")
    L.check(lib.dg_feat_compose_bwd(L.ptr(g), L.ptr(a), L.ptr(alpha), L.ptr(dpre), L.ptr(dalpha), L.ptr(parts), L.ptr(tickets),
                                    nchunk, dt, B, N, P, C, L.stream_ptr()), "dg_feat_compose_bwd")
    dalpha2 = torch.full_like(alpha, float("nan"))
    L.check(lib.dg_feat_compose_bwd(L.ptr(g), L.ptr(a), L.ptr(alpha), L.ptr(dpre), L.ptr(dalpha2), L.ptr(parts), L.ptr(tickets),
                                    nchunk, dt, B, N, P, C, L.stream_ptr()), "dg_feat_compose_bwd")
    assert int(tickets.abs().sum()) == 0 and float(parts.abs().sum()) == 0.0   # scratch left zero
    return out, dpre, dalpha, dalpha2, nchunk


def compose_reference(a, g, alpha):
    """float64, on the device, from the inputs as stored"""
    B, N, C = alpha.shape
    P = a.shape[1]
    a4, g4, al = a.double().view(B, N, P, C), g.double().view(B, 1, P, C), alpha.double().view(B, N, 1, C)
    terms = al * a4
    f = torch.where(a4 > 0, torch.full_like(a4, F_POS), torch.full_like(a4, F_NEG))
    dpre = g4 * al * f
    ga = g4 * a4
    return terms.sum(dim=1), float(terms.abs().max()), dpre.view(B * N, P, C), ga.sum(dim=2), float(ga.abs().max())


@pytest.mark.parametrize("B,N,P,C", [(2, 3, 40, 4), (1, 1, 8, 16), (1, 64, 256, 512)])
def test_compose_kernels_fp32(B, N, P, C):
    a, g, alpha = compose_inputs(torch.float32, B, N, P, C)
    out, dpre, dalpha, dalpha2, nchunk = run_compose(a, g, alpha)
    r_out, tmax, r_dpre, r_dalpha, gamax = compose_reference(a, g, alpha)
    e_out = float((out.double() - r_out).abs().max())
    e_dpre = float((dpre.double() - r_dpre).abs().max())
    e_da = float((dalpha.double() - r_dalpha).abs().max())
    u = 2.0 ** -23
    print(f"fp32 B{B} N{N} P{P} C{C} nchunk {nchunk}: out {e_out:.3g} (bound {N * u * tmax:.3g}), dpre {e_dpre:.3g} "
          f"(bound {N * u * float(r_dpre.abs().max()):.3g}), dalpha {e_da:.3g} (bound {P * u * gamax:.3g})")
    assert e_out <= N * u * tmax
    assert e_dpre <= N * u * float(r_dpre.abs().max())
    assert e_da <= P * u * gamax
    assert torch.equal(dalpha, dalpha2)
    if B == 2:   # several workgroups per (scan, code): the cross-workgroup sum on a shape whose chunks are ragged
        _, dpre3, dalpha3, dalpha4, _ = run_compose(a, g, alpha, nchunk=7)
        assert torch.equal(dalpha3, dalpha4) and torch.equal(dpre3, dpre)
        assert float((dalpha3.double() - r_dalpha).abs().max()) <= P * u * gamax


def bf16_ulp_report(got, ref64, what):
    """got (bf16) against ref64 rounded once to bf16: equal, or one bf16 ulp apart; returns the share of unequal elements"""
    want = ref64.float().to(torch.bfloat16)
    ne = got != want
    share = float(ne.float().mean())
    gi, wi = got.view(torch.int16).int(), want.view(torch.int16).int()
    far = ne & ((gi - wi).abs() > 1)
    print(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ from the once-rounded float64 value (share {share:.3g}), "
          f"{int(far.sum())} by more than one bf16 ulp")
    assert int(far.sum()) == 0, f"{what}: {int(far.sum())} elements off by more than one bf16 ulp (share unequal {share:.3g})"
    assert share < 1e-3, f"{what}: share of elements one ulp off {share:.3g}"
    return share


def test_compose_kernels_bf16_full_width_a3():
    B, N, P, C = 2, 5, 16384, 64
    a, g, alpha = compose_inputs(torch.bfloat16, B, N, P, C, same_sign=True)
    out, dpre, dalpha, dalpha2, nchunk = run_compose(a, g, alpha)
    assert nchunk > 1
    r_out, tmax, r_dpre, r_dalpha, gamax = compose_reference(a, g, alpha)
    bf16_ulp_report(out, r_out, "abar")
    bf16_ulp_report(dpre, r_dpre, "dpre")
    e_da = float((dalpha.double() - r_dalpha).abs().max())
    print(f"bf16 dalpha {e_da:.3g} (bound {P * 2.0 ** -23 * gamax:.3g}), nchunk {nchunk}")
    assert e_da <= P * 2.0 ** -23 * gamax
    assert torch.equal(dalpha, dalpha2)


def test_dpre_slope_convention_equals_epi_mask():
    """dg_feat_compose_bwd's leaky-relu factor against the conv kernels' EPI_MASK epilogue on the same aux, exact zeros and
    negative zeros included: one GEMM launch with EPI_LINEAR (= g) and one with EPI_MASK and aux = a; with alpha = 1 and N = 1
    dpre must be the masked launch's output - the same branch at every element, the same factor to fp32 rounding"""
    import math

    from dusty_gan_amd import _lib as L
    from dusty_gan_amd import engine as E
    R, K, C = 40, 8, 16
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(R, K, generator=gen).to(DEV)
    w = torch.randn(C, K, generator=gen).to(DEV)
    aux = torch.randn(R, C, generator=gen)
    aux[torch.rand(R, C, generator=gen) < 0.2] = 0.0
    aux[0, :4] = -0.0
    aux = aux.to(DEV)
    ops = E.Ops(torch.float32)
    lin, msk = torch.empty(R, C, device=DEV), torch.empty(R, C, device=DEV)
    s = 1.0 / math.sqrt(K)
    ops.conv(L.MODE_GEMM, 0, 1, R, 1, 1, K, C, x, (K, 0, 1), lin, (C, 0, 1), L.ptr(w), s, L.EPI_LINEAR)
    ops.conv(L.MODE_GEMM, 0, 1, R, 1, 1, K, C, x, (K, 0, 1), msk, (C, 0, 1), L.ptr(w), s, L.EPI_MASK, aux=aux)
    alpha = torch.ones(1, 1, C, device=DEV)
    _, dpre, _, _, _ = run_compose(aux.view(1, R, C).contiguous(), lin.view(1, R, C), alpha, nchunk=1)
    dpre = dpre.view(R, C)
    pos_conv, pos_mine = (msk / lin) > 1.0, (dpre / lin) > 1.0
    assert bool((lin != 0).all())
    assert torch.equal(pos_conv, pos_mine) and torch.equal(pos_conv, aux > 0)
    assert int((~pos_conv).sum()) > 0 and int(pos_conv.sum()) > 0 and int((aux == 0).sum()) > 4
    err = float(((dpre - msk).abs() / msk.abs()).max())
    print("dpre against the EPI_MASK launch: max relative difference", err)
    assert err <= 2.0 ** -22


# ------------------------------------------------------------------------------------------------ 2., 3. the fixture
def run_case(arch, distance, layer, dtype=torch.float32):
    from dusty_gan_amd.inversion import invert
    g = load("mgan_inversion")
    c = fixture_case(g, arch, distance, layer)
    G = make_G(arch, c["params"], dtype=dtype)
    steps = []
    noise = c["noise"][:, None]
    res = invert(G, c["inv_ref"].to(DEV), c["mask"].to(DEV), num_step=c["S"], distance=distance, latent=c["latent0"][None],
                 noise_fn=lambda k: noise[k], gumbel_noise=c["gumbel"], num_code=c["N"], composition_layer=c["name"],
                 on_step=lambda k, *t: steps.append(tuple(x.cpu() for x in t)))
    return g, c, steps, res


@pytest.mark.parametrize("arch,distance,layer", CASES, ids=IDS)
def test_fp32_matches_reference_fixture(arch, distance, layer):
    g, c, steps, res = run_case(arch, distance, layer)
    t = lambda k: torch.from_numpy(g[c["pre"] + k])
    loss0 = t("s0/loss")
    worst = dict(loss=float(((steps[0][0] - loss0).abs() / loss0.abs()).max()), grad=0.0, cos=1.0, dalpha=0.0, cos_a=1.0,
                 latent=0.0, alpha=0.0)
    for k, (loss, gz, lat, ga, al) in enumerate(steps):
        gr, ar = t(f"s{k}/grad"), t(f"s{k}/dalpha")
        for n in range(c["N"]):
            worst["grad"], worst["cos"] = max(worst["grad"], rel_max(gz[0, n], gr[n])), min(worst["cos"], cosine(gz[0, n], gr[n]))
            worst["dalpha"] = max(worst["dalpha"], rel_max(ga[0, n], ar[n]))
            worst["cos_a"] = min(worst["cos_a"], cosine(ga[0, n], ar[n]))
        worst["latent"] = max(worst["latent"], float((lat[0] - t(f"s{k}/latent")).abs().max()))
        worst["alpha"] = max(worst["alpha"], float((al[0] - t(f"s{k}/alpha")).abs().max()))
    print(c["pre"], "fp32 worst over the steps:", worst)
    assert worst["loss"] <= 1e-5
    assert worst["grad"] <= 1e-4 and worst["cos"] >= 0.99999
    assert worst["dalpha"] <= 1e-4 and worst["cos_a"] >= 0.99999
    assert worst["latent"] <= 1e-4
    assert worst["alpha"] <= 1e-6
    assert torch.equal(res["latent"].cpu(), steps[-1][2]) and torch.equal(res["alpha"].cpu(), steps[-1][4])
    assert torch.equal(res["loss"].cpu(), steps[-1][0])
    assert res["latent"].shape == (1, c["N"], 8) and res["alpha"].shape == steps[-1][3].shape


# bf16 against the bf16-emulating restatement (tests/mgan_inv_util.py: oracle.dusty_oracle's roundings plus the composite's and its
# gradient's).  The BF16 bounds of tests/test_gpu_inversion.py (loss 5e-4, gradient 0.15 of max, cosine 0.995, latent 4e-2) hold
# as they are, for d loss / d alpha as for d loss / d latent.  Measured on an MI355X, six cases x six steps, worst per quantity:
#   loss 2.4e-5 relative (dusty1 l2, layer 2); d loss/dz 8.4e-2 of max, cosine 0.99764 (dusty2 l1, layer 3);
#   d loss/dalpha 2.5e-2 of max, cosine 0.99968 (dusty1 l2, layer 2); latent 4.7e-3 (dusty2 l1, layer 3);
#   alpha 3.0e-5 (dusty1 l2, layer 2; 1.4e-6 or less in the other five cases); d loss/dz of the layer-0 and layer-1 cases is bit-equal
#   to the restatement's on every step.  (DESIGN.md 7b carries the same figures.)
# The alpha bound is 2.2 x the worst seen, the margin that file uses: 6.6e-5.  (An Adam step of alpha is about
# alpha_lr lr_schedule(k) sign(g), 1e-3 per step here: a single component stepped the wrong way would be 30 x the bound.)
BF16_ALPHA = 6.6e-5


@pytest.mark.parametrize("arch,distance,layer", CASES, ids=IDS)
def test_bf16_matches_emulating_oracle(arch, distance, layer):
    _, c, steps, _ = run_case(arch, distance, layer, dtype=torch.bfloat16)
    ref = oracle_invert_multi(c["params"], arch, c["gumbel"], c["inv_ref"], c["mask"], c["latent0"][None], c["noise"][:, None],
                              c["S"], distance, layer, dtype=torch.bfloat16)
    worst = dict(loss=0.0, grad=0.0, cos=1.0, dalpha=0.0, cos_a=1.0, latent=0.0, alpha=0.0)
    for k, ((loss, gz, lat, ga, al), (l_r, gz_r, ga_r, lat_r, al_r)) in enumerate(zip(steps, ref)):
        worst["loss"] = max(worst["loss"], float(((loss - l_r).abs() / l_r.abs()).max()))
        for n in range(c["N"]):
            worst["grad"] = max(worst["grad"], rel_max(gz[0, n], gz_r[0, n]))
            worst["cos"] = min(worst["cos"], cosine(gz[0, n], gz_r[0, n]))
            worst["dalpha"] = max(worst["dalpha"], rel_max(ga[0, n], ga_r[0, n]))
            worst["cos_a"] = min(worst["cos_a"], cosine(ga[0, n], ga_r[0, n]))
        worst["latent"] = max(worst["latent"], float((lat - lat_r).abs().max()))
        worst["alpha"] = max(worst["alpha"], float((al - al_r).abs().max()))
    print(c["pre"], "bf16 worst over the steps:", worst, "alpha bound", BF16_ALPHA)
    assert worst["loss"] <= BF16["loss"]
    assert worst["grad"] <= BF16["grad"] and worst["cos"] >= BF16["cos"]
    assert worst["dalpha"] <= BF16["grad"] and worst["cos_a"] >= BF16["cos"]
    assert worst["latent"] <= BF16["latent"]
    assert worst["alpha"] <= BF16_ALPHA


# ------------------------------------------------------------------------------------------------ 4. one-hot, full width
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("layer", [0, 3])
def test_one_hot_alpha_equals_single_code_full_width(layer, dtype, monkeypatch):
    """64x1024, nz 512, ch_base 64, dusty2, B = 2, N = 4: with alpha one-hot on code 0 the composite IS code 0's feature map, so
    step 0 has the single-code loss and gradient for code 0 and an exactly zero gradient for codes 1..3; d loss / d alpha
    equals sum_p g a_n recomputed from the engines' own buffers"""
    from dusty_gan_amd import inversion as I
    torch.manual_seed(0)
    G = make_G("dusty2", None, in_ch=512, ch_base=64, ch_max=512, shape=(64, 1024), dtype=dtype)
    B, N, nz = 2, 4, 512
    C = I.composition_layers(G)[f"backbone.{layer}"][0]
    gen = torch.Generator().manual_seed(11)
    lat = I.normalize_rows(torch.randn(B * N, nz, generator=gen)).view(B, N, nz)
    ref = torch.rand(B, 1, 64, 1024, generator=gen).to(DEV)
    mask = (torch.rand(B, 1, 64, 1024, generator=gen) > 0.1).float().to(DEV)
    gum = torch.zeros(1, 1, 64, 1024)
    alpha = torch.zeros(B, N, C)
    alpha[:, 0] = 1.0
    states = []
    orig = I.InvState.multi_code
    monkeypatch.setattr(I.InvState, "multi_code", lambda self, *a: (states.append(self), orig(self, *a))[1])
    multi, single, recomputed = [], [], []

    def on_multi(k, loss, gz, latent, ga, al):
        multi.append((loss.cpu(), gz.cpu(), ga.cpu()))
        if k == 0:
            S = states[0]
            P = S.lower.compose_geometry(layer)[0]
            g = G.backbone.engine().dp[layer].double().view(B, 1, P, C)
            a = S.lower.a[layer].double().view(B, N, P, C)
            ga64 = g * a
            recomputed.append((ga64.sum(dim=2).cpu(), float(ga64.abs().max()), P))
    I.invert(G, ref, mask, num_step=2, latent=lat, noise_fn=lambda k: torch.zeros(B, N, nz), gumbel_noise=gum, num_code=N,
             composition_layer=layer, alpha=alpha, on_step=on_multi)
    I.invert(G, ref, mask, num_step=2, latent=lat[:, 0], noise_fn=lambda k: torch.zeros(B, nz), gumbel_noise=gum,
             on_step=lambda k, loss, gz, latent: single.append((loss.cpu(), gz.cpu())))
    (l_m, gz_m, ga_m), (l_s, gz_s) = multi[0], single[0]
    e_loss = float(((l_m - l_s).abs() / l_s.abs()).max())
    e_g = max(rel_max(gz_m[b, 0], gz_s[b]) for b in range(B))
    cos = min(cosine(gz_m[b, 0], gz_s[b]) for b in range(B))
    want_da, gamax, P = recomputed[0]
    e_da = float((ga_m.double() - want_da).abs().max())
    print(f"one-hot layer {layer} {dtype}: loss {e_loss:.3g}, dlatent rel_max {e_g:.3g} cosine {cos:.6f}, "
          f"dalpha {e_da:.3g} (bound {P * 2.0 ** -23 * gamax:.3g})")
    assert int(torch.count_nonzero(gz_m[:, 1:])) == 0
    assert e_loss <= 1e-5
    if dtype == torch.float32:
        assert e_g <= 1e-4
    else:
        assert e_g <= BF16["grad"] and cos >= BF16["cos"]
    assert e_da <= P * 2.0 ** -23 * gamax


# ------------------------------------------------------------------------------------------------ 5. determinism and capture
def test_deterministic_and_graph_equals_eager():
    from dusty_gan_amd.inversion import invert
    from tests.test_gpu_chamfer_inversion import make_lidar
    g = load("mgan_inversion")
    c = fixture_case(g, "dusty2", "l1", 3)
    G = make_G("dusty2", c["params"])
    kw = dict(num_step=12, seed=5, gumbel_noise=c["gumbel"], distance=("l1", "chamfer"), lidar=make_lidar(), num_code=4,
              composition_layer="backbone.2")
    ref, mask = c["inv_ref"].to(DEV), c["mask"].to(DEV)
    a = invert(G, ref, mask, graph=True, **kw)
    b = invert(G, ref, mask, graph=True, **kw)
    e = invert(G, ref, mask, graph=False, **kw)
    for k in ("latent", "alpha", "loss", "inv_gen"):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], e[k]), k
    for k in a["out"]:
        assert torch.equal(a["out"][k], b["out"][k]) and torch.equal(a["out"][k], e["out"][k]), k
    assert not torch.equal(a["alpha"], torch.full_like(a["alpha"], 0.25))   # (alpha did move)


# ------------------------------------------------------------------------------------------------ 6. independence, isolation
def test_batch_independence():
    from dusty_gan_amd.inversion import invert
    g = load("mgan_inversion")
    c = fixture_case(g, "dusty1", "l2", 2)
    G = make_G("dusty1", c["params"])
    S, N = c["S"], 4
    gen = torch.Generator().manual_seed(9)
    lat = torch.randn(2, N, 8, generator=gen)
    nz = torch.randn(S, 2, N, 8, generator=gen) * 0.03
    ref2 = torch.cat([c["inv_ref"], c["inv_ref"].flip(3)]).to(DEV)
    m2 = torch.cat([c["mask"], c["mask"].flip(3)]).to(DEV)
    kw = dict(num_step=S, distance="l2", gumbel_noise=c["gumbel"], num_code=N, composition_layer=2)
    full = invert(G, ref2, m2, latent=lat, noise_fn=lambda k: nz[k], **kw)
    for i in range(2):
        one = invert(G, ref2[i:i + 1], m2[i:i + 1], latent=lat[i:i + 1], noise_fn=lambda k: nz[k, i:i + 1], **kw)
        assert float((one["latent"][0] - full["latent"][i]).abs().max()) <= 1e-5, i
        assert abs(float(one["loss"][0] - full["loss"][i])) <= 1e-5 * max(1.0, abs(float(full["loss"][i]))), i
        assert float((one["alpha"][0] - full["alpha"][i]).abs().max()) <= 1e-6, i


def test_num_code_one_is_the_single_code_path():
    from dusty_gan_amd.inversion import invert
    g = load("mgan_inversion")
    c = fixture_case(g, "dusty2", "l1", 1)
    G = make_G("dusty2", c["params"])
    ref, mask = c["inv_ref"].to(DEV), c["mask"].to(DEV)
    a = invert(G, ref, mask, num_step=8, seed=3, gumbel_noise=c["gumbel"])
    b = invert(G, ref, mask, num_step=8, seed=3, gumbel_noise=c["gumbel"], num_code=1)
    assert a.keys() == b.keys() and "alpha" not in a
    for k in ("latent", "loss", "inv_gen"):
        assert torch.equal(a[k], b[k]), k


def test_next_trainer_step_equals_a_twin_that_never_inverted(monkeypatch):
    """a multi-code inversion on a live trainer's G_ema between two of its replayed steps: the following steps equal, bit for
    bit, those of a twin that never inverted (tests/test_gpu_inversion.py, the same test of the single-code path)"""
    from dusty_gan_amd.inversion import invert
    from tests.test_gpu_step import make_trainer
    monkeypatch.setenv("DUSTY_GAN_GRAPH", "1")

    def make():
        torch.manual_seed(21)
        return make_trainer("dusty2", True, (32, 64), 8, 4, 16, 4)
    a, b = make(), make()
    for i in range(3):
        assert a.step(i) == b.step(i)
    inv = torch.rand(3, 1, 32, 64, device=DEV)
    invert(a.G_ema, inv, (inv > 0.2).float(), num_step=12, seed=4, graph=True, num_code=4, composition_layer="backbone.1")
    invert(a.G_ema, inv, (inv > 0.2).float(), num_step=3, seed=4, graph=False, num_code=2, composition_layer=3)
    for i in range(3, 6):
        sa, sb = a.step(i), b.step(i)
        assert sa == sb, (i, sa, sb)
    for net in ("G", "D", "G_ema"):
        fa = getattr(a, net).store.flat if not hasattr(getattr(a, net), "backbone") else getattr(a, net).backbone.store.flat
        fb = getattr(b, net).store.flat if not hasattr(getattr(b, net), "backbone") else getattr(b, net).backbone.store.flat
        assert torch.equal(fa, fb), net


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_evaluate_reconstruction_multi_code_end_to_end(tmp_path):
    """the evaluation command with --num-code 4 --composition-layer backbone.2 on a synthetic full-width dusty2 bf16 checkpoint
    and three .npy test scans (tests/test_gpu_inversion.py's recipe): one finite CSV row per scan, the reference's columns"""
    import csv

    from dusty_gan_amd import evaluate_reconstruction as E
    from dusty_gan_amd.models import define_G
    from dusty_gan_amd.utils.config import dump_config, load_config
    from tests.test_gpu_data import write_kitti_tree
    root = str(tmp_path / "kitti")
    write_kitti_tree(root, 64, 2048, {11: 3})
    cfg = load_config(["model=dusty2_dcgan_eqlr", "dataset=kitti_odometry", f"dataset.root={root}",
                       "dataset.shape=[64,1024]", "enable_amp=true"])
    cfg_path, ckpt = str(tmp_path / "config.yaml"), str(tmp_path / "model.pth")
    dump_config(cfg, cfg_path)
    torch.manual_seed(0)
    cfg.model.gen.shape = cfg.dataset.shape
    torch.save({"step": 0, "G_ema": define_G(cfg).state_dict()}, ckpt)
    path = E.main(["--model-path", ckpt, "--config-path", cfg_path, "--save-dir-path", str(tmp_path / "out"), "--batch-size", "2",
                   "--num-step", "6", "--num-code", "4", "--composition-layer", "backbone.2"])
    rows = list(csv.reader(open(path)))
    assert rows[0] == [""] + E.COLUMNS and len(rows) == 4
    vals = np.array([[float(v) for v in r[1:]] for r in rows[1:]])
    assert np.isfinite(vals).all(), vals
