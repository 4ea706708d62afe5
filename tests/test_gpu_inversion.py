"""GAN inversion on the MI355X (dusty_gan_amd.inversion, csrc/inversion.hip): parity with the reference's loop
(tests/golden/inversion.npz and its restatement in tests/test_inversion_cpu.py), the loss kernel against the head
post-processing's backward, the depth metrics, the paired Chamfer distance, determinism, batch independence,
isolation from a live trainer, and a full-width self-inversion."""

import math

import numpy as np
import pytest
import torch

from tests.golden_util import load
from tests.test_inversion_cpu import ARCHS, DISTANCES, fixture_case, oracle_invert

pytestmark = pytest.mark.gpu
DEV = "cuda"


def make_G(arch, params, in_ch=8, ch_base=4, ch_max=16, shape=(32, 64), dtype=torch.float32):
    from dusty_gan_amd.models import dusty
    from dusty_gan_amd.models.gans.dcgan_eqlr import Generator
    heads = {"none": {"depth": 1}, "dusty1": {"depth": 1, "confidence": 1}, "dusty2": {"depth": 1, "confidence": 2}}[arch]
    bb = Generator(in_ch, heads, ch_base, ch_max, shape, ring=True)
    bb.set_precision(dtype)
    G = bb if arch == "none" else {"dusty1": dusty.DUSty1, "dusty2": dusty.DUSty2}[arch](bb, tau=1, drop_const=-1)
    if params is not None:
        G.load_state_dict(params)
    G.to(DEV)
    G.eval()
    return G


def run_case(arch, distance, dtype=torch.float32, graph=False):
    from dusty_gan_amd.inversion import invert
    g = load("inversion")
    params, gumbel, inv_ref, mask, latent0, noise, S = fixture_case(g, arch, distance)
    G = make_G(arch, params, dtype=dtype)
    steps = []
    res = invert(G, inv_ref.to(DEV), mask.to(DEV), num_step=S, distance=distance, latent=latent0,
                 noise_fn=lambda k: noise[k], gumbel_noise=gumbel,
                 on_step=lambda k, loss, grad, lat: steps.append((loss.cpu(), grad.cpu(), lat.cpu())))
    return g, steps, res


def rel_max(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def cosine(a, b):
    return float((a * b).sum() / (a.norm() * b.norm()))


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("distance", DISTANCES)
def test_fp32_matches_reference_fixture(arch, distance):
    g, steps, res = run_case(arch, distance)
    pre = f"{arch}_{distance}/"
    loss0 = torch.from_numpy(g[pre + "s0/loss"])
    assert float(((steps[0][0] - loss0).abs() / loss0.abs()).max()) <= 1e-5
    for k, (loss, grad, lat) in enumerate(steps):
        gr = torch.from_numpy(g[pre + f"s{k}/grad"])
        for b in range(gr.shape[0]):
            assert rel_max(grad[b], gr[b]) <= 1e-4 and cosine(grad[b], gr[b]) >= 0.99999, (k, b)
        # the latent after each step: a gradient component within rounding of zero could flip Adam's early ~lr sign(g)
        # steps; none of the fixture's components is that small (min |g| / max |g| is checked here), so the bound is tight
        assert float(gr.abs().min() / gr.abs().max()) > 1e-4 or k == 0, k
        assert float((lat - torch.from_numpy(g[pre + f"s{k}/latent"])).abs().max()) <= 1e-4, k
    assert torch.equal(res["latent"].cpu(), steps[-1][2])
    assert torch.equal(res["loss"].cpu(), steps[-1][0])


# bf16 G against the bf16-EMULATING oracle (oracle.dusty_oracle._Emu: it rounds to bf16 exactly where the engine stores bf16 -
# latent, weight shadows, feature maps, the backward-data chain; the head output, the loss and the optimizer stay fp32).
# What remains is fp32 accumulation order inside the convolutions (matrix cores against ATen), which now and then moves a
# stored value across a bf16 rounding boundary (one bf16 ulp = 2^-7 relative).  Step 0 runs with lr = 0, so steps 0-1 see
# the same latent on both sides; after that the two trajectories differ by those roundings, and under l1 a pixel whose
# output lies within them of its target flips its sign(gen - ref) term of the gradient - the comparison is sensitive there.
# Measured on an MI355X, all three archs x both distances x all six steps, worst case over two builds whose Adam step
# sizes differed by one fp32 rounding (which alone took dusty2-l1 from bit-equal gradients to the worst row below):
#   loss 1.4e-4 relative (dusty1 l2, step 5); d loss/dz 6.7e-2 of max, cosine 0.99769 (dusty2 l1, step 4);
#   latent 1.8e-2 absolute (dusty2 l1, step 4); in the final build 24 of the 36 (case, step) pairs have bit-equal gradients
#   and the worst are 2.1e-2 / 0.99976 / 4.8e-3.
# Bounds: 5e-4 / 0.15 / cosine 0.995 / 4e-2 - 3.6x, 2.2x, 2.2x (on 1 - cos) and 2.2x the worst seen.
BF16 = dict(loss=5e-4, grad=0.15, cos=0.995, latent=4e-2)


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("distance", DISTANCES)
def test_bf16_matches_emulating_oracle(arch, distance):
    g = load("inversion")
    params, gumbel, inv_ref, mask, latent0, noise, S = fixture_case(g, arch, distance)
    _, steps, _ = run_case(arch, distance, dtype=torch.bfloat16)
    ref = oracle_invert(params, arch, gumbel, inv_ref, mask, latent0, noise, S, distance, dtype=torch.bfloat16)
    for k, ((loss, grad, lat), (l_r, g_r, lat_r)) in enumerate(zip(steps, ref)):
        assert float(((loss - l_r).abs() / l_r.abs()).max()) <= BF16["loss"], k
        for b in range(grad.shape[0]):
            assert rel_max(grad[b], g_r[b]) <= BF16["grad"] and cosine(grad[b], g_r[b]) >= BF16["cos"], (k, b)
        assert float((lat - lat_r).abs().max()) <= BF16["latent"], k


def test_loss_grad_kernel_equals_head_post_bwd():
    """arch none, fp32: dg_inv_loss_grad's head gradient == dg_head_post_bwd fed with torch's d loss / d depth"""
    from dusty_gan_amd import _lib as L
    g = load("inversion")
    params, gumbel, inv_ref, mask, latent0, noise, S = fixture_case(g, "none", "l2")
    G = make_G("none", params)
    eng = G.engine()
    z = latent0.to(DEV)
    out = G(z)
    depth = out["depth"].detach().clone().requires_grad_()
    ref, m = inv_ref.to(DEV), mask.to(DEV)
    loss = (((ref - (depth + 1) / 2) ** 2) * m).sum(dim=(1, 2, 3)) / m.sum(dim=(1, 2, 3))
    loss.sum().backward()
    lib, B, HW = L.lib(), z.shape[0], eng.HW
    want = torch.zeros_like(eng.draw)
    L.check(lib.dg_head_post_bwd(L.ptr(eng.gout), None, None, None, L.ptr(depth.grad.contiguous()), 0, 1.0, -1.0, B, HW,
                                 eng.head_scales[0], 0.0, L.ptr(want), None, None, 1, None, L.stream_ptr()), "dg_head_post_bwd")
    got = torch.zeros_like(eng.draw)
    msum = m.sum(dim=(1, 2, 3)).contiguous()
    lo = torch.empty(B, device=DEV)
    parts, tk = torch.zeros(B * 2, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    L.check(lib.dg_inv_loss_grad(L.ptr(eng.gout), HW, 1, L.ptr(ref), L.ptr(m), L.ptr(msum), 1, B, HW, eng.head_scales[0],
                                 L.ptr(got), 1, None, 1, L.ptr(parts), L.ptr(tk), 2, L.ptr(lo), L.stream_ptr()), "dg_inv_loss_grad")
    assert rel_max(got, want) <= 1e-6
    assert torch.allclose(lo, loss.detach(), rtol=1e-6, atol=0)
    from dusty_gan_amd.utils import masked_loss
    assert torch.allclose(masked_loss(ref, (depth.detach() + 1) / 2, m, "l2"), loss.detach(), rtol=1e-6, atol=0)
    assert int(tk.abs().sum()) == 0 and float(parts.abs().sum()) == 0.0   # scratch left zero


def test_depth_metrics_match_reference():
    from dusty_gan_amd.utils.metrics.depth import compute_depth_accuracy, compute_depth_error
    g = load("inversion")
    ref, gen, mask = (torch.from_numpy(g[f"depth/{k}"]).to(DEV) for k in ("ref", "gen", "mask"))
    for name, d in (("error", compute_depth_error(ref, gen, mask)), ("accuracy", compute_depth_accuracy(ref, gen, mask))):
        for k, v in d.items():
            want = torch.from_numpy(g[f"depth/{name}/{k}"])
            v = v.cpu()
            assert torch.equal(torch.isnan(v), torch.isnan(want)), k
            ok = ~torch.isnan(want)
            assert float(((v[ok] - want[ok]).abs() / want[ok].abs().clamp_min(1e-6)).max()) <= 1e-5, k


def test_compute_cd_is_the_diagonal():
    """paired Chamfer == diag of the all-pairs matrix.  Clouds above 1024 points sum their 512-point slices with float
    atomics in both launches (arrival order), so the two agree to the rounding of that sum, not bit for bit"""
    from dusty_gan_amd.utils.metrics import chamfer_distance_matrix, compute_cd
    gen = torch.Generator().manual_seed(3)
    for n in (300, 1000, 4096):
        a = torch.rand(5, n, 3, generator=gen).to(DEV)
        b = torch.rand(5, n, 3, generator=gen).to(DEV)
        cd = compute_cd(a, b).cpu()
        diag = torch.diagonal(chamfer_distance_matrix(a, b)).cpu()
        if n <= 1024:
            assert torch.equal(cd, diag), n
        else:
            assert float(((cd - diag).abs() / diag).max()) <= 1e-6, n
    # the reference's own CPU search (tests/golden/chamfer.npz case 2: per-point minima of every pair of two 5-cloud sets)
    from dusty_gan_amd.utils.metrics import chamfer_paired
    c = load("chamfer")
    A, Bc, dist = (torch.from_numpy(c[f"2/{k}"]) for k in ("A", "B", "dist"))
    got = chamfer_paired(A.to(DEV).float(), Bc.to(DEV).float()).cpu()
    want = torch.stack([dist[i, i].double().mean() for i in range(A.shape[0])]).float()
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-7)


def test_deterministic_and_graph_equals_eager():
    from dusty_gan_amd.inversion import invert
    g = load("inversion")
    params, gumbel, inv_ref, mask, latent0, noise, S = fixture_case(g, "dusty2", "l1")
    G = make_G("dusty2", params)
    a = invert(G, inv_ref.to(DEV), mask.to(DEV), num_step=12, seed=5, gumbel_noise=gumbel, graph=True)
    b = invert(G, inv_ref.to(DEV), mask.to(DEV), num_step=12, seed=5, gumbel_noise=gumbel, graph=True)
    c = invert(G, inv_ref.to(DEV), mask.to(DEV), num_step=12, seed=5, gumbel_noise=gumbel, graph=False)
    for k in ("latent", "loss", "inv_gen"):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    for k in a["out"]:
        assert torch.equal(a["out"][k], c["out"][k]), k


def test_batch_independence():
    from dusty_gan_amd.inversion import invert
    g = load("inversion")
    params, gumbel, inv_ref, mask, latent0, noise, S = fixture_case(g, "dusty1", "l2")
    G = make_G("dusty1", params)
    gen = torch.Generator().manual_seed(9)
    lat = torch.randn(4, 8, generator=gen)
    nz = torch.randn(S, 4, 8, generator=gen) * 0.03
    ref4 = torch.cat([inv_ref, inv_ref[:1]]).to(DEV)
    m4 = torch.cat([mask, mask[:1]]).to(DEV)
    full = invert(G, ref4, m4, num_step=S, latent=lat, noise_fn=lambda k: nz[k], gumbel_noise=gumbel)
    for i in range(4):
        one = invert(G, ref4[i:i + 1], m4[i:i + 1], num_step=S, latent=lat[i:i + 1], noise_fn=lambda k: nz[k, i:i + 1],
                     gumbel_noise=gumbel)
        assert float((one["latent"][0] - full["latent"][i]).abs().max()) <= 1e-5, i
        assert abs(float(one["loss"][0] - full["loss"][i])) <= 1e-5 * max(1.0, abs(float(full["loss"][i]))), i
    # the Philox perturbation is keyed by the row: row 0 draws the same noise alone as inside the batch
    a = invert(G, ref4, m4, num_step=S, latent=lat, seed=2, gumbel_noise=gumbel)
    b = invert(G, ref4[:1], m4[:1], num_step=S, latent=lat[:1], seed=2, gumbel_noise=gumbel)
    assert float((a["latent"][0] - b["latent"][0]).abs().max()) <= 1e-5


def test_invert_leaves_a_live_trainer_untouched():
    from dusty_gan_amd.inversion import invert
    from tests.test_gpu_step import make_trainer
    tr = make_trainer("dusty2", True, (32, 64), 8, 4, 16, 2)

    def snap():
        out = {}
        for name in ("G", "D", "G_ema"):
            net = getattr(tr, name)
            st = (net.backbone if hasattr(net, "backbone") else net).store
            out[name] = st.flat.detach().clone()
            if getattr(st, "grad", None) is not None:
                out[name + ".grad"] = st.grad.detach().clone()
        for oname in ("optim_G", "optim_D"):
            opt = getattr(tr, oname)
            for k, v in vars(opt).items():
                if isinstance(v, torch.Tensor):
                    out[f"{oname}.{k}"] = v.detach().clone()
        out["rng"] = tr.rng.ctr.clone()
        return out

    before = snap()
    inv = torch.rand(2, 1, 32, 64, device=DEV)
    invert(tr.G_ema, inv, torch.ones_like(inv), num_step=8)
    after = snap()
    assert before.keys() == after.keys()
    for k in before:
        assert torch.equal(before[k], after[k]), k


def test_next_trainer_step_equals_a_twin_that_never_inverted(monkeypatch):
    """invert on a live trainer's G_ema between two of its replayed (hipGraph) steps: the trainer's following steps equal,
    bit for bit, those of a twin built from the same seed that never inverted - scalars and G, D, G_ema.  (What a snapshot
    of tensors cannot show: a shared split-K workspace, capture stream, counter queue or engine buffer would.)"""
    from dusty_gan_amd.inversion import invert
    from tests.test_gpu_step import make_trainer
    monkeypatch.setenv("DUSTY_GAN_GRAPH", "1")

    def make():
        torch.manual_seed(21)
        return make_trainer("dusty2", True, (32, 64), 8, 4, 16, 4)
    a, b = make(), make()
    for i in range(3):
        assert a.step(i) == b.step(i)
    assert a._graph is not None and b._graph is not None
    inv = torch.rand(3, 1, 32, 64, device=DEV)
    invert(a.G_ema, inv, (inv > 0.2).float(), num_step=12, seed=4, graph=True)
    invert(a.G_ema, inv, (inv > 0.2).float(), num_step=3, seed=4, graph=False)
    for i in range(3, 6):
        sa, sb = a.step(i), b.step(i)
        assert sa == sb, (i, sa, sb)
    for net in ("G", "D", "G_ema"):
        fa = getattr(a, net).store.flat if not hasattr(getattr(a, net), "backbone") else getattr(a, net).backbone.store.flat
        fb = getattr(b, net).store.flat if not hasattr(getattr(b, net), "backbone") else getattr(b, net).backbone.store.flat
        assert torch.equal(fa, fb), net


def test_device_drawn_perturbation_follows_the_schedule():
    """the latent perturbation dg_sphere_adam draws on the device: with lr = 0 the latent stays put, so the generator input
    it writes for step k + 1 minus the latent is the perturbation itself.  Per step its RMS over 16 x 512 draws is
    noise_strength(k + 1) within 5 % (the RMS of n = 8192 standard normals has relative sd 1 / sqrt(2 n) = 0.8 %: six sd),
    its mean within 5 sd of zero, and it is exactly zero once progress reaches noise_ratio.  noise_sigma = 2 and
    noise_ratio = 0.5 pin both arguments."""
    from dusty_gan_amd.inversion import invert, noise_strength
    G = make_G("none", None, in_ch=512)
    eng = G.engine()
    B, n_step = 16, 8
    ref = torch.rand(B, 1, 32, 64, device=DEV)
    seen = []

    def on_step(k, loss, grad, lat):
        seen.append((k, (eng.zT.view(B, 512).float() - lat.to(DEV)).cpu()))
    invert(G, ref, torch.ones_like(ref), num_step=n_step, lr=0.0, noise_sigma=2.0, noise_ratio=0.5, seed=3,
           on_step=on_step)
    assert [k for k, _ in seen] == list(range(n_step))
    for k, d in seen:
        want = noise_strength(k + 1, n_step, 0.5, 2.0)
        if want == 0.0:
            assert torch.count_nonzero(d) == 0, k
            continue
        rms = float(d.pow(2).mean().sqrt())
        assert abs(rms / want - 1) < 0.05, (k, rms, want)
        assert abs(float(d.mean())) < 5 * want / math.sqrt(d.numel()), k
        frac = float((d.abs() < want).float().mean())      # P(|N(0,1)| < 1) = 0.6827, sd 0.005 at n = 8192
        assert abs(frac - 0.6827) < 0.03, (k, frac)
    assert seen[0][1].abs().max() > 0 and not torch.equal(seen[0][1], seen[1][1])   # fresh draws every step


def test_full_width_self_inversion_bf16():
    """64x1024, nz 512, ch_base 64, dusty2, bf16, B = 8: 200 steps on targets G(z*) lower every sample's masked L1.
    Calibrated on an MI355X: final / first-step loss 0.005 ... 0.162 over the eight samples; bound 0.3 (1.85x margin)"""
    from dusty_gan_amd.inversion import invert
    from dusty_gan_amd.utils import masked_loss
    torch.manual_seed(0)
    G = make_G("dusty2", None, in_ch=512, ch_base=64, ch_max=512, shape=(64, 1024), dtype=torch.bfloat16)
    B = 8
    zs = torch.randn(B, 512, device=DEV)
    gum = torch.zeros(1, 1, 64, 1024)
    with torch.no_grad():
        out = G(zs, noise={"pixel": gum.to(DEV).expand(B, 1, 64, 1024).contiguous()})
        target = (out["depth_orig"].clone() + 1) / 2
    mask = (torch.rand(B, 1, 64, 1024, device=DEV) > 0.1).float()
    res1 = invert(G, target, mask, num_step=1, seed=1, gumbel_noise=gum)
    res = invert(G, target, mask, num_step=200, seed=1, gumbel_noise=gum)
    l0, l1 = res1["loss"].cpu(), res["loss"].cpu()
    ratio = (l1 / l0)
    print("self-inversion loss ratio after 200 steps:", ratio.tolist())
    assert bool(torch.isfinite(l1).all()) and bool((ratio < 0.3).all()), ratio
    assert torch.allclose(masked_loss(target, res["inv_gen"], mask, "l1").cpu(), l1, rtol=1e-5, atol=0)


def test_evaluate_reconstruction_end_to_end(tmp_path):
    """the evaluation command on a synthetic full-width dusty2 bf16 checkpoint and three .npy test scans (batch 2: a full
    and a ragged batch): one finite CSV row per scan in the reference's columns"""
    import csv
    import os

    from dusty_gan_amd import evaluate_reconstruction as E
    from dusty_gan_amd.models import define_G
    from dusty_gan_amd.utils.config import dump_config, load_config
    from tests.test_gpu_data import write_kitti_tree
    root = str(tmp_path / "kitti")
    write_kitti_tree(root, 64, 2048, {11: 3})   # sequence 11: the test split
    cfg = load_config(["model=dusty2_dcgan_eqlr", "dataset=kitti_odometry", f"dataset.root={root}",
                       "dataset.shape=[64,1024]", "enable_amp=true"])
    cfg_path, ckpt = str(tmp_path / "config.yaml"), str(tmp_path / "model.pth")
    dump_config(cfg, cfg_path)
    torch.manual_seed(0)
    cfg.model.gen.shape = cfg.dataset.shape
    torch.save({"step": 0, "G_ema": define_G(cfg).state_dict()}, ckpt)
    out_dir = str(tmp_path / "out")
    path = E.main(["--model-path", ckpt, "--config-path", cfg_path, "--save-dir-path", out_dir, "--batch-size", "2",
                   "--num-step", "20"])
    rows = list(csv.reader(open(path)))
    assert rows[0] == [""] + E.COLUMNS and len(rows) == 4
    vals = np.array([[float(v) for v in r[1:]] for r in rows[1:]])
    assert np.isfinite(vals).all(), vals
    assert os.path.dirname(path) == out_dir
