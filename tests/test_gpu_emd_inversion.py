"""GAN inversion with the earth mover's term on the MI355X (dg_points_gather, dg_inv_points_grad,
dusty_gan_amd.inversion.invert(distance="emd")) against tests/golden/emd_inversion.npz: the reference's modules run in
float64 over the restated EarthMoverDistanceFunction, with e_ref = |reference float32 - float64| as the yardstick of every
bound.

Figures measured on an MI355X are printed by every test before it asserts."""
import math

import numpy as np
import pytest
import torch

from tests import chamfer_inv_util as CU
from tests import emd_inv_util as U
from tests.golden_util import load
from tests.test_gpu_inversion import make_G

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W, HW = U.H, U.W, U.HW


def make_lidar(max_depth=120.0):
    from dusty_gan_amd.utils.lidar import LiDAR
    lidar = LiDAR(H, W, CU.MIN_DEPTH, max_depth)
    lidar.angle = CU.angle_grid(H, W).to(DEV)
    return lidar


def case(name):
    return U.fixture_case(load("emd_inversion"), load("chamfer_inversion"), name)


def gather(X, strides, n, idx):
    from dusty_gan_amd import _lib as L
    B, K = idx.shape
    out = torch.full((B, K, 3), float("nan"), device=DEV)
    L.check(L.lib().dg_points_gather(L.ptr(X), *strides, n, L.ptr(idx), B, K, L.ptr(out), L.stream_ptr()), "dg_points_gather")
    return out


@pytest.mark.parametrize("K", (1, 64, 700))
def test_gather_equals_indexing_in_both_stride_forms(K):
    gen = torch.Generator().manual_seed(K)
    B, n = 3, 2048
    packed = torch.randn(B, n, 3, generator=gen).to(DEV)
    planar = packed.transpose(1, 2).contiguous()
    idx = torch.stack([torch.randperm(n, generator=gen)[:K] for _ in range(B)]).to(torch.int32).to(DEV)
    want = packed.gather(1, idx.long()[:, :, None].expand(-1, -1, 3))
    assert torch.equal(gather(planar, (3 * n, 1, n), n, idx), want)
    assert torch.equal(gather(packed, (3 * n, 3, 1), n, idx), want)
    bad = idx.clone()
    bad[0, 0], bad[B - 1, K - 1] = -1, n          # outside [0, n): zeros, the rest as before
    want[0, 0], want[B - 1, K - 1] = 0.0, 0.0
    assert torch.equal(gather(planar, (3 * n, 1, n), n, bad), want)
    assert torch.equal(gather(packed, (3 * n, 3, 1), n, bad), want)


@pytest.mark.parametrize("name", [c[0] for c in U.CASES])
def test_engine_sample_is_the_fixtures(name):
    from dusty_gan_amd.inversion import EmdState, PointMaps
    params, gumbel, inv_ref, mask, latent0, noise, S, idx, max_depth = case(name)
    M = EmdState(PointMaps(inv_ref.to(DEV), make_lidar(max_depth), CU.TOL), idx.shape[1])
    got = M.idx.cpu().long()
    print(f"{name}: indices off the fixture's {int((got != idx).sum())} of {idx.numel()}")
    assert torch.equal(got, idx)
    slot = M.slot.cpu().long()
    K = idx.shape[1]
    assert torch.equal(slot.gather(1, idx), torch.arange(K).expand(3, K))          # the inverse on the sample ...
    assert int((slot >= 0).sum()) == 3 * K and int(slot.min()) == -1               # ... and -1 everywhere else
    assert torch.equal(M.Rs.cpu(), M.maps.R.flatten(2).transpose(1, 2).cpu().gather(1, idx[:, :, None].expand(-1, -1, 3)))


def head_inputs(g, name):
    """the forward pass's buffers as dg_head_post_fwd leaves them in eval mode, from the recorded step-0 head output"""
    params, gumbel, inv_ref, mask, latent0, noise, S, idx, max_depth = case(name)
    raw = torch.from_numpy(g[f"{name}/head/raw"])
    B, nh = raw.shape[:2]
    gout = raw.clone()
    gout[:, 0] = torch.tanh(raw[:, 0].double()).float()
    m = torch.ones(B, max(nh - 1, 1), H, W)
    if nh >= 2:
        m[:, 0] = ((raw[:, 1] + gumbel[0, 0]) > 0).float()    # sigmoid(l / tau) > 0.5
    if nh == 3:
        m[:, 1] = (raw[:, 2] > 0).float()
    keep = m.prod(dim=1, keepdim=True)
    depth = keep * gout[:, 0:1] + (1 - keep) * -1.0
    return inv_ref, gumbel.expand(B, 1, H, W).contiguous(), gout, m, depth, idx


def run_points_grad(lidar, inv_ref, noise_pixel, gout, m, depth, idx, arch_id, prior=None, prior_loss=None):
    """gather -> dg_emd_grad -> dg_inv_points_grad, twice; prior: the head gradient and loss of an earlier term (add = 1)"""
    from dusty_gan_amd import _lib as L
    from dusty_gan_amd.utils.metrics.distance import earth_mover_distance
    lib, sp = L.lib(), L.stream_ptr()
    B, nh = gout.shape[:2]
    K = idx.shape[1]
    cp = 2 if nh <= 2 else 4
    dev = lambda t: t.to(DEV).float().contiguous()
    inv_ref, noise_pixel, gout, m, depth = map(dev, (inv_ref, noise_pixel, gout, m, depth))
    idx32 = idx.to(torch.int32).to(DEV)
    R = lidar.inv_to_xyz(inv_ref, tol=CU.TOL)
    P = lidar.inv_to_xyz(depth, tol=CU.TOL, from_tanh=True)
    angle = lidar.angle.reshape(2, HW).contiguous()
    Rs, Ps = gather(R, (3 * HW, 1, HW), HW, idx32), gather(P, (3 * HW, 1, HW), HW, idx32)
    cost = torch.empty(B, device=DEV)
    gA, gB = torch.empty_like(Ps), torch.empty_like(Ps)
    scale = torch.full((B,), 1.0 / K, device=DEV)
    L.check(lib.dg_emd_grad(L.ptr(Ps), K, L.ptr(Rs), K, B, L.ptr(scale), L.ptr(cost), L.ptr(gA), L.ptr(gB), sp), "dg_emd_grad")
    assert torch.equal(cost, earth_mover_distance(Ps, Rs))
    slot = torch.full((B, HW), -1, dtype=torch.int32, device=DEV)
    slot.scatter_(1, idx.to(DEV), torch.arange(K, dtype=torch.int32, device=DEV).expand(B, K))
    s_depth = 1.0 / math.sqrt(16.0)
    s_conf = 1.0 / math.sqrt((nh - 1) * 16.0) if nh > 1 else 0.0
    res = []
    for _ in range(2):
        draw = torch.full((B, nh, H, W), float("nan"), device=DEV) if prior is None else prior.to(DEV).clone()
        pm = torch.full((B, H, W, cp), float("nan"), dtype=torch.bfloat16, device=DEV)
        loss = torch.full((B,), float("nan"), device=DEV) if prior is None else prior_loss.to(DEV).clone()
        L.check(lib.dg_inv_points_grad(L.ptr(gA), L.ptr(slot), L.ptr(cost), 1.0 / K, K, L.ptr(depth), L.ptr(angle), L.ptr(gout),
                                       L.ptr(noise_pixel) if arch_id else None, L.ptr(m) if arch_id else None, arch_id, 1.0, -1.0,
                                       CU.MIN_DEPTH, lidar.max_depth, CU.TOL, B, HW, s_depth, s_conf, int(prior is not None),
                                       L.ptr(draw), nh, L.ptr(pm), cp, 2, L.ptr(loss), sp), "dg_inv_points_grad")
        res.append((draw.cpu(), pm.cpu(), loss.cpu()))
    return res, (s_depth, s_conf), cost.cpu()


@pytest.mark.parametrize("name,arch,distance,K,inputs,max_depth", U.SINGLE)
def test_points_grad_matches_float64(name, arch, distance, K, inputs, max_depth):
    """Per element 4 e_ref + 1e-6 max|grad|: the factor the project gives a row of the EMD gradient
    (tests/test_gpu_point_distance_grad.py test_emd_grad_matches_the_fixture), the floor of the Chamfer term's head gradient."""
    g = load("emd_inversion")
    arch_id = CU.ARCHS.index(arch)
    inputs = head_inputs(g, name)
    (first, second), (s_depth, s_conf), cost = run_points_grad(make_lidar(max_depth), *inputs, arch_id)
    draw, pm, loss = first
    scale = torch.tensor([s_depth, s_conf, s_conf][:draw.shape[1]]).view(1, -1, 1, 1)
    want = torch.from_numpy(g[f"{name}/head/grad"]).double() * scale
    e_ref = torch.from_numpy(g[f"{name}/head/e_grad"]).double() * scale
    err = (draw.double() - want).abs()
    bound = 4 * e_ref + 1e-6 * float(want.abs().max())
    print(f"{name}: head gradient max |err| {float(err.max()):.3g} (max |grad| {float(want.abs().max()):.3g}, max e_ref "
          f"{float(e_ref.max()):.3g}), worst err / bound {float((err / bound).max()):.3g}, elements over {int((err > bound).sum())}, "
          f"non-zero pixels {int((draw.abs().sum(dim=1) > 0).sum())}")
    l64, e_l = torch.from_numpy(g[f"{name}/s0/loss"]), torch.from_numpy(g[f"{name}/s0/e_loss"]).double()
    print(f"{name}: step-0 loss |err| {(loss.double() - l64).abs().tolist()} e_ref {e_l.tolist()}")
    assert bool((err <= bound).all())
    assert torch.equal(loss, cost * torch.tensor(1.0 / K, dtype=torch.float32))      # cost / K: the product, rounded once
    assert bool(((loss.double() - l64).abs() <= 4 * e_l + 1e-5 * l64.abs()).all())
    if arch == "dusty2":
        assert not bool(draw[:, 2].any())                                             # eval mode: the image-level mask is a threshold
    nh = draw.shape[1]
    assert torch.equal(pm[..., :nh], draw.permute(0, 2, 3, 1).to(torch.bfloat16))     # round to nearest even
    assert not bool(pm[..., nh:].any())
    for x, y in zip(first, second):                                                   # a second call: identical bytes
        assert torch.equal(x, y)
    # add = 1 on a pre-filled gradient: the fill plus this term's gradient, to half an ulp of the gradient plus one of the sum
    gen = torch.Generator().manual_seed(8)
    prior = torch.randn(draw.shape, generator=gen) * float(draw.abs().max())
    prior_loss = torch.rand(loss.shape, generator=gen)
    (added, again), _, _ = run_points_grad(make_lidar(max_depth), *inputs, arch_id, prior=prior, prior_loss=prior_loss)
    total = prior + draw
    err = (added[0].double() - total.double()).abs()
    assert bool((err <= 2.0 ** -24 * draw.abs().double() + 2.0 ** -23 * total.abs().double()).all())
    assert torch.equal(added[2], prior_loss + loss)
    assert torch.equal(added[1][..., :nh], added[0].permute(0, 2, 3, 1).to(torch.bfloat16)) and not bool(added[1][..., nh:].any())
    for x, y in zip(added, again):
        assert torch.equal(x, y)


def run_case(name, arch, distance, dtype=torch.float32):
    from dusty_gan_amd.inversion import invert
    g = load("emd_inversion")
    params, gumbel, inv_ref, mask, latent0, noise, S, idx, max_depth = case(name)
    G = make_G(arch, params, dtype=dtype)
    steps = []
    res = invert(G, inv_ref.to(DEV), mask.to(DEV), num_step=S, distance=distance[0] if len(distance) == 1 else distance,
                 latent=latent0, noise_fn=lambda k: noise[k], gumbel_noise=gumbel, lidar=make_lidar(max_depth), tol=CU.TOL,
                 emd_points=idx.shape[1], on_step=lambda k, loss, grad, lat: steps.append((loss.cpu(), grad.cpu(), lat.cpu())))
    return g, steps, res


@pytest.mark.parametrize("name,arch,distance,K,inputs,max_depth", U.CASES)
def test_fp32_steps_match_float64(name, arch, distance, K, inputs, max_depth):
    """Per step, against the reference's float64 run: loss, d loss / d latent and the latent within 4 e_ref plus the fp32
    engine's floors of tests/test_gpu_chamfer_inversion.py: 1e-5 of the loss, 1e-4 of the sample's largest gradient component,
    1e-4 absolute on the latent."""
    g, steps, res = run_case(name, arch, distance)
    ok = True
    for k, (loss, grad, lat) in enumerate(steps):
        rows = []
        for key, got in (("loss", loss), ("grad", grad), ("latent", lat)):
            w = torch.from_numpy(g[f"{name}/s{k}/{key}"])
            e = torch.from_numpy(g[f"{name}/s{k}/e_{key}"]).double()
            if key == "loss":
                floor = 1e-5 * w.abs()
            elif key == "grad":
                floor = 1e-4 * w.abs().max(dim=1, keepdim=True).values
            else:
                floor = torch.full_like(w, 1e-4)
            err = (got.double() - w).abs()
            bound = 4 * e + floor
            rows.append(f"{key} err {float(err.max()):.3g} e_ref {float(e.max()):.3g} err/bound {float((err / bound).max()):.3g}")
            ok = ok and bool((err <= bound).all())
        print(f"{name} step {k}: " + "; ".join(rows))
    assert ok
    assert torch.equal(res["latent"].cpu(), steps[-1][2]) and torch.equal(res["loss"].cpu(), steps[-1][0])


def dusty2_run(dtype=torch.float32, **fixed):
    from dusty_gan_amd.inversion import invert
    params, gumbel, inv_ref, mask, latent0, noise, S, idx, max_depth = case("dusty2_l1_emd")
    G = make_G("dusty2", params, dtype=dtype)
    kw = dict(num_step=8, seed=5, gumbel_noise=gumbel, lidar=make_lidar(max_depth), emd_points=100)
    kw.update(fixed)
    return lambda **more: invert(G, inv_ref.to(DEV), mask.to(DEV), **{**kw, **more})


@pytest.mark.parametrize("distance", ("emd", ("l1", "emd"), ("chamfer", "emd")))
def test_deterministic_and_graph_equals_eager(distance):
    run = dusty2_run()
    a, b, c = run(distance=distance, graph=True), run(distance=distance, graph=True), run(distance=distance, graph=False)
    for k in ("latent", "loss"):
        assert bool(torch.isfinite(a[k]).all()), k
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k


def test_emd_points_is_not_looked_at_without_emd():
    run = dusty2_run()
    for distance in ("l1", ("l1", "chamfer")):
        a, b = run(distance=distance, emd_points=2048), run(distance=distance, emd_points=7)
        for k in ("latent", "loss", "inv_gen"):
            assert torch.equal(a[k], b[k]), (distance, k)


def test_bf16_engine_runs_and_graph_equals_eager():
    """No tolerance against the reference is invented for bf16: its distance to the fp32 engine at step 0 is printed."""
    run = dusty2_run(torch.bfloat16)
    for distance in ("emd", ("l1", "emd"), ("chamfer", "emd")):
        a, c = run(distance=distance, graph=True), run(distance=distance, graph=False)
        for k in ("latent", "loss"):
            assert bool(torch.isfinite(a[k]).all()), (distance, k)
            assert torch.equal(a[k], c[k]), (distance, k)
    first = {}
    for dtype in (torch.float32, torch.bfloat16):
        steps = []
        dusty2_run(dtype)(distance="emd", num_step=1, perturb_latent=False, latent=case("dusty2_l1_emd")[4],
                          on_step=lambda k, loss, grad, lat: steps.append((loss.cpu().double(), grad.cpu().double())))
        first[dtype] = steps[0]
    (l32, g32), (l16, g16) = first[torch.float32], first[torch.bfloat16]
    print(f"bf16 engine against the fp32 engine, emd at K = 100, step 0: loss off by {float(((l16 - l32).abs() / l32).max()):.3g} "
          f"relative, d loss / d latent by {float((g16 - g32).abs().max() / g32.abs().max()):.3g} of its largest component")
    assert bool(torch.isfinite(g16).all())


def test_multi_code_graph_equals_eager():
    run = dusty2_run(distance=("l1", "emd"), num_code=2, composition_layer=1)
    a, b, c = run(graph=True), run(graph=True), run(graph=False)
    for k in ("latent", "loss", "alpha"):
        assert bool(torch.isfinite(a[k]).all()), k
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    assert a["latent"].shape[:2] == (3, 2)


def test_refusals_come_before_the_first_step(monkeypatch):
    from dusty_gan_amd import engine as E
    from dusty_gan_amd.inversion import invert
    params, gumbel, inv_ref, mask, latent0, noise, S, idx, max_depth = case("dusty2_l1_emd")
    G = make_G("dusty2", params)

    def no_step(*a, **k):
        raise AssertionError("a step was launched")
    monkeypatch.setattr(E.GEngine, "inversion_step", no_step)
    few_ref, few_mask = inv_ref.clone(), mask.clone()
    few_mask[1].view(-1)[40:] = 0.0          # scan 1 keeps at most 40 rays: fewer than K = 64 candidates
    few_ref = few_ref * few_mask
    with pytest.raises(ValueError, match=r"scan\(s\) \[1\]"):
        invert(G, few_ref.to(DEV), few_mask.to(DEV), num_step=3, distance="emd", lidar=make_lidar(), emd_points=64)
    with pytest.raises(ValueError, match=r"scan\(s\) \[1\]"):
        invert(G, few_ref.to(DEV), few_mask.to(DEV), num_step=3, distance=("l1", "emd"), lidar=make_lidar(), emd_points=64)
    with pytest.raises(ValueError):
        invert(G, inv_ref.to(DEV), mask.to(DEV), num_step=3, distance="emd", lidar=make_lidar(), emd_points=3201)
    with pytest.raises(ValueError):
        invert(G, inv_ref.to(DEV), mask.to(DEV), num_step=3, distance="emd", lidar=make_lidar(), emd_points=HW + 1)


def test_evaluate_reconstruction_with_l1_emd(tmp_path):
    """the evaluation command with --distance l1+emd --emd-points 64 on a small fp32 dusty2 checkpoint and three .npy test
    scans (batch 2: a full and a ragged batch): one finite CSV row per scan, in the columns the command has without the term"""
    import csv

    from dusty_gan_amd import evaluate_reconstruction as E
    from dusty_gan_amd.models import define_G
    from dusty_gan_amd.utils.config import dump_config, load_config
    from tests.test_gpu_data import write_kitti_tree
    from tests.test_inversion_cpu import REF_COLUMNS
    root = str(tmp_path / "kitti")
    write_kitti_tree(root, 32, 128, {11: 3})   # sequence 11: the test split
    cfg = load_config(["model=dusty2_dcgan_eqlr", "dataset=kitti_odometry", f"dataset.root={root}", "dataset.shape=[32,64]",
                       "model.gen.in_ch=8", "model.gen.ch_base=4", "model.gen.ch_max=16", "enable_amp=false"])
    cfg_path, ckpt = str(tmp_path / "config.yaml"), str(tmp_path / "model.pth")
    dump_config(cfg, cfg_path)
    torch.manual_seed(0)
    cfg.model.gen.shape = cfg.dataset.shape
    torch.save({"step": 0, "G_ema": define_G(cfg).state_dict()}, ckpt)
    path = E.main(["--model-path", ckpt, "--config-path", cfg_path, "--save-dir-path", str(tmp_path / "out"), "--batch-size", "2",
                   "--num-step", "6", "--distance", "l1+emd", "--emd-points", "64"])
    rows = list(csv.reader(open(path)))
    assert rows[0] == [""] + REF_COLUMNS and len(rows) == 4
    vals = np.array([[float(v) for v in r[1:]] for r in rows[1:]])
    assert np.isfinite(vals).all(), vals
