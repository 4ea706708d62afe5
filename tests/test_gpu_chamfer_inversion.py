"""GAN inversion with the Chamfer term on the MI355X (dg_chamfer_nn, dg_inv_chamfer_scatter, dg_inv_chamfer_grad,
dusty_gan_amd.inversion.invert(distance="chamfer")) against tests/golden/chamfer_inversion.npz: the reference's modules run
in float64, with e_ref = |reference float32 - float64| as the yardstick of every bound.

Figures measured on an MI355X are printed by every test before it asserts."""
import math

import numpy as np
import pytest
import torch

from tests import chamfer_inv_util as U
from tests.golden_util import load
from tests.test_gpu_inversion import make_G

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W = 32, 64
HW = H * W


def make_lidar():
    from dusty_gan_amd.utils.lidar import LiDAR
    lidar = LiDAR(H, W, U.MIN_DEPTH, U.MAX_DEPTH)
    lidar.angle = U.angle_grid(H, W).to(DEV)
    return lidar


def search(a, b, planar=False):
    """dg_chamfer_nn of clouds a [B,n,3], b [B,m,3] (planar: handed over as [B,3,n] point maps) -> dist, idx on the host"""
    from dusty_gan_amd import _lib as L
    B, n, m = a.shape[0], a.shape[1], b.shape[1]
    a, b = a.to(DEV).float(), b.to(DEV).float()
    if planar:
        a, b = a.transpose(1, 2).contiguous(), b.transpose(1, 2).contiguous()
        sa, sb = (3 * n, 1, n), (3 * m, 1, m)
    else:
        a, b = a.contiguous(), b.contiguous()
        sa, sb = (3 * n, 3, 1), (3 * m, 3, 1)
    dist = torch.full((B, n), -1.0, device=DEV)
    idx = torch.full((B, n), -1, dtype=torch.int32, device=DEV)
    L.check(L.lib().dg_chamfer_nn(L.ptr(a), *sa, n, L.ptr(b), *sb, m, B, L.ptr(dist), L.ptr(idx), L.stream_ptr()), "dg_chamfer_nn")
    return dist.cpu(), idx.cpu().long()


@pytest.mark.parametrize("name", U.PAIR_NAMES)
def test_search_matches_float64(name):
    from dusty_gan_amd.utils.metrics import chamfer_paired
    g = load("chamfer_inversion")
    a, b = U.pair(name, int(g["meta/pair_seed"]))
    fix = torch.from_numpy(g[f"pairs/{name}/idx"]).long()
    # two pairs per launch: the recorded one and the same clouds with their points reversed (sample strides, other slices)
    A, Bc = torch.stack([a, a.flip(0)]), torch.stack([b, b.flip(0)])
    dist, idx = search(A, Bc)
    dist_p, idx_p = search(A, Bc, planar=True)
    assert torch.equal(dist, dist_p) and torch.equal(idx, idx_p)          # both stride forms
    assert int(idx.min()) >= 0 and int(idx.max()) < b.shape[0]
    min64 = (a.double() - b.double()[fix]).pow(2).sum(dim=1)
    for s, (aa, bb, m64) in enumerate(((a, b, min64), (a.flip(0), b.flip(0), min64.flip(0)))):
        d_idx = (aa.double() - bb.double()[idx[s]]).pow(2).sum(dim=1)   # float64 distance of the chosen point
        rel = ((dist[s].double() - m64).abs() / m64.clamp_min(1e-300)).masked_fill(m64 == 0, 0.0)
        print(f"{name}[{s}]: max dist error {float(rel.max()):.3g} relative, indices off the float64 argmin "
              f"{int((d_idx != m64).sum())}")
        assert bool((d_idx <= m64 * (1 + 2.0 ** -20)).all())              # admissible
        assert float(rel.max()) <= 2.0 ** -21 and bool((dist[s][m64 == 0] == 0).all())
    if name == U.DYADIC[0]:   # exact arithmetic, many ties: the LOWEST index, bit-equal distances
        assert torch.equal(idx[0], fix) and torch.equal(dist[0], min64.float())
        d = U.sqdist(a.flip(0).double(), b.flip(0).double())
        assert torch.equal(idx[1], U.nn_first(a.flip(0).double(), b.flip(0).double())[1]) and torch.equal(dist[1], d.min(dim=1).values.float())
    paired = chamfer_paired(A.to(DEV), Bc.to(DEV)).cpu()
    mean = dist.mean(dim=1)
    assert float(((mean - paired).abs() / paired.abs().clamp_min(1e-30)).max()) <= 1e-6


def test_search_refuses_oversized_clouds():
    from dusty_gan_amd import _lib as L
    x = torch.zeros(8, device=DEV)
    i = torch.zeros(8, dtype=torch.int32, device=DEV)
    n = (1 << 18) + 1
    assert L.lib().dg_chamfer_nn(L.ptr(x), 0, 3, 1, n, L.ptr(x), 0, 3, 1, 1, 1, L.ptr(x), L.ptr(i), L.stream_ptr()) == L.DG_EUNSUPPORTED
    assert L.lib().dg_chamfer_nn(L.ptr(x), 0, 3, 1, 1, L.ptr(x), 0, 3, 1, n, 1, L.ptr(x), L.ptr(i), L.stream_ptr()) == L.DG_EUNSUPPORTED


@pytest.mark.parametrize("planar", (False, True))
def test_search_lowest_index_across_chunks_and_the_repeated_tail(planar):
    """The streamed search's tie rule (csrc/nn_stream.h), where only the chunk walk can get it wrong: m = 1025 targets are three
    LDS chunks of 512, the last holding ONE real entry and 511 repeats of entry 0.  Chunk 1 repeats chunk 0 point for point and
    B[1024] = B[3], so every query has its minimum in two or three chunks: the first chunk must win, and inside it the lowest
    index.  All coordinates are multiples of 2^-10 below 1, so every squared distance (a multiple of 2^-20 below 4) is exact in
    float32: idx equals the float64 first minimum and dist its value, bit for bit."""
    k = torch.arange(512)
    first = torch.stack([k & 255, k >> 8, (k * 37) & 255], dim=1).double() / 256.0   # distinct: (x, y) determines k
    b = torch.cat([first, first, first[3:4]])
    assert b.shape[0] == 1025 and len({tuple(p) for p in first.tolist()}) == 512
    a = torch.stack([b[0], b[3], b[511], b[300] + torch.tensor([2.0 ** -10, 0.0, 0.0], dtype=torch.float64),
                     torch.tensor([0.9990234375, 0.5, 0.25], dtype=torch.float64)])
    best, want = U.nn_first(a, b)
    assert want[:4].tolist() == [0, 3, 511, 300] and int(want.max()) < 512         # the restatement itself
    dist, idx = search(a[None].float(), b[None].float(), planar=planar)
    print(f"planar={planar}: idx {idx[0].tolist()} (float64 first minimum {want.tolist()}), dist {dist[0].tolist()}")
    assert idx[0].tolist() == want.tolist()
    assert idx[0, :4].tolist() == [0, 3, 511, 300] and int(idx.max()) < 512
    assert torch.equal(dist[0], best.float()) and torch.equal(dist[0].double(), best)


def head_inputs(g, name, arch):
    """the forward pass's buffers as dg_head_post_fwd leaves them in eval mode, from the recorded step-0 head output"""
    params, gumbel, inv_ref, mask, latent0, noise, S = U.fixture_case(g, name)
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
    return inv_ref, gumbel.expand(B, 1, H, W).contiguous(), gout, m, depth


def run_head_grad(lidar, inv_ref, noise_pixel, gout, m, depth, arch_id, prior=None, prior_loss=None):
    """two calls of the scatter + gradient launches; prior: the head gradient and loss of an earlier term, added to (add = 1)"""
    from dusty_gan_amd import _lib as L
    lib, sp = L.lib(), L.stream_ptr()
    B, nh = gout.shape[:2]
    cp = 2 if nh <= 2 else 4
    dev = lambda t: t.to(DEV).float().contiguous()
    inv_ref, noise_pixel, gout, m, depth = map(dev, (inv_ref, noise_pixel, gout, m, depth))
    R = lidar.inv_to_xyz(inv_ref, tol=U.TOL)
    P = lidar.inv_to_xyz(depth, tol=U.TOL, from_tanh=True)
    angle = lidar.angle.reshape(2, HW).contiguous()
    d1, d2 = torch.empty(B, HW, device=DEV), torch.empty(B, HW, device=DEV)
    i1 = torch.empty(B, HW, dtype=torch.int32, device=DEV)
    i2 = torch.empty_like(i1)
    acc = torch.zeros(B, HW, 4, dtype=torch.int64, device=DEV)
    cloud = (3 * HW, 1, HW, HW)
    L.check(lib.dg_chamfer_nn(L.ptr(R), *cloud, L.ptr(P), *cloud, B, L.ptr(d1), L.ptr(i1), sp), "dg_chamfer_nn")
    L.check(lib.dg_chamfer_nn(L.ptr(P), *cloud, L.ptr(R), *cloud, B, L.ptr(d2), L.ptr(i2), sp), "dg_chamfer_nn")
    parts = torch.zeros(B * 2, device=DEV)
    tk = torch.zeros(B, dtype=torch.int32, device=DEV)
    s_depth = 1.0 / math.sqrt(16.0)
    s_conf = 1.0 / math.sqrt((nh - 1) * 16.0) if nh > 1 else 0.0
    res = []
    for _ in range(2):
        draw = torch.full((B, nh, H, W), float("nan"), device=DEV) if prior is None else prior.to(DEV).clone()
        pm = torch.full((B, H, W, cp), float("nan"), dtype=torch.bfloat16, device=DEV)
        loss = torch.full((B,), float("nan"), device=DEV) if prior is None else prior_loss.to(DEV).clone()
        L.check(lib.dg_inv_chamfer_scatter(L.ptr(R), L.ptr(i1), B, HW, L.ptr(acc), sp), "dg_inv_chamfer_scatter")
        assert int(acc[..., 3].sum()) == B * HW   # every target point counted once
        L.check(lib.dg_inv_chamfer_grad(L.ptr(P), L.ptr(R), L.ptr(d1), L.ptr(d2), L.ptr(i2), L.ptr(acc), L.ptr(depth),
                                        L.ptr(angle), L.ptr(gout), L.ptr(noise_pixel) if arch_id else None,
                                        L.ptr(m) if arch_id else None, arch_id, 1.0, -1.0, U.MIN_DEPTH, U.MAX_DEPTH, U.TOL, B, HW,
                                        s_depth, s_conf, int(prior is not None), L.ptr(draw), nh, L.ptr(pm), cp, L.ptr(parts), L.ptr(tk), 2,
                                        L.ptr(loss), sp), "dg_inv_chamfer_grad")
        assert int(acc.abs().sum()) == 0 and int(tk.abs().sum()) == 0 and float(parts.abs().sum()) == 0.0   # zero at rest
        res.append((draw.cpu(), pm.cpu(), loss.cpu()))
    return res, (s_depth, s_conf)


@pytest.mark.parametrize("arch", U.ARCHS)
def test_head_gradient_matches_float64(arch):
    g = load("chamfer_inversion")
    name = f"{arch}_chamfer"
    arch_id = U.ARCHS.index(arch)
    (first, second), (s_depth, s_conf) = run_head_grad(make_lidar(), *head_inputs(g, name, arch), arch_id)
    draw, pm, loss = first
    scale = torch.tensor([s_depth, s_conf, s_conf][:draw.shape[1]]).view(1, -1, 1, 1)
    want = torch.from_numpy(g[f"{name}/head/grad"]).double() * scale
    e_ref = torch.from_numpy(g[f"{name}/head/e_grad"]).double() * scale
    err = (draw.double() - want).abs()
    bound = 2 * e_ref + 1e-6 * float(want.abs().max())
    worst = float((err / bound).max())
    print(f"{arch}: head gradient max |err| {float(err.max()):.3g} (max |grad| {float(want.abs().max()):.3g}, max e_ref "
          f"{float(e_ref.max()):.3g}), worst err / bound {worst:.3g}, elements over {int((err > bound).sum())}")
    l64, e_l = torch.from_numpy(g[f"{name}/s0/loss"]), torch.from_numpy(g[f"{name}/s0/e_loss"]).double()
    print(f"{arch}: step-0 loss |err| {(loss.double() - l64).abs().tolist()} e_ref {e_l.tolist()}")
    assert bool((err <= bound).all())
    assert bool(((loss.double() - l64).abs() <= 2 * e_l + 1e-5 * l64.abs()).all())
    if arch == "dusty2":
        assert not bool(draw[:, 2].any())                                   # eval mode: the image-level mask is a threshold
    nh = draw.shape[1]
    assert torch.equal(pm[..., :nh], draw.permute(0, 2, 3, 1).to(torch.bfloat16))   # round to nearest even
    assert not bool(pm[..., nh:].any())
    for x, y in zip(first, second):                                         # a second call: identical bytes
        assert torch.equal(x, y)


def run_case(name, arch, distance, dtype=torch.float32):
    from dusty_gan_amd.inversion import invert
    g = load("chamfer_inversion")
    params, gumbel, inv_ref, mask, latent0, noise, S = U.fixture_case(g, name)
    G = make_G(arch, params, dtype=dtype)
    steps = []
    res = invert(G, inv_ref.to(DEV), mask.to(DEV), num_step=S, distance=distance[0] if len(distance) == 1 else distance,
                 latent=latent0, noise_fn=lambda k: noise[k], gumbel_noise=gumbel, lidar=make_lidar(), tol=U.TOL,
                 on_step=lambda k, loss, grad, lat: steps.append((loss.cpu(), grad.cpu(), lat.cpu())))
    return g, steps, res


@pytest.mark.parametrize("name,arch,distance", U.CASES)
def test_fp32_steps_match_float64(name, arch, distance):
    """Per step, against the reference's float64 run: loss, d loss / d latent and the latent within 2 e_ref plus the fp32
    engine's documented generator error of that tensor class, the bounds of tests/test_gpu_inversion.py as additive floors:
    1e-5 of the loss, 1e-4 of the sample's largest gradient component, 1e-4 absolute on the latent."""
    g, steps, res = run_case(name, arch, distance)
    ok = True
    for k, (loss, grad, lat) in enumerate(steps):
        rows = []
        for key, got, floor in (("loss", loss, None), ("grad", grad, None), ("latent", lat, None)):
            w = torch.from_numpy(g[f"{name}/s{k}/{key}"])
            e = torch.from_numpy(g[f"{name}/s{k}/e_{key}"]).double()
            if key == "loss":
                floor = 1e-5 * w.abs()
            elif key == "grad":
                floor = 1e-4 * w.abs().max(dim=1, keepdim=True).values
            else:
                floor = torch.full_like(w, 1e-4)
            err = (got.double() - w).abs()
            bound = 2 * e + floor
            rows.append(f"{key} err {float(err.max()):.3g} e_ref {float(e.max()):.3g} err/bound {float((err / bound).max()):.3g}")
            ok = ok and bool((err <= bound).all())
        print(f"{name} step {k}: " + "; ".join(rows))
    assert ok
    assert torch.equal(res["latent"].cpu(), steps[-1][2]) and torch.equal(res["loss"].cpu(), steps[-1][0])


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
def test_deterministic_and_graph_equals_eager(dtype):
    from dusty_gan_amd.inversion import invert
    g = load("chamfer_inversion")
    params, gumbel, inv_ref, mask, latent0, noise, S = U.fixture_case(g, "dusty2_chamfer")
    G = make_G("dusty2", params, dtype=dtype)
    kw = dict(num_step=8, seed=5, gumbel_noise=gumbel, distance="chamfer", lidar=make_lidar())
    a = invert(G, inv_ref.to(DEV), mask.to(DEV), graph=True, **kw)
    b = invert(G, inv_ref.to(DEV), mask.to(DEV), graph=True, **kw)
    c = invert(G, inv_ref.to(DEV), mask.to(DEV), graph=False, **kw)
    for k in ("latent", "loss"):
        assert bool(torch.isfinite(a[k]).all()), k
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    # sums of terms, in their fixed order (bf16: the planar fp32 sum, its pixel-major bf16 copy written by the last term)
    for distance in (("l1", "chamfer"), ("l1", "l2")):
        kw["distance"] = distance
        a = invert(G, inv_ref.to(DEV), mask.to(DEV), graph=True, **kw)
        b = invert(G, inv_ref.to(DEV), mask.to(DEV), graph=True, **kw)
        c = invert(G, inv_ref.to(DEV), mask.to(DEV), graph=False, **kw)
        for k in ("latent", "loss"):
            assert bool(torch.isfinite(a[k]).all()), (distance, k)
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), (distance, k)


@pytest.mark.parametrize("arch", U.ARCHS)
def test_added_head_gradient_and_its_bf16_copy(arch):
    """add = 1 (a further term: what a bf16 generator's ("l1", "chamfer") step runs last): the planar gradient is the earlier
    term's plus this one's, and the pixel-major bf16 copy is that SUM rounded to bf16, exactly.  The sum may be formed with a
    fused multiply-add (the unrounded scaled gradient plus the prior), so it equals prior + gradient to half an ulp of the
    gradient plus one ulp of the sum: 2^-24 |grad| + 2^-23 |sum|."""
    g = load("chamfer_inversion")
    name = f"{arch}_chamfer"
    arch_id = U.ARCHS.index(arch)
    inputs = head_inputs(g, name, arch)
    (alone, _), _ = run_head_grad(make_lidar(), *inputs, arch_id)
    gen = torch.Generator().manual_seed(8)
    prior = torch.randn(alone[0].shape, generator=gen) * float(alone[0].abs().max())
    prior_loss = torch.rand(alone[2].shape, generator=gen)
    (added, again), _ = run_head_grad(make_lidar(), *inputs, arch_id, prior=prior, prior_loss=prior_loss)
    draw, pm, loss = added
    want = prior + alone[0]
    err = (draw.double() - want.double()).abs()
    assert bool((err <= 2.0 ** -24 * alone[0].abs().double() + 2.0 ** -23 * want.abs().double()).all())
    assert torch.equal(loss, prior_loss + alone[2])
    nh = draw.shape[1]
    assert torch.equal(pm[..., :nh], draw.permute(0, 2, 3, 1).to(torch.bfloat16)) and not bool(pm[..., nh:].any())
    for x, y in zip(added, again):
        assert torch.equal(x, y)


def test_sum_of_terms_adds_the_gradients():
    """fp32, one step of ("l1", "chamfer") against the two single-term steps from the same latent: the loss is the sum of the
    two losses and d loss / d latent the sum of the two gradients (the backward chain is linear in the head gradient), to
    fp32 rounding of the chain: 1e-5 of the largest component, the generator's documented fp32 error class"""
    from dusty_gan_amd.inversion import invert
    g = load("chamfer_inversion")
    params, gumbel, inv_ref, mask, latent0, noise, S = U.fixture_case(g, "dusty2_chamfer")
    G = make_G("dusty2", params)
    got = {}
    for distance in ("l1", "chamfer", ("l1", "chamfer")):
        steps = []
        invert(G, inv_ref.to(DEV), mask.to(DEV), num_step=1, distance=distance, latent=latent0, gumbel_noise=gumbel,
               perturb_latent=False, lidar=make_lidar(),
               on_step=lambda k, loss, grad, lat: steps.append((loss.cpu().double(), grad.cpu().double())))
        got[distance] = steps[0]
    loss, grad = got[("l1", "chamfer")]
    want_l, want_g = got["l1"][0] + got["chamfer"][0], got["l1"][1] + got["chamfer"][1]
    err = float((grad - want_g).abs().max() / want_g.abs().max())
    print(f"summed-terms gradient off the sum of gradients by {err:.3g} of max, loss by "
          f"{float(((loss - want_l).abs() / want_l).max()):.3g}")
    assert float(((loss - want_l).abs() / want_l).max()) <= 1e-6
    assert err <= 1e-5


def l1_run():
    from dusty_gan_amd.inversion import invert
    g = load("chamfer_inversion")
    params, gumbel, inv_ref, mask, latent0, noise, S = U.fixture_case(g, "dusty2_chamfer")
    G = make_G("dusty2", params)
    kw = dict(num_step=8, seed=2, gumbel_noise=gumbel)
    run = lambda **more: invert(G, inv_ref.to(DEV), mask.to(DEV), **kw, **more)
    return run, {k: v.cpu() for k, v in run(distance="l1").items() if k in ("latent", "loss", "inv_gen")}


def l1_baseline(path):
    """(child process) distance="l1" in a process in which no Chamfer inversion ever ran"""
    torch.save(l1_run()[1], path)


def test_l1_is_untouched_by_a_chamfer_inversion(tmp_path):
    """distance="l1" after Chamfer inversions in this process equals, bit for bit, the same call made in a fresh process
    that never ran one: the new branch leaves no state behind (engine buffers, workspaces, library-side statics)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "l1_baseline.pt")
    subprocess.run([sys.executable, "-c", f"from tests.test_gpu_chamfer_inversion import l1_baseline; l1_baseline({path!r})"],
                   cwd=root, check=True, timeout=300)
    pristine = torch.load(path)
    run, _ = l1_run()
    run(distance=("l2", "chamfer"), lidar=make_lidar())
    run(distance="chamfer", lidar=make_lidar())
    after = run(distance="l1")
    for k in ("latent", "loss", "inv_gen"):
        assert torch.equal(pristine[k], after[k].cpu()), k
