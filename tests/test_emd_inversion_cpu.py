"""The earth mover's term of the GAN inversion, on the CPU: the argument checks of dusty_gan_amd.inversion.invert and of the
commands, which come before any launch; the restated EarthMoverDistanceFunction (tests/emd_inv_util.EmdFn) against float64
finite differences; the conditions tests/golden/emd_inversion.npz was made under, re-checked from its contents; and the two
new C entries' argument refusals, which need no device."""
import numpy as np
import pytest
import torch

from tests import emd_grad_util as EU
from tests import emd_inv_util as U
from tests.golden_util import load


def nominal_lidar():
    from dusty_gan_amd.utils.lidar import LiDAR
    return LiDAR(32, 64, 0.9, 120.0).use_nominal_angles()


def test_check_distance_takes_emd_in_the_fixed_order():
    from dusty_gan_amd.inversion import DISTANCES, check_distance
    lidar = nominal_lidar()
    assert DISTANCES == ("l1", "l2", "chamfer", "emd")
    assert check_distance("emd", lidar) == ("emd",)
    assert check_distance(("emd", "l1"), lidar) == ("l1", "emd")
    assert check_distance(("emd", "chamfer", "l2"), lidar) == ("l2", "chamfer", "emd")


def test_emd_needs_a_lidar_with_an_angle_grid():
    from dusty_gan_amd.inversion import check_distance, invert
    from dusty_gan_amd.utils.lidar import LiDAR
    x = torch.zeros(1, 1, 32, 64)
    with pytest.raises(ValueError):
        check_distance("emd")
    with pytest.raises(ValueError):
        invert(None, x, x, distance="emd")
    with pytest.raises(ValueError):
        invert(None, x, x, distance=("l1", "emd"), lidar=LiDAR(32, 64, 0.9, 120.0))   # no angle grid


@pytest.mark.parametrize("K", (0, 3201, 32 * 64 + 1))
def test_emd_points_out_of_range_is_refused_before_the_device_check(K):
    from dusty_gan_amd.inversion import invert
    x = torch.zeros(1, 1, 32, 64)   # a CPU tensor: the argument errors come before the GPU-only one (a RuntimeError)
    with pytest.raises(ValueError):
        invert(None, x, x, distance="emd", lidar=nominal_lidar(), emd_points=K)
    with pytest.raises(ValueError):
        invert(None, x, x, distance=("l1", "emd"), lidar=nominal_lidar(), emd_points=K)
    with pytest.raises(RuntimeError):   # not looked at without "emd"
        invert(None, x, x, distance="l1", emd_points=K)


@pytest.mark.parametrize("command", ("evaluate_reconstruction", "reconstruct", "transfer_raydrop"))
def test_commands_take_emd_and_emd_points(command, tmp_path):
    import importlib

    from dusty_gan_amd.utils.config import dump_config, load_config
    mod = importlib.import_module(f"dusty_gan_amd.{command}")
    cfg = str(tmp_path / "dusty1.yaml")   # (transfer_raydrop reads the generator's arch while it parses)
    dump_config(load_config(["model=dusty1_dcgan_eqlr", "dataset=synthetic", "dataset.shape=[64,1024]"]), cfg)
    base = ["--model-path", str(tmp_path / "g.pth"), "--config-path", cfg]
    if command != "evaluate_reconstruction":   # the two commands on point clouds name their files
        np.zeros((5, 4), np.float32).tofile(tmp_path / "a.bin")
        base += ["--points", str(tmp_path / "a.bin")]
    plain = mod.parse_args(base)
    assert plain.distance == "l1" and plain.emd_points == 2048
    assert mod.parse_args(base + ["--distance", "emd"]).distance == "emd"
    got = mod.parse_args(base + ["--distance", "l1+emd", "--emd-points", "512"])
    assert got.distance == "l1+emd" and got.emd_points == 512
    for bad in (["--emd-points", "0"], ["--distance", "l1+emd+"], ["--emd-points", "3201"]):
        with pytest.raises(SystemExit):
            mod.parse_args(base + bad)


def small_pair(seed=3, n=12):
    gen = torch.Generator().manual_seed(seed)
    a = torch.rand(2, n, 3, generator=gen, dtype=torch.float64) * 0.2
    b = torch.rand(2, n, 3, generator=gen, dtype=torch.float64) * 0.2
    return a, b


def test_restated_function_is_quadratic_with_the_match_frozen():
    a, b = small_pair()
    match = EU.approxmatch(a.numpy(), b.numpy(), np.float64)[0]
    U.EmdFn.frozen = match
    try:
        f = lambda x: U.EmdFn.apply(x, b).sum()
        gen = torch.Generator().manual_seed(5)
        d = torch.randn(a.shape, generator=gen, dtype=torch.float64) * 1e-2
        # a quadratic's third difference vanishes: f(x + 2d) - 3 f(x + d) + 3 f(x) - f(x - d) = 0
        third = float(f(a + 2 * d) - 3 * f(a + d) + 3 * f(a) - f(a - d))
        second = float(f(a + d) - 2 * f(a) + f(a - d))
        assert second > 0 and abs(third) <= 1e-12 * max(1.0, abs(float(f(a))))
    finally:
        U.EmdFn.frozen = None


def test_restated_backward_matches_finite_differences():
    a, b = small_pair()
    match = EU.approxmatch(a.numpy(), b.numpy(), np.float64)[0]
    U.EmdFn.frozen = match
    try:
        w = torch.tensor([1.0, 0.7], dtype=torch.float64)
        loss = lambda x, y: (U.EmdFn.apply(x, y) * w).sum()
        x, y = a.clone().requires_grad_(), b.clone().requires_grad_()
        loss(x, y).backward()
        h = 1e-4   # (the loss is quadratic: central differences are exact up to rounding)
        for t, grad, first in ((a, x.grad, True), (b, y.grad, False)):
            for i in range(2):
                for p in range(t.shape[1]):
                    for c in range(3):
                        e = torch.zeros_like(t)
                        e[i, p, c] = h
                        hi = loss(t + e, b) if first else loss(a, t + e)
                        lo = loss(t - e, b) if first else loss(a, t - e)
                        assert abs(float(hi - lo) / (2 * h) - float(grad[i, p, c])) <= 1e-8, (first, i, p, c)
    finally:
        U.EmdFn.frozen = None
    # and without the frozen match the saved one is approxmatch's: the same gradient
    x2 = a.clone().requires_grad_()
    (U.EmdFn.apply(x2, b) * w).sum().backward()
    assert torch.equal(x2.grad, x.grad)


@pytest.mark.parametrize("name,arch,distance,K,inputs,max_depth", U.CASES)
def test_fixture_conditions_hold(name, arch, distance, K, inputs, max_depth):
    from oracle import metrics_oracle as MO
    g, gc = load("emd_inversion"), load("chamfer_inversion")
    params, gumbel, inv_ref, mask, latent0, noise, S, idx, md = U.fixture_case(g, gc, name)
    assert md == max_depth and S == 6 and inv_ref.shape == (3, 1, 32, 64) and idx.shape == (3, K) and int(g[f"{name}/meta/K"]) == K
    assert str(g[f"{name}/meta/distance"]) == "+".join(distance)
    assert torch.equal(mask, (inv_ref > 0).float())
    p32, p64 = U.target_points(inv_ref, max_depth=md), U.target_points(inv_ref, torch.float64, md)
    assert bool((torch.from_numpy(U.candidates(p32)) >= K).all())
    assert float(p32[0, 0].abs().max()) == 0.0 and float(p32[1, 0].abs().max()) > 0.0   # pixel 0: dropped in scan 0, kept in scan 1
    for b in range(3):
        want = MO.fps(p32[b].numpy(), K).astype(np.int64)
        assert np.array_equal(idx[b].numpy(), want)                   # the oracle's sample of the stored target
        assert len(set(want.tolist())) == K and want[0] == 0         # distinct, and sample 0 is pixel 0
        again, gap = U.fps_margin(p64[b].numpy(), p32[b].numpy(), K)
        assert np.array_equal(again, want) and gap > U.FPS_MARGIN     # no decision within the margin
    assert float(g[f"{name}/meta/e_ref_rel"]) <= 1e-3
    for k in range(S):
        for key in ("loss", "grad", "latent"):
            assert g[f"{name}/s{k}/{key}"].dtype.name == "float64"
            assert g[f"{name}/s{k}/e_{key}"].shape == g[f"{name}/s{k}/{key}"].shape
    if distance == ("emd",):
        heads = 1 + ("none", "dusty1", "dusty2").index(arch)
        assert g[f"{name}/head/raw"].shape == g[f"{name}/head/grad"].shape == (3, heads, 32, 64)
        grad = torch.from_numpy(g[f"{name}/head/grad"]).flatten(2)
        off = torch.ones(3, 32 * 64, dtype=torch.bool).scatter_(1, idx, False)
        assert not bool(grad.permute(0, 2, 1)[off].any())             # the gradient lives on the sampled rays
        if arch == "dusty2":
            assert not g[f"{name}/head/grad"][:, 2].any()             # eval mode: the image-level mask is a plain threshold


def test_new_entries_refuse_bad_arguments_without_a_device():
    from dusty_gan_amd import _lib as L
    lib = L.lib()
    x = torch.zeros(16)
    i = torch.zeros(16, dtype=torch.int32)
    px, pi = L.ptr(x), L.ptr(i)
    assert lib.dg_points_gather(None, 6, 3, 1, 2, pi, 1, 2, px, None) == L.DG_EINVAL
    assert lib.dg_points_gather(px, 6, 3, 1, 2, None, 1, 2, px, None) == L.DG_EINVAL
    assert lib.dg_points_gather(px, 6, 3, 1, 2, pi, 1, 2, None, None) == L.DG_EINVAL
    for n, B, K in ((0, 1, 2), (2, 0, 2), (2, 1, 0), (-1, 1, 2)):
        assert lib.dg_points_gather(px, 6, 3, 1, n, pi, B, K, px, None) == L.DG_EINVAL
    assert lib.dg_points_gather(px, 6, 0, 1, 2, pi, 1, 2, px, None) == L.DG_EINVAL

    def grad(gP=px, slot=pi, term=px, K=2, depth=px, angle=px, gout=px, arch=0, tau=1.0, mn=0.9, mx=120.0, B=1, HW=4, add=0,
             draw=px, nheads=1, draw_pm=None, cp=2, nchunk=1, loss=px, noise=None, mask=None):
        return lib.dg_inv_points_grad(gP, slot, term, 0.5, K, depth, angle, gout, noise, mask, arch, tau, -1.0, mn, mx, 1e-8, B, HW,
                                      1.0, 1.0, add, draw, nheads, draw_pm, cp, nchunk, loss, None)

    for bad in (dict(gP=None), dict(slot=None), dict(term=None), dict(depth=None), dict(angle=None), dict(gout=None),
                dict(loss=None), dict(K=0), dict(B=0), dict(HW=0), dict(B=-1), dict(arch=3), dict(arch=1, nheads=2),
                dict(nheads=2), dict(tau=0.0), dict(mn=0.0), dict(mn=120.0), dict(draw=None), dict(add=1, draw=None, draw_pm=px),
                dict(draw_pm=px, cp=0), dict(nchunk=0), dict(nchunk=65536)):
        assert grad(**bad) == L.DG_EINVAL, bad
