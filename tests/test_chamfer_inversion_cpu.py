"""The Chamfer term of the GAN inversion, on the CPU: the invariants tests/golden/chamfer_inversion.npz was made under
(tests/golden/make_chamfer_inversion_golden.py), the restated backward of the reference's Chamfer extension
(tests/chamfer_inv_util.ChamferFn, chamfer_distance.cpp:82-140) against float64 finite differences, and the argument checks
of dusty_gan_amd.inversion.invert, which come before any launch."""
import pytest
import torch

from tests import chamfer_inv_util as U
from tests.golden_util import load

MARGIN = 1.0 + 2.0 ** -18


@pytest.mark.parametrize("name", U.PAIR_NAMES)
def test_fixture_pairs_keep_their_margin_and_first_index(name):
    g = load("chamfer_inversion")
    a, b = U.pair(name, int(g["meta/pair_seed"]))
    idx = torch.from_numpy(g[f"pairs/{name}/idx"]).long()
    d = U.sqdist(a.double(), b.double())
    best = d.min(dim=1).values
    assert torch.equal(d[torch.arange(len(idx)), idx], best)           # a minimum ...
    before = torch.arange(b.shape[0])[None, :] < idx[:, None]
    assert not bool(((d == best[:, None]) & before).any())               # ... and the FIRST one
    if name == U.DYADIC[0]:
        assert int(((d == best[:, None]).sum(dim=1) > 1).sum()) > len(idx) // 2   # ties are what this pair is about
        assert torch.equal(d.float().double(), d)                                 # every distance exact in float32
    else:
        assert float(U.runner_up_ratio(a, b).min()) > MARGIN


def test_fixture_records_every_case():
    g = load("chamfer_inversion")
    for name, arch, distance in U.CASES:
        params, gumbel, inv_ref, mask, latent0, noise, S = U.fixture_case(g, name)
        assert S == 6 and inv_ref.shape == (3, 1, 32, 64) and noise.shape == (6, 3, 8) and latent0.shape == (3, 8)
        assert bool(((mask == 0) | (mask == 1)).all()) and float((inv_ref * (1 - mask)).abs().max()) == 0.0
        assert str(g[f"{name}/meta/distance"]) == "+".join(distance)
        for k in range(S):
            for key in ("loss", "grad", "latent"):
                assert g[f"{name}/s{k}/{key}"].dtype.name == "float64"
                assert g[f"{name}/s{k}/e_{key}"].shape == g[f"{name}/s{k}/{key}"].shape
        if distance == ("chamfer",):
            heads = 1 + U.ARCHS.index(arch)
            assert g[f"{name}/head/raw"].shape == g[f"{name}/head/grad"].shape == (3, heads, 32, 64)
            if arch == "dusty2":
                assert not g[f"{name}/head/grad"][:, 2].any()   # eval mode: the image-level mask is a plain threshold


def test_restated_backward_matches_finite_differences():
    gen = torch.Generator().manual_seed(4)
    a = torch.rand(1, 16, 3, generator=gen, dtype=torch.float64)
    b = torch.rand(1, 16, 3, generator=gen, dtype=torch.float64)

    def loss(x, y):
        d1, d2 = U.ChamferFn.apply(x, y)
        return d1.mean() + 0.7 * d2.mean()

    x, y = a.clone().requires_grad_(), b.clone().requires_grad_()
    loss(x, y).backward()
    h = 1e-6   # far inside the margin of any match of these 16 points: the matches do not move
    for t, grad, other, first in ((a, x.grad, b, True), (b, y.grad, a, False)):
        for p in range(16):
            for c in range(3):
                e = torch.zeros_like(t)
                e[0, p, c] = h
                hi = loss(t + e, other) if first else loss(other, t + e)
                lo = loss(t - e, other) if first else loss(other, t - e)
                fd = float(hi - lo) / (2 * h)
                assert abs(fd - float(grad[0, p, c])) <= 1e-8, (first, p, c)   # (the loss is quadratic: central differences are exact)


def test_invert_checks_its_distance_before_any_launch():
    from dusty_gan_amd.inversion import check_distance, invert
    from dusty_gan_amd.utils.lidar import LiDAR
    x = torch.zeros(1, 1, 32, 64)   # a CPU tensor: the argument errors come before the GPU-only one
    with pytest.raises(ValueError):
        invert(None, x, x, distance="chamfer")
    with pytest.raises(ValueError):
        invert(None, x, x, distance=("l1", "chamfer"))
    with pytest.raises(ValueError):
        invert(None, x, x, distance=())
    with pytest.raises(ValueError):
        invert(None, x, x, distance="chamfer", lidar=LiDAR(32, 64, 0.9, 120.0))   # no angle grid
    with pytest.raises(NotImplementedError):
        invert(None, x, x, distance="l3")
    lidar = LiDAR(32, 64, 0.9, 120.0).use_nominal_angles()
    assert check_distance(("chamfer", "l1"), lidar) == ("l1", "chamfer")
    assert check_distance("l2") == ("l2",) and check_distance(["l2", "l1", "l2"]) == ("l1", "l2")


def test_cli_takes_chamfer_and_combinations():
    from dusty_gan_amd import evaluate_reconstruction as E
    base = ["--model-path", "m.pth", "--config-path", "c.yaml"]
    assert E.parse_args(base).distance == "l1"
    assert E.parse_args(base + ["--distance", "chamfer"]).distance == "chamfer"
    assert E.parse_args(base + ["--distance", "l1+chamfer"]).distance == "l1+chamfer"
    assert E.split_distance("l1+chamfer") == ("l1", "chamfer") and E.split_distance("l2") == ("l2",)
    for bad in ("l3", "l1+", "+", "l1+l3"):
        with pytest.raises(SystemExit):
            E.parse_args(base + ["--distance", bad])
