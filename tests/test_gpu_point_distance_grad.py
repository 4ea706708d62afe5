"""GPU tests of the differentiable point-set distances: dg_emd_grad and dg_chamfer_backward (csrc/point_emd.hip, csrc/point_chamfer.hip) through
dusty_gan_amd.utils.metrics, against tests/golden/emd_grad.npz and the float64 restatements of tests/emd_grad_util.py."""
import numpy as np
import pytest
import torch

from tests import emd_grad_util as U
from tests.golden_util import load

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ---------------------------------------------------------------------------------------------------------- EMD
@pytest.fixture(scope="module")
def emd_runs():
    """per fixture case: the clouds on the device and TWO dg_emd_grad launches (cost, grad1, grad2), computed once"""
    from dusty_gan_amd.utils.metrics import earth_mover_distance_grad
    g = load("fps_emd")
    runs = {}
    for name in U.EMD_GRAD_CASES:
        a, b = dev(g[f"emd/{name}/a"]), dev(g[f"emd/{name}/b"])
        runs[name] = (a, b, earth_mover_distance_grad(a, b), earth_mover_distance_grad(a, b))
    return runs


def test_emd_grad_matches_the_fixture(emd_runs):
    """per pair and per gradient max |got - f64| <= 4 e_ref + 1e-6 max|g_f64|, e_ref being the reference's own distance from
    the float64 algorithm (its kernel's match matrix where the fixture was recorded live, the float32-order restatement
    otherwise).  4, where the cost is held to 2 e_ref: a gradient row is one row or column of `match`, not the whole sum, so
    the errors of two float32 orders cancel less."""
    g = load("emd_grad")
    bad = []
    for name, (a, b, (_, g1, g2), _) in emd_runs.items():
        worst = 0.0
        for k, got in ((1, g1), (2, g2)):
            want, e_ref = g[f"{name}/g{k}_f64"], g[f"{name}/e_ref{k}"]
            err = np.abs(got.cpu().numpy().astype(np.float64) - want).max((1, 2))
            bound = 4.0 * e_ref + 1e-6 * np.abs(want).max((1, 2))
            ratio = err / np.maximum(bound, 1e-300)
            worst = max(worst, float(ratio.max()))
            for i in np.flatnonzero(~(err <= bound)):
                bad.append((name, k, int(i), float(err[i]), float(bound[i])))
        print(name, "largest got / bound", worst)
    assert not bad, bad


def test_emd_grad_cost_is_dg_emds(emd_runs):
    from dusty_gan_amd.utils.metrics import earth_mover_distance
    for name, (a, b, (cost, _, _), _) in emd_runs.items():
        assert torch.equal(cost, earth_mover_distance(a, b)), name


def test_emd_grad_two_launches_are_bit_identical(emd_runs):
    for name, (_, _, r1, r2) in emd_runs.items():
        for x, y in zip(r1, r2):
            assert torch.equal(x, y), name


def test_emd_grad_cost_scale_is_applied_after_the_sum(emd_runs):
    from dusty_gan_amd.utils.metrics import earth_mover_distance_grad
    for name in ("p64_64", "p50_150", "b35_8_8"):
        a, b, (cost, g1, g2), _ = emd_runs[name]
        c2, h1, h2 = earth_mover_distance_grad(a, b, torch.full((a.size(0),), 2.0, device=DEV))
        assert torch.equal(c2, cost) and torch.equal(h1, 2.0 * g1) and torch.equal(h2, 2.0 * g2), name
    a, b, (_, g1, g2), _ = emd_runs["p4_4"]
    _, h1, h2 = earth_mover_distance_grad(a, b, torch.tensor([0.0, -1.0], device=DEV))   # per pair
    assert not h1[0].any() and not h2[0].any() and torch.equal(h1[1], -g1[1]) and torch.equal(h2[1], -g2[1])


def test_emd_autograd(emd_runs):
    from dusty_gan_amd import _lib as L
    from dusty_gan_amd.utils.metrics import EarthMoverDistance, earth_mover_distance
    for name in ("p96_32", "p100_30"):
        a, b, (cost, g1, g2), _ = emd_runs[name]
        x1, x2 = a.clone().requires_grad_(), b.clone().requires_grad_()
        c = earth_mover_distance(x1, x2)
        assert c.requires_grad and torch.equal(c.detach(), cost)
        c.sum().backward()
        assert torch.equal(x1.grad, g1) and torch.equal(x2.grad, g2), name
        x1 = a.clone().requires_grad_()
        EarthMoverDistance()(x1, b, 0.005, 50).sum().backward()      # eps, iters: ignored, as in the reference
        assert torch.equal(x1.grad, g1), name
        # without a gradient to record: dg_emd itself, the bits of the launch the function made before it was differentiable
        plain = earth_mover_distance(a, b)
        out = torch.empty_like(cost)
        L.check(L.lib().dg_emd(L.ptr(a), a.size(0), a.size(1), L.ptr(b), b.size(0), b.size(1), 1, L.ptr(out), L.stream_ptr()))
        assert not plain.requires_grad and torch.equal(plain, out), name
        with torch.no_grad():
            assert not earth_mover_distance(a.clone().requires_grad_(), b).requires_grad


def test_emd_gradient_descends(emd_runs):
    """ten steps of A <- A - 0.25 grad1 on p64_64, pair 0: the cost must end below a quarter of its start (the float64
    restatement alone: 6.086 -> 0.707, a factor of 0.116)"""
    from dusty_gan_amd.utils.metrics import earth_mover_distance, earth_mover_distance_grad
    a, b = emd_runs["p64_64"][0][:1].clone(), emd_runs["p64_64"][1][:1]
    start = float(earth_mover_distance(a, b))
    for _ in range(10):
        a = a - 0.25 * earth_mover_distance_grad(a, b)[1]
    end = float(earth_mover_distance(a, b))
    print("cost", start, "->", end, "factor", end / start)
    assert end < 0.25 * start, (start, end)


def test_emd_grad_refuses_clouds_above_the_lds_cap():
    from dusty_gan_amd import _lib as L
    from dusty_gan_amd.utils.metrics import earth_mover_distance_grad
    a, b = torch.zeros(1, 3201, 3, device=DEV), torch.zeros(1, 3200, 3, device=DEV)
    with pytest.raises(L.DgError, match="DG_EUNSUPPORTED"):
        earth_mover_distance_grad(a, b)
    cost, g1, g2 = torch.full((1,), 7.0, device=DEV), torch.full_like(a, 7.0), torch.full_like(b, 7.0)
    rc = L.lib().dg_emd_grad(L.ptr(a), 3201, L.ptr(b), 3200, 1, None, L.ptr(cost), L.ptr(g1), L.ptr(g2), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == L.DG_EUNSUPPORTED and bool((cost == 7).all()) and bool((g1 == 7).all()) and bool((g2 == 7).all())
    assert earth_mover_distance_grad(a[:, :3200], b)[1].shape == (1, 3200, 3)    # n + m = 6400: the cap itself runs


# ---------------------------------------------------------------------------------------------------------- Chamfer
def chamfer_clouds(n, m, B=2):
    rng = np.random.default_rng(1000 * n + m)
    return (rng.uniform(-1, 1, (B, n, 3)).astype(np.float32), rng.uniform(-1, 1, (B, m, 3)).astype(np.float32))


def lattice_clouds():
    """a 4x4x4 lattice (cell 1/4, exact in float32) against itself shifted by half a cell: every inner shifted point has eight
    nearest corners at exactly the same distance"""
    ax = np.arange(4, dtype=np.float32) * np.float32(0.25) - np.float32(0.5)
    a = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(1, 64, 3)
    return a, a + np.float32(0.125)


def nn(a, b):
    from dusty_gan_amd.utils.metrics.distance import _chamfer_nn
    return _chamfer_nn(a, b)


def check_chamfer_grads(a, b, g1, g2, idx1, idx2, grad1, grad2, what):
    w1, w2, abs1, abs2, cnt1, cnt2 = U.chamfer_backward_f64(a, b, g1, g2, idx1, idx2)
    for k, (got, want, ab, cnt) in enumerate(((grad1, w1, abs1, cnt1), (grad2, w2, abs2, cnt2)), 1):
        err = np.abs(got.astype(np.float64) - want)
        bound = U.chamfer_bound(ab, cnt)
        print(what, f"grad{k}", "largest err / bound", float((err / np.maximum(bound, 1e-300)).max()), "max terms per point",
              int(cnt.max()))
        assert np.all(err <= bound), (what, k, float((err - bound).max()))


@pytest.mark.parametrize("n,m", [(1, 1), (7, 5), (64, 64), (513, 300), (1030, 520), (600, 3), (300, 1), ("lattice", "lattice")])
def test_chamfer_backward(n, m):
    """indices from dg_chamfer_nn, expected gradients from the float64 restatement with those indices; per entry
    |err| <= 2^-21 sum |terms| + 2^-39 count (tests/emd_grad_util.chamfer_bound); two launches bit-identical; the scatter
    words zero afterwards"""
    from dusty_gan_amd.utils.metrics import chamfer_backward
    from dusty_gan_amd.utils.metrics import distance as D
    a, b = lattice_clouds() if n == "lattice" else chamfer_clouds(n, m)
    rng = np.random.default_rng(5)
    g1 = (rng.normal(size=a.shape[:2]) / a.shape[1]).astype(np.float32)    # what a mean over the points hands down, signed
    g2 = (rng.normal(size=b.shape[:2]) / b.shape[1]).astype(np.float32)
    ta, tb, tg1, tg2 = dev(a), dev(b), dev(g1), dev(g2)
    (_, idx1), (_, idx2) = nn(ta, tb), nn(tb, ta)
    if n == "lattice":   # exact arithmetic, exact ties: the lowest index wins
        d = ((a[0].astype(np.float64)[:, None] - b[0].astype(np.float64)[None]) ** 2).sum(-1)
        assert (d == d.min(1, keepdims=True)).sum(1).max() == 8
        assert np.array_equal(idx1[0].cpu().numpy(), d.argmin(1)) and np.array_equal(idx2[0].cpu().numpy(), d.argmin(0))
    r1 = chamfer_backward(ta, tb, tg1, tg2, idx1, idx2)
    r2 = chamfer_backward(ta, tb, tg1, tg2, idx1, idx2)
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])
    acc = D._CHAMFER_ACC[torch.cuda.current_device()]
    assert acc.numel() >= a.shape[0] * (a.shape[1] + b.shape[1]) * 4 and not bool(acc.any())
    check_chamfer_grads(a, b, g1, g2, idx1.cpu().numpy(), idx2.cpu().numpy(), r1[0].cpu().numpy(), r1[1].cpu().numpy(), (n, m))


def test_chamfer_backward_skips_indices_outside_the_cloud_and_poisons_what_does_not_fit():
    from dusty_gan_amd.utils.metrics import chamfer_backward
    from dusty_gan_amd.utils.metrics import distance as D
    a, b = chamfer_clouds(7, 5, B=1)
    ta, tb = dev(a), dev(b)
    idx1 = torch.tensor([[0, 1, 5, -1, 2, 2, 4]], dtype=torch.int32, device=DEV)   # 5 and -1: outside cloud 2
    idx2 = torch.tensor([[0, 6, 7, 3, 3]], dtype=torch.int32, device=DEV)          # 7: outside cloud 1
    g1, g2 = torch.ones(1, 7, device=DEV), torch.ones(1, 5, device=DEV)
    grad1, grad2 = chamfer_backward(ta, tb, g1, g2, idx1, idx2)
    k1, k2 = idx1.cpu().numpy(), idx2.cpu().numpy()
    ok1, ok2 = (k1 >= 0) & (k1 < 5), (k2 >= 0) & (k2 < 7)
    w1, w2, abs1, abs2, cnt1, cnt2 = U.chamfer_backward_f64(a, b, np.where(ok1, 1.0, 0.0), np.where(ok2, 1.0, 0.0),
                                                            np.where(ok1, k1, 0), np.where(ok2, k2, 0))
    assert np.all(np.abs(grad1.cpu().numpy() - w1) <= U.chamfer_bound(abs1, cnt1))
    assert np.all(np.abs(grad2.cpu().numpy() - w2) <= U.chamfer_bound(abs2, cnt2))
    g1[0, 1] = float("inf")                       # point 1 of cloud 1 -> its own row and its neighbour's (point 1 of cloud 2)
    grad1, grad2 = chamfer_backward(ta, tb, g1, g2, idx1, idx2)
    assert not torch.isfinite(grad1[0, 1]).any() and torch.isnan(grad2[0, 1]).all()
    assert torch.isfinite(grad2[0, [0, 2, 3, 4]]).all() and torch.isfinite(grad1[0, [0, 2, 4, 5]]).all()
    assert not bool(D._CHAMFER_ACC[torch.cuda.current_device()].any())


@pytest.mark.parametrize("n,m", [(513, 300), (64, 64)])
def test_chamfer_autograd(n, m):
    from dusty_gan_amd.utils.metrics import ChamferDistance, chamfer_distance, chamfer_paired
    a, b = chamfer_clouds(n, m)
    x1, x2 = dev(a).requires_grad_(), dev(b).requires_grad_()
    d1, d2 = chamfer_distance(x1, x2)
    (n1, idx1), (n2, idx2) = nn(x1.detach(), x2.detach()), nn(x2.detach(), x1.detach())
    assert torch.equal(d1.detach(), n1) and torch.equal(d2.detach(), n2)
    for mean, pair in ((d1.detach().mean(1), chamfer_paired(x1.detach(), x2.detach())),
                       (d2.detach().mean(1), chamfer_paired(x2.detach(), x1.detach()))):
        assert float(((mean - pair).abs() / pair.abs()).max()) <= 1e-6
    (d1.mean() + d2.mean()).backward()
    B = a.shape[0]
    g1, g2 = np.full((B, n), np.float32(1.0 / (B * n))), np.full((B, m), np.float32(1.0 / (B * m)))
    check_chamfer_grads(a, b, g1, g2, idx1.cpu().numpy(), idx2.cpu().numpy(), x1.grad.cpu().numpy(), x2.grad.cpu().numpy(),
                        ("autograd", n, m))
    e1, e2 = ChamferDistance()(x1.detach(), x2.detach())
    assert torch.equal(e1, n1) and torch.equal(e2, n2) and not e1.requires_grad
