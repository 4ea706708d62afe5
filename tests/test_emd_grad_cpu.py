"""CPU-side checks of the point-set distance gradients' yardsticks (tests/emd_grad_util.py, tests/golden/emd_grad.npz) and of
the argument errors of dusty_gan_amd.utils.metrics.distance, which come before any launch."""
import numpy as np
import pytest
import torch

from oracle import metrics_oracle as MO
from tests import emd_grad_util as U
from tests.golden_util import load


@pytest.fixture(scope="module")
def clouds():
    g = load("fps_emd")
    return {name: (g[f"emd/{name}/a"], g[f"emd/{name}/b"]) for name in U.EMD_GRAD_CASES}


@pytest.fixture(scope="module")
def f64(clouds):
    """(cost, g1, g2) of the float64 restatement, computed once"""
    return {name: U.emd_grads(a, b, np.float64) for name, (a, b) in clouds.items()}


def test_restatement_cost_is_the_oracles(clouds, f64):
    for name, (a, b) in clouds.items():
        want = MO.emd_costs(a, b, np.float64)
        assert np.all(np.abs(f64[name][0] - want) <= 1e-12 * np.abs(want)), name


def test_restatement_gradients_are_translation_free_and_euler_homogeneous(clouds, f64):
    """with match constant the cost is sum match |a - b|^2: moving both clouds together changes nothing (sum g1 + sum g2 = 0)
    and scaling both scales it by the square (<g1, a> + <g2, b> = 2 cost)"""
    for name, (a, b) in clouds.items():
        cost, g1, g2 = f64[name]
        for i in range(a.shape[0]):
            gmax = max(np.abs(g1[i]).max(), np.abs(g2[i]).max())
            drift = np.abs(g1[i].sum(0) + g2[i].sum(0)).max()
            euler = abs((g1[i] * a[i]).sum() + (g2[i] * b[i]).sum() - 2.0 * cost[i])
            print(name, i, "drift / max|g|", drift / max(gmax, 1e-300), "euler / max|g|", euler / max(gmax, 1e-300))
            assert drift <= 1e-11 * gmax, (name, i, drift, gmax)
            assert euler <= 1e-11 * gmax, (name, i, euler, gmax)


def test_fixture_holds_the_restatement_and_stays_well_conditioned(clouds, f64):
    """the file's float64 gradients are the restatement's; e_ref is at least the float32-order restatement's distance from
    them (more where the reference's kernel was recorded) and never above 1e-3 max|g|: a case that needs a wider band tests
    the conditioning of approxmatch, not a kernel"""
    g = load("emd_grad")
    assert list(g["meta/cases"]) == U.EMD_GRAD_CASES
    for name, (a, b) in clouds.items():
        _, g1, g2 = f64[name]
        _, s1, s2 = U.emd_grads(a, b, np.float32)
        for k, (want, f32) in enumerate(((g1, s1), (g2, s2)), 1):
            got, e_ref = g[f"{name}/g{k}_f64"], g[f"{name}/e_ref{k}"]
            gmax = np.abs(want).max((1, 2))
            assert got.shape == want.shape and np.all(np.abs(got - want) <= 1e-9 * gmax[:, None, None]), (name, k)
            e32 = np.abs(f32 - want).max((1, 2))
            print(name, f"g{k}", "e_ref / max|g|", (e_ref / np.maximum(gmax, 1e-300)).max(), "float32 order alone",
                  (e32 / np.maximum(gmax, 1e-300)).max())
            assert np.all(1.01 * e_ref + 1e-9 * gmax >= e32), (name, k)   # (the exponentials' last bits may differ by libm)
            assert np.all(e_ref <= 1e-3 * gmax), (name, k, e_ref, gmax)
            if f"{name}/ref_g{k}" in g.files:
                assert np.all(np.abs(g[f"{name}/ref_g{k}"] - want).max((1, 2)) <= e_ref), (name, k)


def test_match_grads_reads_the_reference_layout():
    rng = np.random.default_rng(0)
    a, b = rng.normal(size=(2, 5, 3)), rng.normal(size=(2, 7, 3))
    match = rng.random((2, 5, 7))
    g1, g2 = U.match_grads(a, b, match, grad_cost=[1.0, -2.0])
    h1, h2 = U.match_grads_ref_layout(a, b, match.transpose(0, 2, 1).reshape(-1))
    assert np.allclose(h1[0], g1[0]) and np.allclose(-2.0 * h2[1], g2[1])
    # the literal loops of matchcostgrad1 / matchcostgrad2
    want1, want2 = np.zeros((5, 3)), np.zeros((7, 3))
    for k in range(5):
        for l in range(7):
            want1[k] += (a[0, k] - b[0, l]) * match[0, k, l] * 2
            want2[l] += (b[0, l] - a[0, k]) * match[0, k, l] * 2
    assert np.allclose(g1[0], want1, rtol=1e-13, atol=1e-13) and np.allclose(g2[0], want2, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("n,m", [(1, 1), (7, 5), (40, 64)])
def test_chamfer_backward_restatement_against_autograd(n, m):
    """from given indices, against torch autograd in float64 through the gathered distances, on tie-free clouds"""
    rng = np.random.default_rng(n * 100 + m)
    a, b = rng.normal(size=(3, n, 3)), rng.normal(size=(3, m, 3))
    g1, g2 = rng.normal(size=(3, n)), rng.normal(size=(3, m))
    ta, tb = torch.from_numpy(a).requires_grad_(), torch.from_numpy(b).requires_grad_()
    d = ((ta[:, :, None, :] - tb[:, None, :, :]) ** 2).sum(-1)
    d1, idx1 = d.min(2)
    d2, idx2 = d.min(1)
    ((d1 * torch.from_numpy(g1)).sum() + (d2 * torch.from_numpy(g2)).sum()).backward()
    grad1, grad2, abs1, abs2, cnt1, cnt2 = U.chamfer_backward_f64(a, b, g1, g2, idx1.numpy(), idx2.numpy())
    assert np.allclose(grad1, ta.grad.numpy(), rtol=1e-12, atol=1e-13)
    assert np.allclose(grad2, tb.grad.numpy(), rtol=1e-12, atol=1e-13)
    assert cnt1.sum() == cnt2.sum() == 3 * (n + m) and np.all(abs1 >= np.abs(grad1) * (1 - 1e-12))
    assert U.chamfer_bound(abs1, cnt1).shape == grad1.shape


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """the C entries validate before they touch the HIP runtime: null pointers and empty clouds are DG_EINVAL, clouds above
    the caps (n + m > 6400 for dg_emd_grad, 2^18 points for dg_chamfer_backward) DG_EUNSUPPORTED"""
    import ctypes as C
    from dusty_gan_amd import _lib as L
    L.build()
    lib = L.lib()
    p = C.cast((C.c_float * 4)(), C.c_void_p)   # never dereferenced: every call below returns before a launch
    assert lib.dg_emd_grad(None, 4, p, 4, 1, None, None, p, p, None) == L.DG_EINVAL
    assert lib.dg_emd_grad(p, 4, p, 4, 1, None, None, None, p, None) == L.DG_EINVAL
    assert lib.dg_emd_grad(p, 0, p, 4, 1, None, None, p, p, None) == L.DG_EINVAL
    assert lib.dg_emd_grad(p, 3201, p, 3200, 1, None, None, p, p, None) == L.DG_EUNSUPPORTED
    assert lib.dg_emd_grad(p, 1, p, 6400, 1, None, p, p, p, None) == L.DG_EUNSUPPORTED
    assert lib.dg_chamfer_backward(p, 4, p, 4, 1, p, p, p, p, p, p, None, None) == L.DG_EINVAL
    assert lib.dg_chamfer_backward(p, 4, p, 4, 0, p, p, p, p, p, p, p, None) == L.DG_EINVAL
    assert lib.dg_chamfer_backward(p, (1 << 18) + 1, p, 4, 1, p, p, p, p, p, p, p, None) == L.DG_EUNSUPPORTED
    assert lib.dg_chamfer_backward(p, 4, p, (1 << 18) + 1, 1, p, p, p, p, p, p, p, None) == L.DG_EUNSUPPORTED


def test_argument_errors_come_before_any_launch():
    """CPU tensors here, so anything that reached a launch would fail differently: shapes are refused first (AssertionError),
    then the device (the module's RuntimeError: no CPU fallback)"""
    from dusty_gan_amd.utils import metrics as M
    a, b = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3)
    for bad in (torch.zeros(2, 5), torch.zeros(2, 5, 4), torch.zeros(5, 3)):
        with pytest.raises(AssertionError):
            M.earth_mover_distance_grad(bad, b)
        with pytest.raises(AssertionError):
            M.earth_mover_distance_grad(a, bad)
        with pytest.raises(AssertionError):
            M.chamfer_distance(bad, b)
        with pytest.raises(AssertionError):
            M.chamfer_backward(a, bad, torch.zeros(2, 5), torch.zeros(2, 7), torch.zeros(2, 5), torch.zeros(2, 7))
    with pytest.raises(AssertionError):
        M.earth_mover_distance_grad(a, torch.zeros(3, 7, 3))           # paired clouds
    for gc in (torch.zeros(3), torch.zeros(2, 1), torch.zeros(())):
        with pytest.raises(AssertionError):
            M.earth_mover_distance_grad(a, b, gc)
    with pytest.raises(AssertionError):
        M.chamfer_backward(a, b, torch.zeros(2, 7), torch.zeros(2, 7), torch.zeros(2, 5), torch.zeros(2, 7))
    i5, i7 = torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 7, dtype=torch.int32)
    for call in (lambda: M.earth_mover_distance_grad(a, b), lambda: M.earth_mover_distance_grad(a, b, torch.ones(2)),
                 lambda: M.earth_mover_distance(a.clone().requires_grad_(), b), lambda: M.EarthMoverDistance()(a, b, 0.005, 50),
                 lambda: M.chamfer_distance(a, b), lambda: M.ChamferDistance()(a, b),
                 lambda: M.chamfer_backward(a, b, torch.zeros(2, 5), torch.zeros(2, 7), i5, i7)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
