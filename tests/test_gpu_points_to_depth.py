"""LiDAR.points_to_depth / dg_points_to_depth on the GPU (csrc/points_depth.hip, dusty_gan_amd/utils/lidar.py).

Against the reference (tests/golden/points_to_depth.npz, written by tests/golden/make_points_to_depth_golden.py from its
utils/lidar.py): the index of every point equals the float64 argmin (the fixture asserts a margin of 1e-4 rad, so no
precision can flip one), `valid` is equal everywhere and per pixel |depth - fp64| <= 2 e_ref + 1e-6, e_ref = the
reference's own max |fp32 - fp64| read from the fixture (the rule of test_gpu_render / test_gpu_raw_scan: twice what the
reference loses in float32, plus a floor for the sums' 2^-40 quantum and the normalisation).  Edge shapes against the
float64 restatement of tests/points_to_depth_util.py, which tests/test_points_to_depth_cpu.py pins to the same fixture.

Figures printed on an MI355X are recorded in DESIGN.md 7g."""
import numpy as np
import pytest
import torch

from tests import points_to_depth_util as PU

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def g():
    return PU.load_golden()


def make_lidar(g, grid="grid"):
    from dusty_gan_amd.utils.lidar import LiDAR
    lidar = LiDAR(16, 64, float(g["meta/min_depth"]), float(g["meta/max_depth"]))
    lidar.angle = torch.from_numpy(g[grid])[None].contiguous()
    return lidar.to(DEV)


@pytest.fixture(scope="module")
def first(g):
    """the fixture's clouds through the Python surface, once: (depth, valid, idx) that the other tests compare with"""
    lidar = make_lidar(g)
    xyz = torch.from_numpy(g["xyz"]).to(DEV)
    keep = xyz.clone()
    out = lidar.points_to_depth(xyz, drop_value=1, tau=float(g["meta/tau"]), return_index=True)
    assert torch.equal(xyz, keep)
    return lidar, xyz, out


def test_fixture_parity(g, first):
    lidar, xyz, (depth, valid, idx) = first
    assert depth.shape == (2, 1, 16, 64) and depth.dtype == torch.float32
    assert valid.shape == (2, 1, 16, 64) and valid.dtype == torch.bool and idx.shape == (2, 1500) and idx.dtype == torch.int32
    want = np.where(g["weightless"], -1, g["f64/ids"])
    assert np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(valid[:, 0].cpu().numpy(), g["f64/valid"])
    bound = 2 * float(g["e_ref"]) + 1e-6
    err = np.abs(depth[:, 0].double().cpu().numpy() - g["f64/depth"])
    print(f"fixture parity: max err {err.max():.3e}, bound {bound:.3e}, ratio {err.max() / bound:.3f} (e_ref {float(g['e_ref']):.3e})")
    assert (err <= bound).all()
    for drop in (1.0, 0.0):
        d, v = lidar.points_to_depth(xyz, drop_value=drop, tau=float(g["meta/tau"]))
        assert torch.equal(v, valid) and bool((d[~v] == drop).all()) and torch.equal(d[v], depth[valid])


def test_a_tie_goes_to_the_lower_index(g):
    lidar = make_lidar(g, "tie/grid")
    depth, valid, idx = lidar.points_to_depth(torch.from_numpy(g["tie/xyz"]).to(DEV), tau=float(g["meta/tau"]), return_index=True)
    idx = idx.cpu().numpy()
    assert ((idx // 64) == 4).all() and np.array_equal(idx, g["tie/ids"])
    assert np.array_equal(valid[:, 0].cpu().numpy(), g["tie/valid"]) and not bool(valid[0, 0, 5].any())
    err = np.abs(depth[:, 0].double().cpu().numpy() - g["tie/depth"])
    print(f"tie grid: max err {err.max():.3e}")
    assert (err <= 1e-6).all()   # (float64 arithmetic on the same inputs, rounded once: the floor alone)


def test_a_tie_across_chunks_goes_to_the_first_chunk(g):
    """The streamed search's tie rule (csrc/nn_stream.h) across LDS chunks: a 3 x 512 grid is three chunks of 512 pixels, and
    rows 0 and 2 hold the SAME angles, so a point aimed at row 0 is exactly as far from pixel j as from pixel 1024 + j (the same
    bits, in any precision).  Every index must lie below 1024.  1030 points: a second workgroup, with six of them."""
    from dusty_gan_amd.utils.lidar import LiDAR
    lo, hi, tau = float(g["meta/min_depth"]), float(g["meta/max_depth"]), float(g["meta/tau"])
    yaw = np.linspace(np.pi, -np.pi, 513)[:512]
    grid = np.stack([np.repeat(np.array([0.05, -0.2, 0.05])[:, None], 512, axis=1), np.repeat(yaw[None], 3, axis=0)]).astype(np.float32)
    rng = np.random.default_rng(23)
    N = 1030
    pix = rng.integers(0, 1024, N)                                   # pixels of rows 0 and 1
    u, v = grid[0].reshape(-1)[pix].astype(np.float64), grid[1].reshape(-1)[pix].astype(np.float64)
    xyz = (0.3 * np.stack([np.cos(u) * np.cos(v), np.cos(u) * np.sin(v), np.sin(u)], -1)).astype(np.float32)[None]
    rd, rv, ri = PU.points_to_depth(xyz, grid, lo, hi, tau)
    # the restatement itself (np.argmin's rule).  (A point aimed at column 0 lands across the +-pi seam, in column 511.)
    assert ri.min() >= 0 and ri.max() < 1024 and (ri < 512).sum() > 100 and (ri[0] != pix).sum() <= 8
    lidar = LiDAR(3, 512, lo, hi)
    lidar.angle = torch.from_numpy(grid)[None].contiguous()
    lidar = lidar.to(DEV)
    depth, valid, idx = lidar.points_to_depth(torch.from_numpy(xyz).to(DEV), tau=tau, return_index=True)
    idx = idx.cpu().numpy()
    err = np.abs(depth[:, 0].double().cpu().numpy() - rd)
    bound = 2 * float(g["e_ref"]) + 1e-6
    print(f"3 x 512 grid: max idx {idx.max()}, indices off {(idx != ri).sum()}, max err {err.max():.3e}, bound {bound:.3e}")
    assert np.array_equal(idx, ri) and idx.max() < 1024
    assert np.array_equal(valid[:, 0].cpu().numpy(), rv) and not bool(valid[0, 0, 2].any())
    assert (err <= bound).all()


def test_the_order_of_the_points_does_not_matter(g, first):
    lidar, xyz, (depth, valid, idx) = first
    tau = float(g["meta/tau"])
    d2, v2, i2 = lidar.points_to_depth(xyz, tau=tau, return_index=True)
    assert torch.equal(d2.view(torch.int32), depth.view(torch.int32)) and torch.equal(v2, valid) and torch.equal(i2, idx)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(xyz.shape[1])).to(DEV)
    d3, v3, i3 = lidar.points_to_depth(xyz[:, perm].contiguous(), tau=tau, return_index=True)
    assert torch.equal(d3.view(torch.int32), depth.view(torch.int32)) and torch.equal(v3, valid)
    assert torch.equal(i3, idx[:, perm])


def test_graph_replay_equals_eager(g, first):
    """the two launches captured once and replayed: integer sums and a zero-at-rest workspace, so the same bytes"""
    lidar, xyz, (depth, valid, idx) = first
    tau = float(g["meta/tau"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lidar.points_to_depth(xyz, tau=tau)          # (the stream's workspace exists before the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        d, v, i = lidar.points_to_depth(xyz, tau=tau, return_index=True)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(d.view(torch.int32), depth.view(torch.int32)) and torch.equal(v, valid) and torch.equal(i, idx)


def test_strides_and_counts(g, first):
    lidar, xyz, (depth, valid, idx) = first
    lo, hi, tau = float(g["meta/min_depth"]), float(g["meta/max_depth"]), float(g["meta/tau"])
    B, N = xyz.shape[:2]
    rec = torch.cat([xyz, torch.full((B, N, 1), float("nan"), device=DEV)], dim=2)   # (x, y, z, r) records; r is never read
    d4, v4, i4 = lidar.points_to_depth(rec, tau=tau, return_index=True)
    assert torch.equal(d4.view(torch.int32), depth.view(torch.int32)) and torch.equal(v4, valid) and torch.equal(i4, idx)
    # a tail that must not be read: NaN records and points aimed at pixels that are empty
    grid = g["grid"].astype(np.float64).reshape(2, -1)
    tail = np.full((B, 37, 3), np.nan, np.float32)
    empty = [np.nonzero(~g["f64/valid"][b].reshape(-1))[0][:18] for b in range(B)]
    for b in range(B):
        u, v = grid[0][empty[b]], grid[1][empty[b]]
        tail[b, :18] = 0.3 * np.stack([np.cos(u) * np.cos(v), np.cos(u) * np.sin(v), np.sin(u)], -1)
    cut = xyz.clone()
    cut[:, N - 37:] = torch.from_numpy(tail).to(DEV)
    lit = lidar.points_to_depth(cut, tau=tau)[1].flatten(1).cpu().numpy()
    assert all(lit[b][empty[b]].all() for b in range(B))   # read in full, the tail lights its pixels
    counts = np.array([N - 37, 1000])          # (1000: the second workgroup of that cloud has nothing to do)
    d5, v5, i5 = lidar.points_to_depth(cut, tau=tau, counts=torch.from_numpy(counts).to(DEV), return_index=True)
    rd, rv, ri = PU.points_to_depth(cut.cpu().numpy(), g["grid"], lo, hi, tau, counts=counts)
    assert np.array_equal(i5.cpu().numpy(), ri) and np.array_equal(v5[:, 0].cpu().numpy(), rv)
    assert (ri[0, N - 37:] == -1).all() and (ri[1, 1000:] == -1).all() and not any(rv[b].reshape(-1)[empty[b]].any() for b in range(B))
    err = np.abs(d5[:, 0].double().cpu().numpy() - rd)
    bound = 2 * float(g["e_ref"]) + 1e-6
    print(f"counts: max err {err.max():.3e}, bound {bound:.3e}")
    assert (err <= bound).all()
    d6, v6, i6 = lidar.points_to_depth(cut, drop_value=0.25, tau=tau, counts=torch.zeros(B, dtype=torch.int32, device=DEV),
                                       return_index=True)
    assert not bool(v6.any()) and bool((d6 == 0.25).all()) and bool((i6 == -1).all())
    # the sums are zero at rest again: the next call is the first call
    d7, v7 = lidar.points_to_depth(xyz, tau=tau)
    assert torch.equal(d7.view(torch.int32), depth.view(torch.int32)) and torch.equal(v7, valid)


def test_round_trip_at_the_workload_size():
    from dusty_gan_amd.synthesis import export_points
    from dusty_gan_amd.utils.lidar import LiDAR
    lidar = LiDAR(64, 1024, 0.9, 120.0).use_nominal_angles().to(DEV)
    rng = np.random.default_rng(11)
    inv = rng.uniform(0.02, 0.98, (2, 1, 64, 1024)).astype(np.float32)
    inv[rng.random(inv.shape) < 0.30] = 0.0
    inv = torch.from_numpy(inv).to(DEV)
    records, counts = export_points(inv, lidar, tol=0.0, from_tanh=False)
    unit = records / lidar.max_depth
    depth, valid, idx = lidar.points_to_depth(unit, counts=counts, return_index=True)
    keep = lidar.inv_to_xyz(inv, tol=0.0).abs().sum(dim=1, keepdim=True) > 0
    assert torch.equal(keep, inv != 0) and torch.equal(valid, keep)
    n = counts.cpu().numpy()
    idx, unit_h = idx.cpu().numpy(), unit.cpu().numpy()
    for b in range(2):
        assert n[b] == int(keep[b].sum())
        assert np.array_equal(idx[b, :n[b]], np.nonzero(keep[b].reshape(-1).cpu().numpy())[0]) and (idx[b, n[b]:] == -1).all()
    grid = lidar.angle[0].cpu().numpy()
    r64 = PU.points_to_depth(unit_h, grid, 0.9, 120.0, 2.0, counts=n, split=True)
    r32 = PU.points_to_depth(unit_h, grid, 0.9, 120.0, 2.0, counts=n, split=True, dtype=np.float32)
    assert np.array_equal(r64[1], valid[:, 0].cpu().numpy()) and np.array_equal(r64[2], idx)
    e32 = float(np.abs(r32[0].astype(np.float64) - r64[0]).max())
    err = np.abs(depth[:, 0].double().cpu().numpy() - r64[0])
    bound = 2 * e32 + 1e-6
    print(f"round trip 64x1024: max err {err.max():.3e}, bound {bound:.3e}, ratio {err.max() / bound:.3f} (e32 {e32:.3e})")
    assert (err <= bound).all()
    # and the image that went in comes back.  Export, projection and inversion are some fifteen float32 roundings (6e-8
    # relative each) of 1 / depth <= 1 / min_depth = 1.1 over a span of 1.1: 1e-6 on the inverse depth; ten times that
    back = lidar.invert_depth(depth) * valid
    print(f"round trip, inverse depth: max err {float((back - inv).abs().max()):.3e}")
    assert float((back - inv).abs().max()) < 1e-5


def test_bad_arguments(g, first):
    from dusty_gan_amd import _lib as L
    from dusty_gan_amd.utils.lidar import LiDAR
    lidar, xyz, (depth, valid, idx) = first
    with pytest.raises(RuntimeError, match="GPU only"):
        lidar.points_to_depth(xyz.cpu())
    with pytest.raises(RuntimeError, match="no angle grid"):
        LiDAR(16, 64, 0.9, 120.0).points_to_depth(xyz)
    for bad in (xyz[..., :2], xyz[0], xyz[:, :0]):
        with pytest.raises(ValueError):
            lidar.points_to_depth(bad)
    for tau in (-1, 1e3, float("nan")):
        with pytest.raises(ValueError, match="tau"):
            lidar.points_to_depth(xyz, tau=tau)
    with pytest.raises(ValueError, match="counts"):
        lidar.points_to_depth(xyz, counts=torch.zeros(3, dtype=torch.int32, device=DEV))
    # through the ABI; every refusal comes before a launch, so the image's buffers may be small
    B, N = xyz.shape[:2]
    acc = torch.zeros(B * 1024 * 2, dtype=torch.int64, device=DEV)
    out_d, out_v = torch.full((B, 1024), 7.0, device=DEV), torch.zeros(B, 1024, dtype=torch.bool, device=DEV)

    def call(rec=xyz, sb=N * 3, stride=3, n=N, H=16, W=64, lo=0.9, hi=120.0, tau=2.0, a=acc, d=out_d, v=out_v):
        return L.lib().dg_points_to_depth(L.ptr(rec), sb, stride, None, B, n, L.ptr(lidar.angle), H, W, lo, hi, tau, 1.0,
                                          L.ptr(a), L.ptr(d), L.ptr(v), None, L.stream_ptr())
    assert call(H=512, W=1024) == L.DG_EUNSUPPORTED and call(n=(1 << 18) + 1, sb=3 * ((1 << 18) + 1)) == L.DG_EUNSUPPORTED
    assert call(d=None) == L.DG_EINVAL and call(v=None) == L.DG_EINVAL and call(a=None) == L.DG_EINVAL and call(rec=None) == L.DG_EINVAL
    assert call(stride=5) == L.DG_EINVAL and call(sb=N * 3 - 1) == L.DG_EINVAL and call(n=0) == L.DG_EINVAL
    assert call(tau=-1.0) == L.DG_EINVAL and call(tau=16.5) == L.DG_EINVAL and call(tau=float("nan")) == L.DG_EINVAL
    assert call(lo=-1.0) == L.DG_EINVAL and call(hi=0.5) == L.DG_EINVAL
    torch.cuda.synchronize()
    assert bool((out_d == 7.0).all()) and not bool(acc.any())   # nothing ran
    assert call() == L.DG_OK
    torch.cuda.synchronize()
    assert torch.equal(out_d.view(depth.shape), depth) and torch.equal(out_v.view(valid.shape), valid) and not bool(acc.any())
