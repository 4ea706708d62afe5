"""dg_fps_map (csrc/point_fps.hip): furthest point sampling on strided clouds - planar point maps with the running minima on
chip (16 and 64 slots per thread), everything else through the workspace - must return what dg_fps returns on the packed
copy of the same points, bit for bit, and with it what the reference's own kernel recorded (tests/golden/fps_emd.npz)."""
import numpy as np
import pytest
import torch

from oracle import metrics_oracle as MO
from tests.golden_util import load
from tests.test_gpu_metrics import lidar_like_clouds

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 1024   # threads of a workgroup at n >= 1024: thread t owns the points t, t + T, ...


def fps_map_raw(x, strides, B, n, m, temp="auto", gather=True):
    """dg_fps_map on the device tensor x with (batch, point, channel) strides -> (rc, idx, out)"""
    from dusty_gan_amd import _lib as L
    idx = torch.full((B, m), -7, dtype=torch.int32, device=DEV)
    out = torch.full((B, m, 3), float("nan"), device=DEV) if gather else None
    if isinstance(temp, str):
        temp = torch.empty(B, n, device=DEV)
    rc = L.lib().dg_fps_map(L.ptr(x), *strides, B, n, m, L.ptr(temp), L.ptr(idx), L.ptr(out), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, idx, out


def planar(pts):
    """[B,n,3] -> the planar map [B,3,n] and its strides"""
    n = pts.shape[1]
    return pts.transpose(1, 2).contiguous(), (3 * n, 1, n)


def packed(pts):
    return pts.contiguous(), (3 * pts.shape[1], 3, 1)


def padded(pts):
    """[B,n,3] -> points of 5 floats with the coordinates 2 apart, batches 7 floats further apart than needed"""
    B, n, _ = pts.shape
    buf = torch.full((B, n * 5 + 7), 123.0, device=pts.device)
    v = buf[:, :n * 5].view(B, n, 5)
    v[:, :, 0], v[:, :, 2], v[:, :, 4] = pts[:, :, 0], pts[:, :, 1], pts[:, :, 2]
    return buf, (n * 5 + 7, 5, 2)


def fps_packed(pts, m):
    from dusty_gan_amd.utils.sampling import downsample_point_clouds, furthest_point_sampling
    return furthest_point_sampling(pts, m), downsample_point_clouds(pts, m)


def threshold_points():
    """points of the recorded `thresh` clouds whose float32 squared norm is exactly float32(1e-3), its lower and its upper
    neighbour (the skip is `mag < 1e-3f`: only the lower one is skipped)"""
    xyz = load("fps_emd")["fps/thresh_n2048/xyz"].reshape(-1, 3).astype(np.float32)
    mag = (xyz[:, 0] * xyz[:, 0] + xyz[:, 1] * xyz[:, 1]) + xyz[:, 2] * xyz[:, 2]
    t = np.float32(1e-3)
    out = []
    for want in (np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(1))):
        hit = np.flatnonzero(mag == want)
        assert hit.size, want
        out.append(xyz[hit[0]])
    return np.stack(out)


def tie_skip_clouds(n, seed):
    """[3,n,3]: 0 an integer lattice scaled by 2^-4 (exact arithmetic: ties everywhere) with duplicated points and a block
    of exact origins; 1 a scan-like cloud with dropped returns; 2 a coarse lattice scaled by 2^-2.  Clouds 1 and 2 carry
    the three threshold points in the first, a middle and the last slot of a thread."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-8, 9, (n, 3)).astype(np.float32) * np.float32(2.0 ** -4)
    a[n // 4:n // 4 + max(1, n // 8)] = 0.0
    a[n // 2:n // 2 + n // 16] = a[:n // 16]
    b = lidar_like_clouds(1, n, seed=seed + 1)[0]
    c = rng.integers(-2, 3, (n, 3)).astype(np.float32) * np.float32(2.0 ** -2)
    sp = threshold_points()
    slots = -(-n // T)
    for cloud, lane in ((b, 5), (c, 700)):
        for j, slot in enumerate(sorted({0, slots // 2, slots - 1})):
            for e in range(3):
                k = slot * T + (lane + 17 * e + j) % T
                if k < n:
                    cloud[k] = sp[(e + j) % 3] * np.float32(1 if e != 1 else -1)
    return np.stack([a, b, c]).astype(np.float32)


SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 16383, 16384, 16385, 65535, 65536, 65537, 131072]
_cases = {}


def case(n):
    """the clouds of size n on the device and dg_fps's answer on them, computed once"""
    if n not in _cases:
        pts = torch.from_numpy(tie_skip_clouds(n, seed=n)).to(DEV)
        _cases[n] = (pts, min(64, n)) + fps_packed(pts, min(64, n))
    return _cases[n]


@pytest.mark.parametrize("n", SIZES)
def test_fps_map_equals_dg_fps(n):
    """every slot-count and path boundary (16 x 1024, 64 x 1024 points; the workspace path beyond), B = 3, m = 64, on
    clouds full of ties and skipped points: planar, packed-through-strides and padded input all return dg_fps's bits"""
    pts, m, want_idx, want_out = case(n)
    for layout in (planar, packed, padded):
        x, strides = layout(pts)
        rc, idx, out = fps_map_raw(x, strides, 3, n, m)
        assert rc == 0, (layout.__name__, rc)
        assert torch.equal(idx, want_idx), layout.__name__
        assert torch.equal(out, want_out), layout.__name__
    if n <= 65536:   # the on-chip path leaves the workspace alone: no workspace needed
        x, strides = planar(pts)
        rc, idx, out = fps_map_raw(x, strides, 3, n, m, temp=None)
        assert rc == 0 and torch.equal(idx, want_idx) and torch.equal(out, want_out)
        rc, idx2, none = fps_map_raw(x, strides, 3, n, m, temp=None, gather=False)
        assert rc == 0 and none is None and torch.equal(idx2, want_idx)
    if n == 1025:
        for b in range(3):
            assert idx[b].cpu().tolist() == MO.fps(pts[b].cpu().numpy(), m).tolist(), b


@pytest.mark.parametrize("family", ["lattice", "thresh", "scan"])
def test_fps_map_matches_the_reference_kernel(family):
    """what the reference's own kernel returned on an MI355X (tests/golden/fps_emd.npz, n = 1 .. 2048), from a planar map
    and from the packed cloud through strides: index-exact, and the gathered points"""
    from tests.test_oracle_golden import FPS_RUNGS
    g = load("fps_emd")
    for n in FPS_RUNGS:
        xyz, want = g[f"fps/{family}_n{n}/xyz"], g[f"fps/{family}_n{n}/idx"]
        m = want.shape[1]
        pts = torch.from_numpy(xyz).to(DEV)
        gathered = torch.from_numpy(np.stack([xyz[b][want[b]] for b in range(3)]))
        for layout in (planar, packed):
            x, strides = layout(pts)
            rc, idx, out = fps_map_raw(x, strides, 3, n, m)
            assert rc == 0
            assert idx.cpu().tolist() == want.tolist(), (family, n, layout.__name__)
            assert torch.equal(out.cpu(), gathered), (family, n, layout.__name__)


def test_point_map_functions_on_a_projected_map():
    """downsample_point_map / furthest_point_sampling_map straight off dg_inv_to_xyz's [B,3,32,256] map at tol = 0.05 (which
    has dropped pixels at the origin) against the packed path on the transposed copy"""
    from dusty_gan_amd.utils.lidar import LiDAR
    from dusty_gan_amd.utils.sampling import (downsample_point_clouds, downsample_point_map, furthest_point_sampling,
                                              furthest_point_sampling_map)
    lidar = LiDAR(32, 256, 1.45, 80.0).use_nominal_angles().to(DEV)
    inv = torch.rand(3, 1, 32, 256, generator=torch.Generator().manual_seed(3)).to(DEV) * 0.3
    xyz = lidar.inv_to_xyz(inv, 0.05)
    dropped = int((xyz.abs().sum(1) == 0).sum())
    assert 0 < dropped < xyz[:, 0].numel()
    cloud = xyz.flatten(2).transpose(1, 2).contiguous()
    assert torch.equal(downsample_point_map(xyz, 64), downsample_point_clouds(cloud, 64))
    assert torch.equal(furthest_point_sampling_map(xyz, 64), furthest_point_sampling(cloud, 64))
    assert torch.equal(downsample_point_map(xyz.flatten(2), 64), downsample_point_clouds(cloud, 64))
    with pytest.raises(AssertionError):
        downsample_point_map(cloud, 64)    # a packed cloud is not a point map
    with pytest.raises(AssertionError):
        downsample_point_map(xyz.cpu(), 64)


def test_fps_map_edges():
    from dusty_gan_amd import _lib as L
    pts, _, _, _ = case(65)
    x, strides = planar(pts)
    rc, idx, out = fps_map_raw(x, strides, 3, 65, 65)          # m == n
    want_idx, want_out = fps_packed(pts, 65)
    assert rc == 0 and torch.equal(idx, want_idx) and torch.equal(out, want_out)
    assert fps_map_raw(x, strides, 3, 65, 66)[0] == L.DG_EINVAL   # m > n
    for n in (300, 20000):                                       # nothing is a candidate: index 0 throughout
        z = torch.zeros(2, 3, n, device=DEV)
        rc, idx, out = fps_map_raw(z, (3 * n, 1, n), 2, n, 5)
        assert rc == 0 and idx.cpu().tolist() == [[0] * 5] * 2 and float(out.abs().max()) == 0.0
    big, m, want_idx, _ = case(65537)
    x, strides = planar(big)
    assert fps_map_raw(x, strides, 3, 65537, m, temp=None)[0] == L.DG_EINVAL   # the workspace path needs its workspace
    big, m, want_idx, _ = case(65536)
    x, strides = planar(big)
    rc, idx, _ = fps_map_raw(x, strides, 3, 65536, m, temp=None)
    assert rc == 0 and torch.equal(idx, want_idx)
    x, strides = packed(big)
    assert fps_map_raw(x, strides, 3, 65536, m, temp=None)[0] == L.DG_EINVAL   # packed input: workspace path
    assert L.lib().dg_fps_map(None, 3, 1, 1, 1, 1, 1, None, L.ptr(idx), None, L.stream_ptr()) == L.DG_EINVAL
    assert L.lib().dg_fps_map(L.ptr(x), 3, 1, 1, 1, 1, 1, None, None, None, L.stream_ptr()) == L.DG_EINVAL


@pytest.mark.parametrize("n", [1025, 65536])
def test_fps_map_is_deterministic(n):
    pts, m, _, _ = case(n)
    x, strides = planar(pts)
    a, b = fps_map_raw(x, strides, 3, n, m, temp=None), fps_map_raw(x, strides, 3, n, m, temp=None)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
