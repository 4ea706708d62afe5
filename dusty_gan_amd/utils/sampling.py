"""Furthest point sampling -- reference: utils/sampling/fps/furthest_point_sampling.py:21-93 (CUDA extension
furthest_point_sampling.cu).  One kernel (csrc/point_fps.hip fps_kernel) selects and gathers.
Point maps ([B,3,H,W], what dg_inv_to_xyz writes and what a scan's "xyz" is) are sampled where they lie by dg_fps_map:
the same selection, bit for bit, without the transposed [B,HW,3] copy and, up to 65 536 points, without a workspace."""
import torch

from .. import _lib as L


def _check(xyz):
    assert xyz.ndim == 3, "expected 3-dim, but got {}-dim tensor".format(xyz.ndim)
    assert xyz.size(2) == 3, "expected (B,N,3), but got {}".format(xyz.shape)
    assert xyz.is_cuda  # same assertion as the reference (:87): there is no CPU path
    return xyz.contiguous().float()


def _run(xyz, k, gather):
    xyz = _check(xyz)
    B, N, _ = xyz.shape
    idx = torch.empty(B, k, dtype=torch.int32, device=xyz.device)
    temp = torch.empty(B, N, dtype=torch.float32, device=xyz.device)
    out = torch.empty(B, k, 3, dtype=torch.float32, device=xyz.device) if gather else None
    L.check(L.lib().dg_fps(L.ptr(xyz), B, N, int(k), L.ptr(temp), L.ptr(idx), L.ptr(out), L.stream_ptr()), "dg_fps")
    return idx, out


def furthest_point_sampling(xyz, npoint):
    """(B,N,3) -> (B,npoint) int32 indices (:21-43)"""
    return _run(xyz, npoint, False)[0]


def downsample_point_clouds(xyz, k):
    """(B,N,3) -> (B,k,3) (:84-93)"""
    return _run(xyz, k, True)[1]


ON_CHIP_MAX = 65536  # dg_fps_map keeps the minima of a planar map of up to this many points on chip: no workspace


def _run_map(xyz_map, k, gather):
    assert xyz_map.ndim in (3, 4), "expected (B,3,H,W) or (B,3,N), but got {}".format(tuple(xyz_map.shape))
    assert xyz_map.size(1) == 3, "expected (B,3,H,W) or (B,3,N), but got {}".format(tuple(xyz_map.shape))
    assert xyz_map.is_cuda
    x = xyz_map.flatten(2).contiguous().float()  # a view of a contiguous fp32 map
    B, _, N = x.shape
    idx = torch.empty(B, k, dtype=torch.int32, device=x.device)
    temp = torch.empty(B, N, dtype=torch.float32, device=x.device) if N > ON_CHIP_MAX else None
    out = torch.empty(B, k, 3, dtype=torch.float32, device=x.device) if gather else None
    L.check(L.lib().dg_fps_map(L.ptr(x), 3 * N, 1, N, B, N, int(k), L.ptr(temp), L.ptr(idx), L.ptr(out), L.stream_ptr()),
            "dg_fps_map")
    return idx, out


def furthest_point_sampling_map(xyz_map, npoint):
    """(B,3,H,W) or (B,3,N) -> (B,npoint) int32 indices into the flattened map: furthest_point_sampling of its points"""
    return _run_map(xyz_map, npoint, False)[0]


def downsample_point_map(xyz_map, k):
    """(B,3,H,W) or (B,3,N) -> (B,k,3): downsample_point_clouds(xyz_map.flatten(2).transpose(1, 2), k) without the copy"""
    return _run_map(xyz_map, k, True)[1]
