"""Coordinate.points_to_depth (the reference's utils/lidar.py:70-107, with normalize_minmax for the missing minmax_norm)
restated in numpy, for tests/test_points_to_depth_cpu.py and tests/test_gpu_points_to_depth.py.  `dtype` is the precision
of every step (float64: the yardstick; float32: what the format alone loses, the round trip's e32)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "points_to_depth.npz")


def load_golden():
    return dict(np.load(GOLDEN))


def angles(xyz, dtype=np.float64):
    p = np.asarray(xyz)[..., :3].astype(dtype)
    return np.arctan2(p[..., 2], np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2)), np.arctan2(p[..., 1], p[..., 0])


def separable(grid):
    """elevation constant along a row and azimuth constant along a column (the nominal grid): the argmin then splits"""
    return bool((grid[0] == grid[0][:, :1]).all() and (grid[1] == grid[1][:1]).all())


def nearest_pixel(u, v, grid, dtype=np.float64, split=False):
    """[n] angles -> [n] argmin over all pixels of (u - U)^2 + (v - V)^2, the lowest index on a tie (np.argmin's rule).
    split: on a separable grid the minimum of the sum is the sum of the minima, row and column searched on their own
    (lowest row, then lowest column = lowest index): the same pixel wherever the brute-force margin exceeds rounding,
    at H + W instead of H W comparisons per point - what makes the 64 x 1024 round trip a test of seconds."""
    H, W = grid.shape[1:]
    U, V = grid[0].astype(dtype), grid[1].astype(dtype)
    if split:
        assert separable(grid)
        row = np.argmin((u[:, None] - U[:, 0][None]) ** 2, axis=1)
        col = np.argmin((v[:, None] - V[0][None]) ** 2, axis=1)
        return row * W + col
    U, V = U.reshape(-1), V.reshape(-1)
    ids = np.empty(len(u), np.int64)
    for i in range(0, len(u), 256):
        d = (u[i:i + 256, None] - U[None]) ** 2 + (v[i:i + 256, None] - V[None]) ** 2
        ids[i:i + 256] = np.argmin(d, axis=1)
    return ids


def points_to_depth(xyz, grid, min_depth, max_depth, tau=2.0, drop_value=1.0, counts=None, dtype=np.float64, split=False):
    """xyz [B,N,>=3] unit space, grid [2,H,W] -> (depth [B,H,W] dtype, valid [B,H,W] bool, ids [B,N] int64, -1 for a
    point that takes no part: non-finite, out of (min_depth, max_depth), at or beyond counts[b])"""
    xyz = np.asarray(xyz)
    B, N = xyz.shape[:2]
    H, W = grid.shape[1:]
    depth = np.empty((B, H, W), dtype)
    valid = np.empty((B, H, W), bool)
    ids = np.full((B, N), -1, np.int64)
    for b in range(B):
        n = N if counts is None else int(counts[b])
        p = xyz[b, :n, :3].astype(dtype)
        with np.errstate(invalid="ignore", over="ignore"):
            d_u = np.sqrt((p ** 2).sum(1))
            d_m = d_u * dtype(max_depth)
            part = np.isfinite(p).all(1) & (d_m > min_depth) & (d_m < max_depth)
        p, d_u, d_m = p[part], d_u[part], d_m[part]
        w = 1.0 / np.exp(dtype(tau) * d_u)
        u, v = angles(p, dtype)
        k = nearest_pixel(u, v, grid, dtype, split)
        ids[b, :n][part] = k
        num, den = np.zeros(H * W, dtype), np.zeros(H * W, dtype)
        np.add.at(num, k, w * d_m)
        np.add.at(den, k, w)
        d2 = num / (den + dtype(1e-8))
        ok = d2 != 0
        depth[b] = np.where(ok, (d2 - dtype(min_depth)) / dtype(max_depth - min_depth), dtype(drop_value)).reshape(H, W)
        valid[b] = ok.reshape(H, W)
    return depth, valid, ids
