"""Float64 restatements of what csrc/render.hip computes, for the edge-shape tests (tests/test_gpu_render.py); pinned to
the reference's own outputs by tests/test_render_cpu.py (tests/golden/render.npz).

splat / render follow utils/render.py:18-127 of the reference, with the library's stated deviation: a point with a
non-finite coordinate adds nothing.  grid_bytes states the image-log rules: torchvision's make_grid(nrow=4, padding=2),
matplotlib's Normalize(0,1) + 256-entry table lookup, TensorBoard's float -> byte conversion.
"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render.npz")
_cache = {}


def golden():
    """tests/golden/render.npz, loaded once and shared: callers do not write to it"""
    if "g" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["g"] = {k: z[k] for k in z.files}
    return _cache["g"]


def splat(coords, values, H, W):
    """[B,N,2] coords (row first), [B,N,C] values -> [B,C,H,W], all float64 on the CPU"""
    coords, values = coords.double().cpu(), values.double().cpu()
    B, N, C = values.shape
    out = torch.zeros(B, H * W, C, dtype=torch.float64)
    ok = torch.isfinite(coords).all(-1)
    pos = torch.where(ok[..., None], coords, torch.zeros_like(coords))
    values = torch.where(ok[..., None], values, torch.zeros_like(values))
    lo = torch.floor(pos)
    frac = pos - lo
    size = torch.tensor([H, W], dtype=torch.float64)
    for dh in (0, 1):
        for dw in (0, 1):
            cell = lo + torch.tensor([dh, dw], dtype=torch.float64)
            safe = torch.minimum(torch.maximum(cell, torch.zeros(2, dtype=torch.float64)), size - 1)
            side = torch.where(torch.tensor([dh, dw]).bool(), frac, (lo + 1) - pos)     # distance to the OTHER cell
            side = side * (cell == safe)
            wt = side[..., 0] * side[..., 1]
            wt = wt * (wt >= 1e-3) * ok
            index = (safe[..., 0] * W + safe[..., 1]).long()
            for b in range(B):
                out[b].index_add_(0, index[b], values[b] * wt[b, :, None])
    return out.view(B, H, W, C).permute(0, 3, 1, 2).contiguous()


def render(xyz, normals, L, R=None, t=None, focal=1.0):
    """[B,N,3] points and normals -> the bird's-eye view [B,3,L,L], float64 on the CPU"""
    p = xyz.double().cpu().clone()
    n = normals.double().cpu()
    p[..., 2] = -p[..., 2]
    if R is not None:
        p = p @ R.double().cpu()
    if t is not None:
        p = p + t.double().cpu()
    with np.errstate(all="ignore"):
        uv = (p[..., :2] / p[..., 2:3] * focal + 0.5) * L
    inside = ((uv > 0) & (uv < L - 1)).all(-1, keepdim=True)
    depth = p.norm(dim=-1, keepdim=True)
    weight = torch.exp(-3.0 * depth) * (depth > 1e-8)
    both = splat(L - uv, torch.cat([weight * n * inside, weight], -1), L, L)
    return both[:, :3] / (both[:, 3:] + 1e-8)


def grid_bytes(x, color, scale, lut):
    """x [B,1|3,H,W] float32 numpy, lut [256,3] float32 -> uint8 [Hg,Wg,3]"""
    x = np.asarray(x, dtype=np.float32) * np.float32(scale)
    B, C, H, W = x.shape
    xmaps = min(4, B)
    ymaps = -(-B // xmaps)
    grid = np.zeros((3, ymaps * (H + 2) + 2, xmaps * (W + 2) + 2), dtype=np.float32)
    for k in range(B):
        r, c = (k // xmaps) * (H + 2) + 2, (k % xmaps) * (W + 2) + 2
        grid[:, r:r + H, c:c + W] = x[k] if C == 3 else np.repeat(x[k], 3, 0)
    if color:
        v = grid[0]
        with np.errstate(invalid="ignore"):
            idx = np.clip(np.floor(np.nan_to_num(v, nan=0.0) * np.float32(256)), 0, 255).astype(np.int64)
        rgb = np.asarray(lut, dtype=np.float32)[idx]
        rgb[np.isnan(v)] = 0
    else:
        rgb = np.nan_to_num(grid, nan=0.0).transpose(1, 2, 0)
    return np.clip(rgb * np.float32(255), 0, 255).astype(np.uint8)
