"""The target corruptions of the reference's demo (demo.py:71-137) restated on torch CPU tensors, with a closing loop that
ends: what the GPU tests compare against where a golden would be too large to commit.  tests/test_corruption_cpu.py holds
this file to tests/golden/corruption.npz (made from the reference's own functions)."""
import torch
import torch.nn.functional as F

from tests.golden_util import load

CASES = ("c0", "c1", "c2")
NAMED = ("additive noise", "low resolution", "dropout", "closing")
THRESH = 1e-8


def case(name, g=None):
    """{key: tensor} of one case of tests/golden/corruption.npz"""
    g = load("corruption") if g is None else g
    pre = name + "/"
    return {k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}


def every(n, rate):
    keep = torch.zeros(n)
    keep[::int(1 / rate)] = 1.0
    return keep


def mask_corrupt(mask, row_keep=None, col_keep=None, u=None, rate=1.0):
    out = mask.clone()
    if row_keep is not None:
        out = out * row_keep.view(1, 1, -1, 1)
    if col_keep is not None:
        out = out * col_keep.view(1, 1, 1, -1)
    if u is not None:
        out = out * (u.view_as(mask) < rate).float()
    return out


def half_keep(W):
    keep = torch.ones(W)
    keep[W // 2:] = 0.0
    return keep


def quarter_keep(W):
    keep = torch.ones(W)
    keep[: W // 4] = 0.0
    keep[W // 2: W * 3 // 4] = 0.0
    return keep


def rows_keep(H, rows):
    keep = torch.ones(H)
    keep[rows.long()] = 0.0
    return keep


def additive_noise(depth, noise, strength=0.01):
    return depth + noise * strength


def median_blur3(x):
    B, C, H, W = x.shape
    taps = F.unfold(x.reshape(B * C, 1, H, W), 3, padding=1)
    return torch.median(taps, dim=1).values.reshape(B, C, H, W)


def hole_fill(x, thresh=THRESH):
    """Jacobi sweeps per sample until no hole is left, a sweep fills nothing, or max(H, W) - 1 (at least one) sweeps ->
    (image, sweeps [B], left [B])"""
    B, _, H, W = x.shape
    out, sweeps, left = x.clone(), [], []
    for b in range(B):
        inv, n = x[b:b + 1].clone(), 0
        holes = int((inv <= thresh).sum())
        for _ in range(max(1, max(H, W) - 1)):
            valid = (inv > thresh).float()
            filled = F.max_pool2d(inv, (3, 3), 1, (1, 1))
            new = valid * inv + (1 - valid) * filled
            now = int((new <= thresh).sum())
            if now == holes:
                break
            inv, n, holes = new, n + 1, now
            if holes == 0:
                break
        out[b:b + 1] = inv
        sweeps.append(n)
        left.append(holes)
    return out, torch.tensor(sweeps, dtype=torch.int32), torch.tensor(left, dtype=torch.int32)


def closing(x):
    return hole_fill(median_blur3(x))


def apply_corruption(depth, mask, name, u=None, noise=None):
    if name == "additive noise":
        return additive_noise(depth, noise, 0.01), mask
    if name == "low resolution":
        return depth, mask_corrupt(mask, row_keep=every(mask.shape[2], 1 / 8))
    if name == "dropout":
        return depth, mask_corrupt(mask, u=u, rate=0.1)
    if name == "closing":
        return closing(depth)[0], torch.ones_like(mask)
    raise ValueError(name)


def scan_like(B, H, W, keep, hole, seed, at=None):
    """a synthetic normalised depth [B,1,H,W] with validity rate `keep` and a rectangular hole (h, w) whose corner is `at`
    (default: in the middle)"""
    g = torch.Generator().manual_seed(seed)
    mask = (torch.rand(B, 1, H, W, generator=g) < keep).float()
    hh, hw = hole
    h0, w0 = ((H - hh) // 2, (W - hw) // 2) if at is None else at
    mask[:, :, h0:h0 + hh, w0:w0 + hw] = 0.0
    return (0.05 + 0.9 * torch.rand(B, 1, H, W, generator=g)) * mask, mask
