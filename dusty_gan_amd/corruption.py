"""The target corruptions of the reference's restoration experiment -- reference: demo.py:71-137 (the functions of the same
names) and :385-397 (where the demo applies them): the scan a latent is optimised against is degraded - additive noise, an
8x lower vertical resolution, 90 % dropout, or a morphological closing - and the inversion is compared with the full scan.

Every function is a kernel of csrc/corrupt.hip (dg_corrupt_mask, dg_additive_noise, dg_median3x3, dg_hole_fill) and runs on
the GPU only.  Unlike the demo's, none modifies its input: the demo's in-place mask edits (random_lines, corrupt_half,
corrupt_quarter) are a side effect, not a contract.

Draws: the demo seeds torch's generator with 0 and draws once for the whole batch; here scan i of a dataset takes
dg_philox_fill(seed, STREAM_CORRUPT, offset = i ceil(HW / 4)) - uniform for dropout, normal for the noise - so a scan's
corruption does not depend on the batch it travels in (`first_index`: the dataset index of the batch's first scan).  `u`,
`noise` and `rows` inject the numbers instead."""
import torch

from . import _lib as L

CORRUPTIONS = ("additive noise", "low resolution", "dropout", "closing")   # the demo's option names (demo.py:241)
ALIASES = {"additive_noise": "additive noise", "low_resolution": "low resolution"}   # the command line's spellings
STREAM_CORRUPT = 14    # Philox stream id (inversion.py lists the others: 0-16)
HOLE_THRESH = 1e-8     # closing: `inv > 1e-8` is valid (demo.py:120)
MAX_PIXELS = 1 << 18   # dg_hole_fill


def canonical(name):
    """a corruption's name as CORRUPTIONS spells it (None stays None); ValueError for anything else"""
    if name is None:
        return None
    name = ALIASES.get(name, name)
    if name not in CORRUPTIONS:
        raise ValueError(f"{name!r}: one of {', '.join(CORRUPTIONS)}")
    return name


def _image(x, what):
    if not x.is_cuda:
        raise RuntimeError(f"{what} runs on the GPU only (no CPU fallback)")
    if x.dim() != 4 or x.shape[1] != 1:
        raise ValueError(f"{what}: a [B,1,H,W] image, got {tuple(x.shape)}")
    return x.detach().contiguous().float()


def _draw(kind, seed, first_index, like):
    """[B,1,H,W] Philox numbers (kind 0 uniform [0,1), 1 normal): row b from counter (first_index + b) ceil(HW / 4)"""
    B, _, H, W = like.shape
    HW = H * W
    out = torch.empty(B, 1, H, W, dtype=torch.float32, device=like.device)
    lib = L.lib()
    for b in range(B):
        L.check(lib.dg_philox_fill(int(seed), STREAM_CORRUPT, (int(first_index) + b) * ((HW + 3) // 4), kind, 0.0, 1.0, 0, 1, HW,
                                   L.ptr(out[b]), L.stream_ptr()), "dg_philox_fill")
    return out


def _mask(mask, what, row_keep=None, col_keep=None, u=None, rate=1.0):
    m = _image(mask, what)
    B, _, H, W = m.shape
    dev = m.device
    rk = None if row_keep is None else row_keep.to(device=dev, dtype=torch.float32).contiguous()
    ck = None if col_keep is None else col_keep.to(device=dev, dtype=torch.float32).contiguous()
    assert rk is None or rk.shape == (H,)
    assert ck is None or ck.shape == (W,)
    if u is not None:
        u = u.to(device=dev, dtype=torch.float32).contiguous()
        if u.numel() != m.numel():
            raise ValueError(f"{what}: u has {u.numel()} numbers for {m.numel()} pixels")
    out = torch.empty_like(m)
    L.check(L.lib().dg_corrupt_mask(L.ptr(m), L.ptr(rk), L.ptr(ck), L.ptr(u), float(rate), B, H, W, L.ptr(out), L.stream_ptr()),
            "dg_corrupt_mask")
    return out


def dropout_noise(mask, rate=0.5, u=None, *, seed=0, first_index=0):
    """demo.py:71-74: mask * (rand_like(mask) < rate) - a pixel is KEPT with probability `rate`"""
    m = _image(mask, "dropout_noise")
    if u is None:
        u = _draw(0, seed, first_index, m)
    return _mask(m, "dropout_noise", u=u, rate=rate)


def _every(n, rate):
    keep = torch.zeros(n)
    keep[::int(1 / rate)] = 1.0
    return keep


def sparse_hlines(mask, rate=0.5):
    """demo.py:77-81: rows ::int(1 / rate) stay"""
    return _mask(mask, "sparse_hlines", row_keep=_every(mask.shape[2], rate))


def sparse_vlines(mask, rate=0.5):
    """demo.py:84-88: columns ::int(1 / rate) stay"""
    return _mask(mask, "sparse_vlines", col_keep=_every(mask.shape[3], rate))


def random_rows(H, rate, seed=0):
    """the rows random_lines zeroes when none are given, in place of the demo's torch.randperm(H)[:int(H * (1 - rate))]: H
    int32 keys in [0, 2^31 - 1) from Philox (seed, STREAM_CORRUPT, counter 0, dg_philox_fill kind 3), the rows in a stable
    ascending order of their keys, the first int(H * (1 - rate)) of them"""
    keys = torch.empty(H, dtype=torch.int32, device="cuda")
    L.check(L.lib().dg_philox_fill(int(seed), STREAM_CORRUPT, 0, 3, 0.0, 1.0, 0, 2 ** 31 - 1, H, L.ptr(keys), L.stream_ptr()),
            "dg_philox_fill")
    perm = torch.sort(keys.cpu(), stable=True).indices
    return perm[: int(H * (1 - rate))]


def random_lines(mask, rate=0.5, rows=None, *, seed=0):
    """demo.py:91-95: int(H * (1 - rate)) rows are zeroed, the same rows in every sample; `rows` names them (random_rows)"""
    m = _image(mask, "random_lines")
    H = m.shape[2]
    if rows is None:
        rows = random_rows(H, rate, seed)
    keep = torch.ones(H)
    keep[torch.as_tensor(rows, dtype=torch.long).cpu()] = 0.0
    return _mask(m, "random_lines", row_keep=keep)


def corrupt_half(mask):
    """demo.py:98-101: columns W // 2 and above are zeroed"""
    W = mask.shape[3]
    keep = torch.ones(W)
    keep[W // 2:] = 0.0
    return _mask(mask, "corrupt_half", col_keep=keep)


def corrupt_quarter(mask):
    """demo.py:104-108: the first and the third quarter of the columns are zeroed"""
    W = mask.shape[3]
    keep = torch.ones(W)
    keep[: W // 4] = 0.0
    keep[W // 2: W * 3 // 4] = 0.0
    return _mask(mask, "corrupt_quarter", col_keep=keep)


def additive_noise(depth, strength=0.01, noise=None, *, seed=0, first_index=0):
    """demo.py:111-113: depth + randn_like(depth) * strength (two fp32 roundings, as torch's)"""
    x = _image(depth, "additive_noise")
    if noise is None:
        noise = _draw(1, seed, first_index, x)
    noise = noise.to(device=x.device, dtype=torch.float32).contiguous()
    if noise.numel() != x.numel():
        raise ValueError(f"additive_noise: noise has {noise.numel()} numbers for {x.numel()} pixels")
    out = torch.empty_like(x)
    L.check(L.lib().dg_additive_noise(L.ptr(x), L.ptr(noise), float(strength), x.numel(), L.ptr(out), L.stream_ptr()),
            "dg_additive_noise")
    return out


def median_blur3(x):
    """kornia.filters.median_blur(x, (3, 3)) (demo.py:117): zeros outside the image"""
    x = _image(x, "median_blur3")
    B, _, H, W = x.shape
    out = torch.empty_like(x)
    L.check(L.lib().dg_median3x3(L.ptr(x), B, H, W, L.ptr(out), L.stream_ptr()), "dg_median3x3")
    return out


def hole_fill_(x, thresh=HOLE_THRESH):
    """the `while` loop of closing (demo.py:118-123) on x [B,1,H,W] IN PLACE (dg_hole_fill) -> (sweeps [B], left [B]) int32"""
    if not (x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 1):
        raise ValueError("hole_fill_: a contiguous fp32 [B,1,H,W] image on the GPU")
    B, _, H, W = x.shape
    if H * W > MAX_PIXELS:
        raise ValueError(f"closing holds at most 2^18 pixels per scan, got {H}x{W}")
    tmp = torch.empty_like(x)
    sweeps = torch.empty(B, dtype=torch.int32, device=x.device)
    left = torch.empty_like(sweeps)
    L.check(L.lib().dg_hole_fill(L.ptr(x), L.ptr(tmp), B, H, W, float(thresh), L.ptr(sweeps), L.ptr(left), L.stream_ptr()),
            "dg_hole_fill")
    return sweeps, left


def closing(x, return_info=False):
    """demo.py:116-123: a 3x3 median, then holes (<= 1e-8) take the maximum of their 3x3 neighbourhood, sweep after sweep,
    until none is left.  Where the reference's loop never ends - a scan with no pixel above 1e-8 - the scan comes back as
    the median left it.  return_info: also {"sweeps": [B], "left": [B]} (int32, on the device)"""
    y = median_blur3(x)
    sweeps, left = hole_fill_(y)
    return (y, {"sweeps": sweeps, "left": left}) if return_info else y


def apply_corruption(depth, mask, corruption, *, seed=0, first_index=0, u=None, noise=None):
    """demo.py:126-137 on the normalised DEPTH and the mask (before invert_depth, as the demo applies it) -> (depth, mask).
    None returns the inputs themselves; otherwise the changed image is a new tensor and the inputs stay as they are."""
    corruption = canonical(corruption)
    if corruption is None:
        return depth, mask
    if corruption == "additive noise":
        depth = additive_noise(depth, 0.01, noise, seed=seed, first_index=first_index)
    elif corruption == "low resolution":
        mask = sparse_hlines(mask, 1 / 8)
    elif corruption == "dropout":
        mask = dropout_noise(mask, 0.1, u, seed=seed, first_index=first_index)
    elif corruption == "closing":
        depth = closing(depth)
        mask = torch.ones_like(_image(mask, "closing"))
    return depth, mask
