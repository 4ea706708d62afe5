"""The picture log's renderers -- reference: utils/render.py:18-127 (render_point_clouds, bilinear_rasterizer),
utils/__init__.py `flatten` and `colorize`, train.py:28-34 (log_imgs: make_grid, colorize, TensorBoard's byte conversion).

All arithmetic is in csrc/render.hip.  The splatted sums are 64-bit fixed point added with integer atomics, so an image
does not depend on the order of its points; the words live in a workspace per (device, stream, size) that is zero at
rest: dg_splat_finish leaves it so, and a call that fails between the two launches zeroes it before it raises.  Work on one
stream is ordered, so two renders never share words in flight; a workspace is not meant to be used from two host threads
at once.  GPU only: CPU tensors raise, like utils/lidar.py.  A point with a non-finite coordinate is skipped (the
reference's `.long()` of NaN is undefined).  Values are range-checked: the fixed point's window (common.h dg_fix40) holds
|value| <= 8, and anything larger (infinities too) raises ValueError instead of wrapping or being left out silently;
a NaN value's terms are left out, like a NaN coordinate's.
"""
import torch

from .. import _lib as _L   # (render_point_clouds' own parameter is called L, as in the reference)

VALUE_MAX = 8.0   # dg_fix40's range analysis: |value| <= 8 keeps a pixel's total inside the 64-bit word

_words = {}   # (device index, stream, numel) -> int64 words, all zero between calls
_luts = {}    # device index -> the turbo table [256,3] float32 on that device


def _workspace(device, numel):
    index = device.index if device.index is not None else torch.cuda.current_device()
    key = (index, _L.stream_ptr(), int(numel))
    if key not in _words:
        _words[key] = torch.zeros(int(numel), dtype=torch.int64, device=device)
    return _words[key]


def _in_range(t, what):
    if bool((t.abs() > VALUE_MAX).any()):   # (a NaN passes: its terms are left out, like a NaN coordinate's)
        raise ValueError(f"{what}: values must lie within +-{VALUE_MAX:g} (the fixed-point sum's window)")


def _gpu(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"{what} runs on the GPU only (no CPU fallback)")
    return t.contiguous().float()


def flatten(tensor_BCHW):
    """utils/__init__.py: [B,C,H,W] -> [B,H W,C]"""
    return tensor_BCHW.flatten(2).permute(0, 2, 1).contiguous()


def _splat(accumulate, what, B, C, H, W, normalize, device):
    """accumulate(words) then dg_splat_finish -> float [B,C,H,W]; whatever fails, the words are zero again afterwards"""
    out = torch.empty(B, C, H, W, dtype=torch.float32, device=device)
    acc = _workspace(device, B * H * W * C)
    try:
        _L.check(accumulate(_L.ptr(acc)), what)
        _L.check(_L.lib().dg_splat_finish(_L.ptr(acc), B, C, H, W, int(normalize), _L.ptr(out), _L.stream_ptr()), "dg_splat_finish")
    except BaseException:
        acc.zero_()
        raise
    return out


def bilinear_rasterizer(coords, values, out_shape):
    """render.py:67-127: coords [B,N,2] (coordinate 0 = row), values [B,N,C], C <= 4 -> [B,C,H,W]"""
    coords, values = _gpu(coords, "bilinear_rasterizer"), _gpu(values, "bilinear_rasterizer")
    B, N, C = values.shape
    H, W = (int(v) for v in out_shape)
    assert coords.shape == (B, N, 2) and 1 <= C <= 4, (coords.shape, values.shape)
    _in_range(values, "bilinear_rasterizer")
    return _splat(lambda acc: _L.lib().dg_splat_accum(_L.ptr(coords), _L.ptr(values), B, N, C, H, W, acc, _L.stream_ptr()),
                  "dg_splat_accum", B, C, H, W, False, values.device)


def render_point_clouds(xyz, normals, L=512, R=None, t=None, focal_length=1.0):
    """render.py:18-64: xyz, normals [B,N,3] -> the bird's-eye view [B,3,L,L] (a channel slice of the [B,4,L,L] image whose
    last channel is the splatted weight).  The inputs are not modified."""
    xyz, normals = _gpu(xyz, "render_point_clouds"), _gpu(normals, "render_point_clouds")
    B, N, _ = xyz.shape
    assert xyz.shape == (B, N, 3) and normals.shape == (B, N, 3), (xyz.shape, normals.shape)
    size = int(L)
    if R is not None:
        assert R.shape[-2:] == (3, 3) and R.numel() in (9, 9 * B), R.shape
        R = _gpu(R, "render_point_clouds")
    if t is not None:
        assert t.shape[-1:] == (3,) and t.numel() in (3, 3 * B), t.shape
        t = _gpu(t, "render_point_clouds")
    _in_range(normals, "render_point_clouds (normals; the weights are at most 1)")
    return _splat(lambda acc: _L.lib().dg_render_points(_L.ptr(xyz), _L.ptr(normals), B, N, size, _L.ptr(R),
                                                        int(R is not None and R.numel() == 9 * B and B > 1), _L.ptr(t),
                                                        int(t is not None and t.numel() == 3 * B and B > 1),
                                                        float(focal_length), acc, _L.stream_ptr()),
                  "dg_render_points", B, 4, size, size, True, xyz.device)[:, :3]


def grid_shape(B, H, W):
    """(Hg, Wg) of torchvision.utils.make_grid(nrow=4, padding=2) for B images of H x W"""
    xmaps = min(4, B)
    ymaps = -(-B // xmaps)
    return ymaps * (H + 2) + 2, xmaps * (W + 2) + 2


def image_grid(tensor, color=True, scale=1.0):
    """train.py:28-34 (log_imgs) up to the writer: [B,1|3,H,W] float times `scale` -> uint8 [Hg,Wg,3] on the device, laid out
    as make_grid(nrow=4); color: channel 0 through Normalize(0,1) + turbo (the padding too), else plain."""
    if not (isinstance(tensor, torch.Tensor) and tensor.is_cuda):
        raise RuntimeError("image_grid runs on the GPU only (no CPU fallback)")
    assert tensor.ndim == 4 and tensor.shape[1] in (1, 3), tensor.shape
    x = tensor.detach().float()
    B, C, H, W = x.shape
    if not (x[0].is_contiguous() and (B == 1 or x.stride(0) >= C * H * W)):
        x = x.contiguous()
    Hg, Wg = grid_shape(B, H, W)
    out = torch.empty(Hg, Wg, 3, dtype=torch.uint8, device=x.device)
    _L.check(_L.lib().dg_image_grid(_L.ptr(x), x.stride(0) if B > 1 else C * H * W, B, C, H, W, float(scale), int(bool(color)),
                                  _L.ptr(out), _L.stream_ptr()), "dg_image_grid")
    return out


def turbo_lut():
    """the 256 x 3 turbo table compiled into the library (csrc/turbo_lut.h) as a CPU tensor; needs no device"""
    import ctypes as C
    buf = (C.c_float * 768)()
    _L.check(_L.lib().dg_turbo_lut(buf), "dg_turbo_lut")
    return torch.tensor(list(buf), dtype=torch.float32).view(256, 3)


def colorize(tensor, cmap="turbo"):
    """utils/__init__.py:194-210 (utils.colorize): [B,1,H,W] or [B,H,W] in [0,1] -> [B,3,H,W] through the turbo table, index
    round(255 x) of the clamped value.  (The reference clamps its argument in place; here the argument is left alone.)"""
    if cmap != "turbo":
        raise NotImplementedError(cmap)
    if not (isinstance(tensor, torch.Tensor) and tensor.is_cuda):
        raise RuntimeError("colorize runs on the GPU only (no CPU fallback)")
    if tensor.ndim == 4:
        assert tensor.shape[1] == 1, f"expected (B,1,H,W) tensor, but got {tensor.shape}"
        tensor = tensor.squeeze(1)
    assert tensor.ndim == 3, f"got {tensor.ndim}!=3"
    index = torch.round(tensor.clamp(0, 1) * 255.0).long()
    key = tensor.device.index if tensor.device.index is not None else torch.cuda.current_device()
    if key not in _luts:
        _luts[key] = turbo_lut().to(tensor.device)
    return _luts[key].to(tensor.dtype)[index].permute(0, 3, 1, 2)
