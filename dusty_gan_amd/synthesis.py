"""The library behind `python -m dusty_gan_amd.synthesize` -- reference: demo.py:188-234,265-338 (the demo's synthesis
mode) with utils/interp.py (lerp / slerp) and utils/geometry.py:5-35 (the view's rotation).

    latent_walk / sample_latents   the latents: random draws, or a lerp / slerp walk between two draws (dg_latent_walk)
    view                           zoom / yaw / pitch -> (R, t) of render_point_clouds
    synthesize                     latents -> utils.lidar.postprocess's dict, in full batches
    export_points / write_bins     inverse depth -> packed KITTI records on the device (dg_export_points) -> .bin files

GPU only: CPU tensors raise, like utils/lidar.py.  The kernels are in csrc/synthesis.hip."""
import math
import os

import torch

from . import _lib as L

MODES = {"lerp": 0, "slerp": 1}
LATENT_TYPES = ("random", "lerp", "slerp")


def _gpu(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"{what} runs on the GPU only (no CPU fallback)")
    return t.contiguous().float()


def latent_walk(z0, z1, n, mode="slerp"):
    """utils/interp.py:4-16 at w = torch.linspace(0, 1, n): z0, z1 [nz] (or [1,nz]) -> [n, nz].  ValueError when the result
    is not finite: endpoints on one line under slerp (the reference returns NaN there)."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    z0, z1 = _gpu(z0, "latent_walk").reshape(-1), _gpu(z1, "latent_walk").reshape(-1)
    if z0.shape != z1.shape:
        raise ValueError(f"endpoints of different sizes: {tuple(z0.shape)} and {tuple(z1.shape)}")
    n, nz = int(n), z0.numel()
    if n < 1 or nz < 1:
        raise ValueError(f"latent_walk needs n >= 1 and nz >= 1, got n={n}, nz={nz}")
    out = torch.empty(n, nz, dtype=torch.float32, device=z0.device)
    L.check(L.lib().dg_latent_walk(L.ptr(z0), L.ptr(z1), n, nz, MODES[mode], L.ptr(out), L.stream_ptr()), "dg_latent_walk")
    if not bool(torch.isfinite(out).all()):
        raise ValueError(f"{mode} between these endpoints is not finite (parallel or antipodal endpoints have no arc)")
    return out


def sample_latents(cfg, device, n, latent="random", seed=0):
    """[n, in_ch] latents (demo.py:278-293).  "random": n rows of Philox(seed, device).normal, the stream
    evaluate_synthesis.synthetic_2d draws from; "lerp" / "slerp": the walk between the first two rows of that draw."""
    from .utils.rng import Philox
    if latent not in LATENT_TYPES:
        raise ValueError(f"latent must be one of {LATENT_TYPES}, got {latent!r}")
    n, nz = int(n), int(cfg.model.gen.in_ch)
    if n < 1:
        raise ValueError(f"n must be at least 1, got {n}")
    rng = Philox(seed, device)
    if latent == "random":
        return rng.normal(n * nz).view(n, nz)
    ends = rng.normal(2 * nz).view(2, nz)
    return latent_walk(ends[0], ends[1], n, latent)


def view(zoom_m=60, yaw_deg=-45, pitch_deg=60):
    """demo.py:188-226 -> (R [3,3], t [3]) float32 CPU tensors for render_point_clouds: t = (0.1 z, 0, z) with
    z = zoom / 120; R = Rz Ry Rx of the angles (0, pitch, -yaw) in radians (utils/geometry.py:5-35).  Float64 arithmetic on
    three numbers, stored as float32."""
    t_z = float(zoom_m) / 120.0
    ax, ay, az = 0.0, float(pitch_deg) / 180.0 * math.pi, -float(yaw_deg) / 180.0 * math.pi
    R_x = torch.tensor([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]], dtype=torch.float64)
    R_y = torch.tensor([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]], dtype=torch.float64)
    R_z = torch.tensor([[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0], [0, 0, 1]], dtype=torch.float64)
    R = R_z @ (R_y @ R_x)
    return R.float(), torch.tensor([0.1 * t_z, 0.0, t_z], dtype=torch.float64).float()


def generate(cfg, G, latents):
    """G's raw outputs for the rows of `latents`, in full `solver.batch_size` batches: a short last batch is filled up with
    zero rows and cut again (evaluate_synthesis.synthetic_2d); the outputs are views of G's workspace, so they are cloned"""
    latents = _gpu(latents, "synthesize")
    B, n = int(cfg.solver.batch_size), len(latents)
    chunks = []
    for i in range(0, n, B):
        z = torch.zeros(B, latents.shape[1], device=latents.device)
        k = len(latents[i:i + B])
        z[:k] = latents[i:i + B]
        chunks.append({key: value[:k].clone() for key, value in G(latent=z).items()})
    return {key: torch.cat([c[key] for c in chunks], dim=0) for key in chunks[0]}


def synthesize(cfg, G, lidar, latents, tol=0.0, normals=True):
    """demo.py:295-296: latents [n, in_ch] -> utils.lidar.postprocess's dict for all n rows ("depth", "points", "normals"
    and, per architecture, "depth_orig", "confidence", "mask").  normals=False leaves the normal image out."""
    from .utils import lidar as U
    raw = generate(cfg, G, latents)
    if normals:
        return U.postprocess(raw, lidar, tol=tol)
    out = dict(raw)
    for key, mode in (("depth_orig", 0), ("confidence", 1)):
        if key in out:
            out[key] = U.unit_map(out[key], mode)
    out["points"], out["depth"] = lidar.inv_to_xyz(raw["depth"], tol, from_tanh=True, return_depth=True)
    return out


def export_points(inv, lidar, tol=0.0, from_tanh=True):
    """inverse depth [B,1,H,W] (the generator's "depth" in [-1,1]; from_tanh=False: [0,1], postprocess's) ->
    (records [B, H W, 4] float32, counts [B] int32) on the device: records[b, :counts[b]] are the KITTI records
    (x, y, z, 0) in metres of scan b's valid pixels in row-major order - LiDAR.inv_to_xyz(inv, tol, from_tanh) * max_depth
    at the pixels that function keeps.  Rows at and beyond counts[b] are not written."""
    if lidar.angle is None:
        raise RuntimeError(f"no angle grid: {lidar.angle_file!r} does not exist (utils/lidar.py:120)")
    x = _gpu(inv, "export_points")
    B, _, H, W = x.shape
    assert (H, W) == (lidar.H, lidar.W) and x.shape[1] == 1, x.shape
    if lidar.angle.device != x.device:
        lidar.to(x.device)
    HW = H * W
    records = torch.empty(B, HW, 4, dtype=torch.float32, device=x.device)
    counts = torch.empty(B, dtype=torch.int32, device=x.device)
    chunk_counts = torch.empty(B * (-(-HW // L.EXPORT_CHUNK)), dtype=torch.int32, device=x.device)
    L.check(L.lib().dg_export_points(L.ptr(x), L.ptr(lidar.angle), B, H, W, int(from_tanh), lidar.min_depth,
                                     lidar.max_depth, lidar.drop_const, float(tol), L.ptr(chunk_counts), L.ptr(records),
                                     L.ptr(counts), L.stream_ptr()), "dg_export_points")
    return records, counts


def bin_path(dir, index):
    return os.path.join(dir, "{:06d}.bin".format(int(index)))


def write_bins(records, counts, dir, first_index=0, names=None):
    """records [B,HW,4], counts [B] -> dir/<first_index + b:06d>.bin (or dir/<names[b]>.bin), counts[b] * 4 little-endian
    float32 each (what np.fromfile(path, np.float32).reshape(-1, 4) reads back); only records[b, :counts[b]] is copied to
    the host.  Returns the paths."""
    os.makedirs(dir, exist_ok=True)
    paths = []
    for b, k in enumerate(counts.tolist()):
        path = bin_path(dir, first_index + b) if names is None else os.path.join(dir, f"{names[b]}.bin")
        records[b, :int(k)].detach().cpu().contiguous().numpy().astype("<f4", copy=False).tofile(path)
        paths.append(path)
    return paths
