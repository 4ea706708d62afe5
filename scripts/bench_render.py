"""Time the picture log's renderer (csrc/render.hip) next to the same arithmetic as whole-array torch ops on the same GPU.

    python scripts/bench_render.py [--out profiles/render.json]

  * render_us        render_point_clouds at B = 8, 64 x 1024 points per cloud, L = 512 (dg_render_points + dg_splat_finish)
  * torch_ops_us     the reference's formulation (float32 temporaries, four scatter-adds per channel set) in torch on the device
  * image_log_ms     one image-log event of a dusty2 run at that size: the bird's-eye view, nine grids, their copies to the host
Medians of 30 timed repetitions after 5 warm-up ones, device events around each repetition.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dusty_gan_amd.utils.render import image_grid, render_point_clouds  # noqa: E402


def torch_ops_render(xyz, normals, L, t):
    """render_point_clouds as whole-array float32 torch ops with float scatter-adds (arrival-order sums)"""
    p = xyz * torch.tensor([1.0, 1.0, -1.0], device=xyz.device) + t
    uv = (p[..., :2] / p[..., 2:3] + 0.5) * L
    inside = ((uv > 0) & (uv < L - 1)).all(-1, keepdim=True)
    depth = p.norm(dim=-1, keepdim=True)
    weight = torch.exp(-3.0 * depth) * (depth > 1e-8)
    values = torch.cat([weight * normals * inside, weight], -1)
    pos = L - uv
    lo = torch.floor(pos)
    frac = pos - lo
    B, N, C = values.shape
    out = torch.zeros(B, L * L, C, device=xyz.device)
    for dh in (0, 1):
        for dw in (0, 1):
            cell = lo + torch.tensor([dh, dw], device=xyz.device)
            safe = cell.clamp(0, L - 1)
            side = torch.where(torch.tensor([dh, dw], device=xyz.device).bool(), frac, 1 - frac) * (cell == safe)
            wt = side[..., 0] * side[..., 1]
            wt = wt * (wt >= 1e-3)
            index = (safe[..., 0] * L + safe[..., 1]).long()
            out.scatter_add_(1, index[..., None].expand(-1, -1, C), values * wt[..., None])
    out = out.view(B, L, L, C).permute(0, 3, 1, 2)
    return out[:, :3] / (out[:, 3:] + 1e-8)


def timed(fn, reps=30, warmup=5):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render.json"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    B, H, W, L = 8, 64, 1024, 512
    gen = torch.Generator(device=dev).manual_seed(0)
    # a synthetic scan: rays of the nominal angle grid at random depths, 15 % dropped
    pitch = torch.linspace(0.035, -0.433, H, device=dev)[:, None].expand(H, W)
    yaw = torch.linspace(3.14, -3.14, W, device=dev)[None].expand(H, W)
    unit = torch.stack([pitch.cos() * yaw.cos(), pitch.cos() * yaw.sin(), pitch.sin()], -1).view(1, H * W, 3)
    depth = torch.rand(B, H * W, 1, device=dev, generator=gen) * 0.5 + 0.02
    depth = depth * (torch.rand(B, H * W, 1, device=dev, generator=gen) > 0.15)
    xyz, normals = (unit * depth).contiguous(), torch.rand(B, H * W, 3, device=dev, generator=gen)
    t = torch.tensor([0.0, 0.0, 0.5], device=dev)
    a, b = render_point_clouds(xyz, normals, L=L, t=t), torch_ops_render(xyz, normals, L, t)
    diff = float((a - b).abs().max())
    render = timed(lambda: render_point_clouds(xyz, normals, L=L, t=t))
    ops = timed(lambda: torch_ops_render(xyz, normals, L, t))
    maps = {k: torch.rand(B, c, H, W, device=dev, generator=gen) for k, c in
            (("depth", 1), ("depth_orig", 1), ("normals", 3), ("confidence", 2), ("mask", 2))}

    def log_event():
        grids = [image_grid(render_point_clouds(xyz, normals, L=L, t=t), color=False),
                 image_grid(maps["depth"], scale=2.5), image_grid(maps["depth_orig"], scale=2.5),
                 image_grid(maps["normals"], color=False)]
        for k in ("confidence", "mask"):
            grids += [image_grid(maps[k][:, 0:1], color=k == "confidence"), image_grid(maps[k][:, 1:2], color=k == "confidence")]
        grids.append(image_grid(maps["mask"].prod(1, keepdim=True), color=False))
        return [g.cpu() for g in grids]

    event = timed(log_event, reps=10, warmup=2)
    res = {"device": torch.cuda.get_device_name(0), "B": B, "points_per_cloud": H * W, "L": L,
           "render_us": {"median": render[0], "min": render[1], "max": render[2]},
           "torch_ops_us": {"median": ops[0], "min": ops[1], "max": ops[2]},
           "max_abs_diff_render_vs_torch_ops": diff,
           "image_log_ms": {"median": event[0] / 1e3, "min": event[1] / 1e3, "max": event[2] / 1e3}}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
