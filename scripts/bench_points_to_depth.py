"""Event time of one LiDAR.points_to_depth call (dg_points_to_depth: search + finish) on the nominal 64x1024 grid, N points
per cloud drawn uniformly over the grid's field of view at 2 .. 100 m, for B = 1 and B = 16.
    python scripts/bench_points_to_depth.py [--points 131072] [--batches 1 16] [--reps 10]
`warm` untimed calls, then `reps` calls each between two device events; median and minimum, and the shader clock read
right after the timed calls (scripts/bench_inversion.py's way).  Prints one JSON line per batch size."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from scripts.bench_inversion import gpu_clock  # noqa: E402


def cloud(B, N, lidar, seed=0):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.rand(B, N, device="cuda", generator=gen) * math.radians(26.8) - math.radians(24.8)
    v = (torch.rand(B, N, device="cuda", generator=gen) * 2 - 1) * math.pi
    d = (torch.rand(B, N, device="cuda", generator=gen) * 98 + 2) / lidar.max_depth
    return torch.stack([d * u.cos() * v.cos(), d * u.cos() * v.sin(), d * u.sin(), torch.zeros_like(d)], dim=-1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=131072)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 16])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    a = ap.parse_args()
    from dusty_gan_amd.utils.lidar import LiDAR
    lidar = LiDAR(64, 1024, 0.9, 120.0).use_nominal_angles().to("cuda")
    for B in a.batches:
        rec = cloud(B, a.points, lidar)
        times = []
        for r in range(a.warm + a.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            depth, valid = lidar.points_to_depth(rec)
            e1.record()
            torch.cuda.synchronize()
            if r >= a.warm:
                times.append(e0.elapsed_time(e1))
        clock = gpu_clock()
        med = sorted(times)[len(times) // 2]
        pairs = float(B) * a.points * lidar.H * lidar.W
        print(json.dumps({"what": "points_to_depth, one call, ms", "grid": [lidar.H, lidar.W], "B": B, "N": a.points,
                          "median": round(med, 3), "min": round(min(times), 3), "ms_per_cloud": round(med / B, 3),
                          "pairs_per_s": round(pairs / (med * 1e-3), -9), "lit": round(float(valid.float().mean()), 3),
                          "sclk_mhz": clock}), flush=True)


if __name__ == "__main__":
    main()
