#!/usr/bin/env python3
"""Timing of the closing corruption (dusty_gan_amd.corruption.closing: dg_median3x3 + dg_hole_fill) on
B scans of 64x1024 with the synthetic dataset's validity rate (Bernoulli(0.85), utils/synthetic.py).
usage: python scripts/bench_corruption.py [--scans 512] [--keep 0.85] [--reps 20] [--warm 3] [--out FILE]
After `warm` untimed calls, `reps` calls each timed with its own event pair; prints one JSON line with the median (and the
p10 / p90) in ms of the whole closing and of the hole fill alone, and the sweep counts."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": round(float(np.median(ms)), 4), "p10_ms": round(float(np.percentile(ms, 10)), 4),
            "p90_ms": round(float(np.percentile(ms, 90)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=512)
    ap.add_argument("--keep", type=float, default=0.85)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from dusty_gan_amd import corruption as K
    g = torch.Generator(device="cuda").manual_seed(0)
    shape = (args.scans, 1, 64, 1024)
    valid = (torch.rand(shape, device="cuda", generator=g) < args.keep).float()
    depth = (0.05 + 0.9 * torch.rand(shape, device="cuda", generator=g)) * valid
    _, info = K.closing(depth, return_info=True)
    sweeps = info["sweeps"].cpu()
    med = K.median_blur3(depth)
    work = torch.empty_like(med)

    def fill():
        work.copy_(med)
        K.hole_fill_(work)

    res = {"scans": args.scans, "shape": [64, 1024], "keep": args.keep, "reps": args.reps,
           "sweeps_min": int(sweeps.min()), "sweeps_median": int(sweeps.median()), "sweeps_max": int(sweeps.max()),
           "left_total": int(info["left"].sum()),
           "closing": timed(lambda: K.closing(depth), args.warm, args.reps),
           "copy_plus_hole_fill": timed(fill, args.warm, args.reps),
           "copy": timed(lambda: work.copy_(med), args.warm, args.reps)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
