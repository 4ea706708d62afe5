#!/usr/bin/env python3
"""The any-sensor projection beside the KITTI-order one on one MI355X: dg_elev_hist, dg_beam_project and
dg_scan_project on the SAME device-resident records - 16 seeded scans of 64 rings x ~1900 points (bench_process_kitti's) at
64 x 2048 - timed with HIP events, the median of --reps graph-free calls after warm-up, per scan, with the bytes each must move
(histogram: the points in; projections: points in, keys once, projection out) against the HBM rate.  dg_beam_project is also
timed on the records of every scan shuffled: no file order to lean on.  One JSON line.
usage: python scripts/bench_beam_project.py [--chunk 16] [--reps 50] [--out profiles/beam_project.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_process_kitti import HBM_GBPS, ROOT, make_scan, median_us  # noqa: E402

sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=16, help="scans per launch")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3, help="the four timings alternate this many times; the median is reported")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from dusty_gan_amd import _lib as L
    from dusty_gan_amd.datasets import beams as B
    from dusty_gan_amd.datasets import raw
    H, W, S, NB = 64, 2048, args.chunk, B.NB_DEFAULT
    rng = np.random.default_rng(0)
    scans = [make_scan(rng) for _ in range(S)]
    dev = torch.device("cuda")
    o = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)
    pts = torch.from_numpy(np.concatenate(scans)).to(dev)
    shuffled = torch.from_numpy(np.concatenate([s[rng.permutation(len(s))] for s in scans])).to(dev)
    offs = torch.from_numpy(o).to(dev)
    keys = torch.empty(S * H * W, dtype=torch.int64, device=dev)
    status = torch.empty(S, dtype=torch.int32, device=dev)
    out = torch.empty(S, H, W, 4, dtype=torch.float32, device=dev)
    hist = torch.zeros(NB, dtype=torch.int64, device=dev)
    lo, hi = -np.pi / 2, np.pi / 2
    B._add_hist(pts, offs, S, 0.9, 120.0, lo, hi, hist)
    table = B.estimate_beams(hist.cpu().numpy(), H, lo, hi)
    calls = {"elev_hist": lambda: B._add_hist(pts, offs, S, 0.9, 120.0, lo, hi, hist),
             "beam_project": lambda: raw._launch_beam_project(pts, offs, S, table, W, keys, None, out),
             "beam_project_shuffled": lambda: raw._launch_beam_project(shuffled, offs, S, table, W, keys, None, out),
             "scan_project": lambda: raw._launch_project(pts, offs, S, W, keys, status, None, out)}
    runs = {name: [] for name in calls}
    for _ in range(args.rounds):   # the four alternate, so a drifting clock or a busy neighbour shows as spread in each
        for name, fn in calls.items():
            runs[name].append(median_us(fn, args.reps) / S)
    n_pts = float(o[-1]) / S
    proj_bytes, hist_bytes = n_pts * 16 + H * W * (8 + 16), n_pts * 16

    def rate(name, nbytes):
        us = float(np.median(runs[name]))
        return {"us_per_scan": round(us, 2), "rounds_us": [round(v, 2) for v in runs[name]], "GBps": round(nbytes / us / 1e3, 1),
                "frac_of_8TBps": round(nbytes / us / 1e3 / HBM_GBPS, 4)}
    res = {name: rate(name, hist_bytes if name == "elev_hist" else proj_bytes) for name in calls}
    res.update({"beam_over_scan": round(res["beam_project"]["us_per_scan"] / res["scan_project"]["us_per_scan"], 2),
                "points_per_scan": int(n_pts), "chunk": S, "reps": args.reps, "rounds": args.rounds, "NB": NB,
                "table_error_deg": round(float(np.abs(np.rad2deg(table) - np.linspace(2.0, -24.8, H)).max()), 4),
                "lib": L.lib().dg_version().decode()})
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
