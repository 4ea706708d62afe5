#!/usr/bin/env python3
"""Training rate on three data sources in one process: the synthetic device pool, the file loader (datasets/scans.py) and the
resident scan store (dataset.resident: true, datasets/resident.py).

Writes N projected scans (64 x 2048 x 4 fp32, 2 MB each, like process_kitti.py's output) into a scratch directory, builds one
trainer per source (arch none, bf16, hipGraph replay, 64 x 1024, 32 images per step by default) and times them in alternating
rounds.  Prints one JSON line: steps/s and images/s per source (median over rounds), and the resident store's bytes and build
time (GB/s of raw scans read).
usage: python scripts/bench_resident.py [--n 512] [--batch 32] [--width 1024] [--steps 40] [--rounds 3] [--only SOURCE]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SOURCES = ("synthetic", "files", "resident")


def make(source, root, args):
    from dusty_gan_amd.trainers.dcgan_amp import Trainer
    from dusty_gan_amd.utils.config import load_config
    H, W = 64, args.width
    ov = ["model=dcgan_eqlr", f"dataset.shape=[{H},{W}]", f"solver.batch_size={args.batch}", "enable_amp=true"]
    if source == "synthetic":
        ov = ["dataset=synthetic"] + ov
    else:
        ov = ["dataset=kitti_odometry", f"dataset.root={root}", f"dataset.flip={str(args.flip).lower()}",
              f"dataset.resident={str(source == 'resident').lower()}"] + ov
    torch.manual_seed(1234)
    t0 = time.perf_counter()
    tr = Trainer(load_config(ov), {"gpu": 0, "ngpus": 1, "batch_size": args.batch, "num_workers": args.workers})
    return tr, time.perf_counter() - t0


def timed(tr, steps, i0):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        tr.step(i0 + i)
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512, help="scans written (the train split)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--workers", type=int, default=8, help="host reader threads of the file loader")
    ap.add_argument("--flip", action="store_true", help="dataset.flip (stores both variants)")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--steps", type=int, default=40, help="timed steps per source per round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=SOURCES, default=None, help="one source (a kernel-trace run of its own)")
    args = ap.parse_args()
    Hs, Ws = 64, 2048
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as root:
        d = os.path.join(root, "sequences", "00", "velodyne")
        os.makedirs(d)
        for i in range(args.n):
            np.save(os.path.join(d, f"{i:06d}.npy"), rng.normal(0, 20, (Hs, Ws, 4)).astype(np.float32))
        sources = (args.only,) if args.only else SOURCES
        trs, out = {}, {"n_scans": args.n, "batch": args.batch, "shape": [64, args.width], "flip": args.flip,
                        "precision": "bf16", "arch": "none"}
        for s in sources:
            trs[s], secs = make(s, root, args)
            if s == "resident":
                st = trs[s]._scan_loader
                out["resident_store_bytes"] = st.nbytes
                out["resident_build_s"] = round(st.build_seconds, 3)
                out["resident_build_raw_GBps"] = round(st.raw_bytes / st.build_seconds / 1e9, 3)
                out["resident_trainer_init_s"] = round(secs, 3)
            timed(trs[s], args.warmup, 0)   # warm-up, capture
            assert trs[s]._graph is not None, s
        rates = {s: [] for s in sources}
        for r in range(args.rounds):
            for s in sources:
                rates[s].append(timed(trs[s], args.steps, args.warmup + r * args.steps))
        for s in sources:
            sps = statistics.median(rates[s])
            out[s] = {"steps_per_s": round(sps, 2), "images_per_s": round(sps * args.batch, 1),
                      "rounds_steps_per_s": [round(v, 2) for v in rates[s]]}
        if "synthetic" in out and "resident" in out:
            out["resident_vs_synthetic"] = round(out["resident"]["images_per_s"] / out["synthetic"]["images_per_s"], 4)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
