#!/usr/bin/env python3
"""Raw scans -> dataset files on one MI355X box: kernel time, end-to-end rate, and the same work in numpy.

Makes its own seeded raw scans (64 rings x ~1900 points, the size of a KITTI sweep) as `.bin` files in a scratch directory,
then reports one JSON line:
  * project_us_per_scan / angles_us_per_scan: dg_scan_project (fill + scatter + gather) and dg_angle_accum on device-resident
    chunks, graph-free launches timed with HIP events, the MEDIAN of --reps runs after warm-up, per scan; against the bytes
    the kernels must move per scan (points in, keys once, projection out; for the angle sums the projection in) and the
    HBM rate (8 TB/s);
  * end_to_end_scans_per_s: `.bin` -> `.npy` through datasets.raw.project_files (host threads, pinned slots, both copies);
  * numpy_scans_per_s: a plain numpy restatement of process_point_clouds (argsort + fancy-index scatter, arrays in memory,
    nothing written) on --cpu-threads host threads;
  * clock_ghz: the clock the chip holds (scripts/conv_clock.py on the diagnostic library, a child process; null without it).
usage: python scripts/bench_process_kitti.py [--n 64] [--chunk 16] [--workers 8] [--reps 50] [--out profiles/process_kitti.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_GBPS = 8000.0


def make_scan(rng, rings=64, per_ring=1900):
    n = per_ring + rng.integers(-40, 41, rings)
    th = np.concatenate([np.sort(rng.uniform(0.001, 2 * np.pi - 0.001, k)) for k in n])
    phi = np.repeat(np.deg2rad(np.linspace(2.0, -24.8, rings)), n) + rng.normal(0, 5e-4, th.size)
    r = rng.uniform(2.0, 80.0, th.size)
    xyz = np.stack([r * np.cos(phi) * np.cos(th), r * np.cos(phi) * np.sin(th), r * np.sin(phi)], -1)
    return np.concatenate([xyz, rng.random((th.size, 1))], -1).astype(np.float32)


def numpy_project(points, H=64, W=2048):
    """process_point_clouds (process_kitti.py:76-118) restated with whole-array numpy operations"""
    x, y = points[:, 0], points[:, 1]
    depth = np.linalg.norm(points[:, :3], ord=2, axis=1)
    order = np.argsort(-depth)
    quads = np.where(x >= 0, np.where(y >= 0, 0, 3), np.where(y >= 0, 1, 2))
    starts = (np.roll(quads, 1) - quads) == 3
    c = np.cumsum(starts)
    rows = np.where(c == 0, 0, H - int(c[-1]) + c - 1)
    cols = np.floor((-np.arctan2(y, x) / np.float32(np.pi) + 1) / 2 % 1 * W).astype(np.int32)
    proj = np.zeros((H, W, 4), dtype=np.float32)
    proj[rows[order], cols[order]] = points[order]   # repeated indices: the last (nearest) write stays
    return proj


def median_us(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts))


def held_clock():
    if not os.path.exists(os.path.join(ROOT, "dusty_gan_amd", "csrc", "libdustygan_hip_diag.so")):
        return None
    env = dict(os.environ, DUSTY_GAN_LIB_DIAG="1")
    try:
        res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "conv_clock.py"), "2"], capture_output=True,
                             text=True, timeout=120, env=env)
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
        return json.loads(line[-1]).get("clock_ghz") if res.returncode == 0 and line else None
    except Exception:  # noqa: BLE001
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64, help="raw scans written")
    ap.add_argument("--chunk", type=int, default=16, help="scans per launch")
    ap.add_argument("--workers", type=int, default=8, help="host threads of the file pipeline")
    ap.add_argument("--cpu-threads", type=int, default=16, help="host threads of the numpy restatement")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--passes", type=int, default=3, help="timed passes of the file pipeline over the scans")
    ap.add_argument("--no-clock", action="store_true")
    ap.add_argument("--out", type=str, default=None, help="also write the result here (e.g. profiles/process_kitti.json)")
    args = ap.parse_args()
    from dusty_gan_amd import _lib as L
    from dusty_gan_amd.datasets import raw
    W, S = 2048, args.chunk
    rng = np.random.default_rng(0)
    scans = [make_scan(rng) for _ in range(args.n)]
    dev = torch.device("cuda")
    # ---- kernels on device-resident chunks
    pts = torch.from_numpy(np.concatenate(scans[:S])).to(dev)
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s) for s in scans[:S]])]).astype(np.int64)).to(dev)
    keys = torch.empty(S * 64 * W, dtype=torch.int64, device=dev)
    status = torch.empty(S, dtype=torch.int32, device=dev)
    out = torch.empty(S, 64, W, 4, dtype=torch.float32, device=dev)
    proj_us = median_us(lambda: raw._launch_project(pts, offs, S, W, keys, status, None, out), args.reps) / S
    acc = raw.AngleAccumulator(64, W, dev)
    ang_us = median_us(lambda: acc.add(out), args.reps) / S
    n_pts = float(np.mean([len(s) for s in scans[:S]]))
    proj_bytes = n_pts * 16 + 64 * W * (8 + 16)
    ang_bytes = 64 * W * 16
    # ---- .bin -> .npy
    with tempfile.TemporaryDirectory() as root:
        src = os.path.join(root, "dataset/sequences/00/velodyne")
        os.makedirs(src)
        for i, s in enumerate(scans):
            s.tofile(os.path.join(src, f"{i:06d}.bin"))
        pairs = [(os.path.join(src, f"{i:06d}.bin"), os.path.join(root, "dusty-gan/sequences/00/velodyne", f"{i:06d}.npy"))
                 for i in range(args.n)]
        raw.project_files(pairs, W=W, chunk=S, num_workers=args.workers)   # warm-up pass (page cache, pinned buffers)
        t0 = time.perf_counter()
        for _ in range(args.passes):
            raw.project_files(pairs, W=W, chunk=S, num_workers=args.workers)
        e2e = args.passes * args.n / (time.perf_counter() - t0)
        # what the host side alone costs: the same bytes read and written by the same threads, no GPU work
        blank = np.zeros((64, W, 4), dtype=np.float32)

        def host_only(pair):
            np.fromfile(pair[0], dtype=np.float32)
            raw.write_npy(pair[1], blank)
        with ThreadPoolExecutor(args.workers) as pool:
            t0 = time.perf_counter()
            list(pool.map(host_only, pairs))
            host = args.n / (time.perf_counter() - t0)
    # ---- numpy on the host threads
    with ThreadPoolExecutor(args.cpu_threads) as pool:
        list(pool.map(numpy_project, scans[:args.cpu_threads]))
        t0 = time.perf_counter()
        list(pool.map(numpy_project, scans))
        cpu = args.n / (time.perf_counter() - t0)
    res = {"project_us_per_scan": round(proj_us, 2), "project_MB_per_scan": round(proj_bytes / 1e6, 2),
           "project_GBps": round(proj_bytes / proj_us / 1e3, 1), "project_frac_of_8TBps": round(proj_bytes / proj_us / 1e3 / HBM_GBPS, 4),
           "angles_us_per_scan": round(ang_us, 2), "angles_GBps": round(ang_bytes / ang_us / 1e3, 1),
           "angles_frac_of_8TBps": round(ang_bytes / ang_us / 1e3 / HBM_GBPS, 4),
           "end_to_end_scans_per_s": round(e2e, 1), "host_io_only_scans_per_s": round(host, 1),
           "numpy_scans_per_s": round(cpu, 1), "numpy_threads": args.cpu_threads,
           "points_per_scan": int(n_pts), "chunk": S, "workers": args.workers, "scans": args.n, "reps": args.reps,
           "clock_ghz": None if args.no_clock else held_clock(), "lib": L.lib().dg_version().decode()}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
