#!/usr/bin/env python3
"""Timing of the synthesis command's point-cloud export (dusty_gan_amd/synthesis.py: dg_export_points)
on B generated scans of 64x1024, at the drop rate of the tests' generator (a seeded full-width dusty2 net whose depth head is
scaled so that depths spread and pixels drop, tests/test_gpu_synthesis.py).
usage: python scripts/bench_synthesis.py [--scans 32] [--reps 50] [--warm 5] [--command-scans 1024] [--big-scans 1024] [--out FILE]
Prints one JSON line:
    export             export_points alone (device events around the two launches), median / p10 / p90 ms, and its minimal
                       HBM traffic (4 B depth per pixel, 8 B angles per pixel, 16 B per kept point) over that time
    export_big         the same call on the batch tiled to --big-scans scans (a working set far past the caches)
    export_to_host     export_points + the copy of records[b, :counts[b]] of every scan to the host (what write_bins moves)
    host_filter        what there was before: inv_to_xyz, the whole [B,3,H,W] point map and depth copied to the host, a numpy
                       boolean index per scan (host clock; ends with the arrays on the host, like export_to_host)
    command            `synthesize --num-samples N --no-images` end to end (host clock around main(), files included)"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "p10_ms": round(float(np.percentile(ms, 10)), 4),
            "p90_ms": round(float(np.percentile(ms, 90)), 4)}


def timed_events(fn, warm, reps):
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
    return stats(ms)


def timed_host(fn, warm, reps):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def make_world(tmp, batch_size):
    from dusty_gan_amd.models import define_G
    from dusty_gan_amd.utils.config import dump_config, load_config
    cfg = load_config(["model=dusty2_dcgan_eqlr", "dataset=synthetic", "dataset.shape=[64,1024]",
                       f"solver.batch_size={batch_size}", "enable_amp=true"])
    cfg_path, ckpt = os.path.join(tmp, "config.yaml"), os.path.join(tmp, "model.pth")
    dump_config(cfg, cfg_path)
    torch.manual_seed(0)
    cfg.model.gen.shape = cfg.dataset.shape
    sd = define_G(cfg).state_dict()
    sd["backbone.4.heads.depth.1.module.weight"] *= 10.0
    sd["backbone.4.heads.depth.1.module.bias"] -= 1.5
    torch.save({"step": 0, "G_ema": sd}, ckpt)
    return ["--model-path", ckpt, "--config-path", cfg_path]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=32)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--command-scans", type=int, default=1024)
    ap.add_argument("--big-scans", type=int, default=1024, help="export alone on the batch tiled to this many scans (0: skip)")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from dusty_gan_amd import synthesis as S
    from dusty_gan_amd import synthesize as cmd
    from dusty_gan_amd import utils
    with tempfile.TemporaryDirectory() as tmp:
        argv = make_world(tmp, args.scans)
        cfg, G, lidar, device = utils.setup(argv[1], argv[3], ema=True, fix_noise=True)
        B, (H, W) = args.scans, cfg.dataset.shape
        depth = S.synthesize(cfg, G, lidar, S.sample_latents(cfg, device, B, "random", 0), normals=False)["depth"]
        records, counts = S.export_points(depth, lidar, from_tanh=False)
        kept = int(counts.sum())

        def to_host():
            rec, cnt = S.export_points(depth, lidar, from_tanh=False)
            return [rec[b, :k].cpu().numpy() for b, k in enumerate(cnt.tolist())]

        def host_filter():
            pts, d01 = lidar.inv_to_xyz(depth, 0.0, from_tanh=False, return_depth=True)
            pts, valid = pts.cpu().numpy(), d01.cpu().numpy()[:, 0].reshape(B, -1) != 0
            out = []
            for b in range(B):
                xyz = pts[b].reshape(3, -1).T[valid[b]] * np.float32(lidar.max_depth)
                out.append(np.concatenate([xyz, np.zeros((len(xyz), 1), np.float32)], axis=1))
            return out

        same = all(np.array_equal(a, b) for a, b in zip(to_host(), host_filter()))
        res = {"scans": B, "shape": [int(H), int(W)], "kept_points": kept, "drop_rate": round(1.0 - kept / (B * H * W), 4),
               "reps": args.reps, "host_filter_gives_the_same_records": bool(same),
               "export": timed_events(lambda: S.export_points(depth, lidar, from_tanh=False), args.warm, args.reps),
               "export_to_host": timed_host(to_host, args.warm, args.reps),
               "host_filter": timed_host(host_filter, max(1, args.warm // 2), max(5, args.reps // 5))}
        traffic = B * H * W * (4 + 8) + kept * 16
        res["export"]["min_traffic_bytes"] = traffic
        res["export"]["min_traffic_gb_per_s"] = round(traffic / (res["export"]["median_ms"] * 1e-3) / 1e9, 1)
        if args.big_scans > 0:   # past every cache: the same scans tiled to a batch whose traffic is HBM's
            reps_big = -(-args.big_scans // B)
            big = depth.repeat(reps_big, 1, 1, 1)
            res["export_big"] = {"scans": len(big), **timed_events(lambda: S.export_points(big, lidar, from_tanh=False),
                                                                   args.warm, args.reps)}
            res["export_big"]["min_traffic_bytes"] = traffic * reps_big
            res["export_big"]["min_traffic_gb_per_s"] = round(traffic * reps_big / (res["export_big"]["median_ms"] * 1e-3) / 1e9, 1)
            del big
        if args.command_scans > 0:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):   # (the command prints every path it writes)
                out_dir = cmd.main(argv + ["--num-samples", str(args.command_scans), "--no-images", "--save-dir-path", tmp])
            torch.cuda.synchronize()
            sec = time.perf_counter() - t0
            files = os.listdir(os.path.join(out_dir, "points"))
            size = sum(os.path.getsize(os.path.join(out_dir, "points", f)) for f in files)
            res["command"] = {"scans": args.command_scans, "batch_size": B, "seconds": round(sec, 3),
                              "scans_per_s": round(args.command_scans / sec, 1), "bins": len(files), "bin_bytes": size}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
