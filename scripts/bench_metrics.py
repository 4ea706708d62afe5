#!/usr/bin/env python3
"""Timing of the validation-metric kernels at the KITTI validation size: N clouds (sequence 08
has 4071 scans) of 64x1024 points, FPS to 512 points, all-pairs Chamfer, JSD voting.
usage: python scripts/bench_metrics.py [--clouds 4071] [--fps-clouds 256]
       python scripts/bench_metrics.py --fps-map [--fps-map-reps 7] [--fps-map-out profiles/fps_map.txt]
--fps-map: only the comparison of furthest point sampling on 64x1024 point maps - the transposed [B,HW,3] copy followed
by dg_fps (what Trainer.validation() runs) against dg_fps_map on the map where it lies.
Roofline for the Chamfer kernel: VALU fp32.  One point pair = 3 sub + 1 mul + 2 fma + 1 min = 9 flops (8 without the
min); peak = 157.3 TFLOP/s packed fp32 (MI355X_MICROARCH.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def fps_map_table(reps, out_path=None):
    """B clouds of 64x1024 scan-like points (dg_inv_to_xyz of random inverse depths on the nominal HDL-64E grid, a tenth of
    the pixels dropped) down to m samples: `packed` = transposed copy + dg_fps, `map` = dg_fps_map.  Both warm, then `reps`
    alternating repetitions in this process, each timed with its own event pair; ms as median [p10 .. p90]."""
    from dusty_gan_amd.utils.lidar import LiDAR
    from dusty_gan_amd.utils.sampling import downsample_point_clouds, downsample_point_map
    lidar = LiDAR(64, 1024, 1.45, 80.0).use_nominal_angles().to("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    lines = [f"furthest point sampling of 64x1024 point maps, ms per call: median [p10 .. p90] of {reps} alternating "
             f"repetitions after a warm call each", f"{'B':>5} {'m':>5}  {'packed copy + dg_fps':>30}  {'dg_fps_map':>30}  "
             f"{'median ratio':>12}  map p90 < packed p10"]
    rows = []
    for B in (256, 1024):
        xyz = torch.cat([lidar.inv_to_xyz(torch.rand(64, 1, 64, 1024, device="cuda", generator=g), 0.1)
                         for _ in range(B // 64)])
        for m in (512, 2048):
            fns = {"packed": lambda: downsample_point_clouds(xyz.flatten(2).transpose(1, 2).contiguous(), m),
                   "map": lambda: downsample_point_map(xyz, m)}
            assert torch.equal(fns["packed"](), fns["map"]())   # (also the warm call of each)
            ts = {k: [] for k in fns}
            for _ in range(reps):
                for k, fn in fns.items():
                    ts[k].append(once(fn))
            q = {k: np.percentile(v, [50, 10, 90]) for k, v in ts.items()}
            below = bool(q["map"][2] < q["packed"][1])
            cell = {k: f"{v[0]:9.2f} [{v[1]:8.2f} .. {v[2]:8.2f}]" for k, v in q.items()}
            lines.append(f"{B:>5} {m:>5}  {cell['packed']:>30}  {cell['map']:>30}  {q['packed'][0] / q['map'][0]:>12.3f}  "
                         f"{'yes' if below else 'NO'}")
            rows.append({"B": B, "m": m, "packed_ms": [round(float(x), 3) for x in q["packed"]],
                         "map_ms": [round(float(x), 3) for x in q["map"]], "map_p90_below_packed_p10": below})
        del xyz
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)
    print(json.dumps({"fps_map": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=4071)
    ap.add_argument("--points", type=int, default=512)
    ap.add_argument("--fps-clouds", type=int, default=256)
    ap.add_argument("--validation", action="store_true", help="also time a full Trainer.validation() at 64x1024")
    ap.add_argument("--fps-map", action="store_true", help="only: dg_fps_map against the packed copy + dg_fps")
    ap.add_argument("--fps-map-reps", type=int, default=7)
    ap.add_argument("--fps-map-out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    if args.fps_map:
        return fps_map_table(max(7, args.fps_map_reps), args.fps_map_out)
    from dusty_gan_amd.utils.metrics import chamfer_dir, compute_cov_mmd_1nna, compute_jsd
    from dusty_gan_amd.utils.sampling import downsample_point_clouds
    from oracle import metrics_oracle as MO
    g = torch.Generator(device="cuda").manual_seed(0)
    N, n = args.clouds, args.points
    ref = torch.randn(N, n, 3, device="cuda", generator=g) * 0.2
    gen = torch.randn(N, n, 3, device="cuda", generator=g) * 0.25
    ms = timed(lambda: chamfer_dir(ref, gen), reps=2)
    pairs = N * N * n * n
    res = {"chamfer_dir_ms": round(ms, 2), "clouds": N, "points": n,
           "point_pairs_per_s": round(pairs / ms * 1e3, 0), "TFLOPs_9_per_pair": round(9 * pairs / ms / 1e9, 2),
           "frac_of_157_TFLOPs": round(9 * pairs / ms / 1e9 / 157.3, 4)}
    t0 = time.perf_counter()
    compute_cov_mmd_1nna(gen, ref, 512, ("cd",), verbose=False)
    torch.cuda.synchronize()
    res["cov_mmd_1nna_s"] = round(time.perf_counter() - t0, 3)
    t0 = time.perf_counter()
    compute_jsd(gen / 2, ref / 2)
    torch.cuda.synchronize()
    res["jsd_s"] = round(time.perf_counter() - t0, 3)
    full = torch.randn(args.fps_clouds, 65536, 3, device="cuda", generator=g) * 0.3
    res["fps_ms_per_cloud_65536_to_512"] = round(timed(lambda: downsample_point_clouds(full, n), reps=1)
                                                 / args.fps_clouds, 4)
    res["fps_clouds"] = args.fps_clouds
    # CPU restatement on a bounded sample (the reference's own CPU path, nnsearch, is the same O(n*m) loop)
    a, b = ref[:8].cpu().numpy(), gen[:64].cpu().numpy()
    t0 = time.perf_counter()
    MO.chamfer_dir(a, b)
    dt = time.perf_counter() - t0
    res["cpu_oracle_point_pairs_per_s"] = round(8 * 64 * n * n / dt, 0)
    res["cpu_threads"] = torch.get_num_threads()
    t0 = time.perf_counter()
    MO.fps(full[0].cpu().numpy(), n)
    res["cpu_oracle_fps_ms_per_cloud"] = round((time.perf_counter() - t0) * 1e3, 1)
    if args.validation:
        # the whole reference validation pass (trainers/dcgan_amp.py:342-393) at the KITTI size: N real + N generated
        # 64x1024 scans -> point maps -> FPS to 512 -> SWD + JSD + COV/MMD/1-NNA(CD)
        from dusty_gan_amd.trainers.dcgan_amp import Trainer
        from dusty_gan_amd.utils.config import load_config
        del ref, gen, full
        torch.cuda.empty_cache()
        pool = -(-args.clouds // 32)
        cfg = load_config(["model=dusty2_dcgan_eqlr", "dataset=synthetic", "dataset.shape=[64,1024]",
                           "solver.batch_size=32", f"dataset.pool={pool}", "enable_amp=true"])
        tr = Trainer(cfg, {"gpu": 0, "ngpus": 1, "batch_size": 32, "num_workers": 0})
        tr.validation()  # warm-up (workspaces, sort plans)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc = tr.validation()
        torch.cuda.synchronize()
        res["validation_s"] = round(time.perf_counter() - t0, 2)
        res["validation_N"] = pool * 32
        res["validation_scores"] = {k: round(v, 5) for k, v in sc.items() if k in ("swd-mean", "jsd", "mmd-cd", "cov-cd",
                                                                                    "1-nn-accuracy-cd")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
