#!/usr/bin/env python3
"""Label images and object removal on one MI355X box: what the new kernels cost beside what they ride on.

One JSON line:
  * scan_labels_us_per_scan beside project_us_per_scan: dg_scan_labels and dg_scan_project on the same device-resident chunk
    of seeded 64 x 2048 scans (scripts/bench_process_kitti.py's, ~121 000 points each), graph-free launches timed with HIP
    events, the MEDIAN of --reps runs after warm-up, per scan; and the bytes the label launch must move (8 of key + 4 of
    label per non-empty cell in, 1 out per cell);
  * remove_mask_us (r = 1) and compose_us at 64 x 1024, batch 32, beside inversion_step_us: one graph-replayed step of
    inversion.invert on the same batch (bf16 dusty2, l1), the difference of a long and a short run.
usage: python scripts/bench_labels.py [--chunk 16] [--reps 50] [--out profiles/labels.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_process_kitti import make_scan, median_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=16, help="scans per launch")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--short", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from dusty_gan_amd import _lib as L
    from dusty_gan_amd import removal as RM
    from dusty_gan_amd.datasets import labels as LB
    from dusty_gan_amd.datasets import raw
    dev = torch.device("cuda")
    W, S = 2048, args.chunk
    rng = np.random.default_rng(0)
    scans = [make_scan(rng) for _ in range(S)]
    pts = torch.from_numpy(np.concatenate(scans)).to(dev)
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)).to(dev)
    keys = torch.empty(S * 64 * W, dtype=torch.int64, device=dev)
    status = torch.empty(S, dtype=torch.int32, device=dev)
    out = torch.empty(S, 64, W, 4, dtype=torch.float32, device=dev)
    ids = np.flatnonzero(LB.SEMANTIC_KITTI_LUT != LB.UNKNOWN)
    lab = torch.from_numpy(rng.choice(ids, pts.shape[0]).astype(np.int32)).to(dev)
    lut = LB.device_lut(dev)
    sem = torch.empty(S, 64, W, dtype=torch.uint8, device=dev)
    inst = torch.empty(S, 64, W, dtype=torch.int16, device=dev)
    lst = torch.zeros(S, dtype=torch.int32, device=dev)
    proj_us = median_us(lambda: raw._launch_project(pts, offs, S, W, keys, status, None, out), args.reps) / S

    def labels():
        L.check(L.lib().dg_scan_labels(L.ptr(keys), L.ptr(offs), L.ptr(lab), L.ptr(lut), S, 64, W, L.ptr(sem), L.ptr(inst),
                                       L.ptr(lst), L.stream_ptr()), "dg_scan_labels")
    lab_us = median_us(labels, args.reps) / S
    filled = float((keys != -1).sum()) / S
    lab_bytes = 64 * W * (8 + 1 + 2) + filled * 4
    # ---- the removal kernels beside one inversion step
    B, H, Wm = args.batch, 64, 1024
    g = torch.Generator(device="cpu").manual_seed(1)
    # a street scene's proportions: road everywhere, 3 % of the pixels a car
    sem_m = torch.where(torch.rand(B, H, Wm, generator=g) < 0.03, 1, 9).to(torch.uint8).to(dev)
    mask = (torch.rand(B, 1, H, Wm, generator=g) > 0.1).float().to(dev)
    ref = torch.rand(B, 1, H, Wm, generator=g).to(dev)
    gen = torch.rand(B, 1, H, Wm, generator=g).to(dev)
    table = RM.class_table(range(1, 9), dev)
    remove, _ = RM.remove_mask(sem_m, mask, table, 1)
    # (the entry points themselves, outputs allocated once: the counters are added to, which costs what a zeroed run costs)
    rm_out, cls = torch.empty_like(sem_m), torch.zeros(B, 256, dtype=torch.int32, device=dev)
    inv_out, src, sem_out = torch.empty_like(ref), torch.empty_like(sem_m), torch.empty_like(sem_m)
    cnt = torch.zeros(B, 3, dtype=torch.int32, device=dev)
    rm_us = median_us(lambda: L.check(L.lib().dg_remove_mask(L.ptr(sem_m), L.ptr(mask), L.ptr(table), B, H, Wm, 1, L.ptr(rm_out),
                                                             L.ptr(cls), L.stream_ptr()), "dg_remove_mask"), args.reps)
    cp_us = median_us(lambda: L.check(L.lib().dg_compose_removed(L.ptr(ref), L.ptr(mask), L.ptr(gen), L.ptr(mask), 0, 0.0,
                                                                 L.ptr(remove), L.ptr(sem_m), 0, B, H, Wm, L.ptr(inv_out), L.ptr(src),
                                                                 L.ptr(sem_out), L.ptr(cnt), L.stream_ptr()), "dg_compose_removed"),
                      args.reps)
    from dusty_gan_amd.inversion import invert
    from dusty_gan_amd.models import dusty
    from dusty_gan_amd.models.gans.dcgan_eqlr import Generator
    torch.manual_seed(0)
    bb = Generator(512, {"depth": 1, "confidence": 2}, 64, 512, (H, Wm), ring=True)
    bb.set_precision(torch.bfloat16)
    G = dusty.DUSty2(bb, tau=1, drop_const=-1).to(dev).eval()
    gum = torch.zeros(1, 1, H, Wm)
    tgt_mask = mask * (1 - remove[:, None].float())
    invert(G, ref, tgt_mask, num_step=args.short, gumbel_noise=gum)
    ms = {}
    for n in (args.short, args.steps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        invert(G, ref, tgt_mask, num_step=n, gumbel_noise=gum)
        e1.record()
        torch.cuda.synchronize()
        ms[n] = e0.elapsed_time(e1)
    step_us = (ms[args.steps] - ms[args.short]) / (args.steps - args.short) * 1e3
    res = {"project_us_per_scan": round(proj_us, 2), "scan_labels_us_per_scan": round(lab_us, 2),
           "scan_labels_MB_per_scan": round(lab_bytes / 1e6, 2), "scan_labels_GBps": round(lab_bytes / lab_us / 1e3, 1),
           "points_per_scan": int(pts.shape[0] / S), "cells_filled_per_scan": int(filled), "chunk": S,
           "remove_mask_r1_us": round(rm_us, 2), "compose_us": round(cp_us, 2), "inversion_step_us": round(step_us, 1),
           "removal_shape": [B, H, Wm], "removed_share": round(float(remove.float().mean()), 3), "reps": args.reps,
           "lib": L.lib().dg_version().decode()}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
