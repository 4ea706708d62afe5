"""python -m dusty_gan_amd.process_clouds --in-dir IN --out-dir OUT --rings H [--width 2048] [--beams kmeans|uniform|FILE] ...

Point clouds of ANY spinning LiDAR -> the files `dataset=scan_folder` trains from:
    IN/<recording>/**/<stem>.bin | .npy   ->  OUT/sequences/<recording>/velodyne/<stem>.npy   (H x W x 4)
    OUT/angles.pt   = the mean (elevation, azimuth) grid [2,H,W] over the --train recordings
    OUT/beams.json  = the beam table and how well the clouds fit it (of the clouds this run projected)
A cloud is a `.bin` (N x 4 float32: x, y, z, reflectance) or a `.npy` of shape N x 3 or N x 4, metres, points in any order -
the files `reconstruct` takes.  Pass 1 counts the elevations of the --train recordings' points (all of them by default, or
--beam-scans evenly spaced files) and makes the sensor's beam table from the histogram; pass 2 gives every point the row of
its nearest beam, projects every cloud and averages the angle grid.  --skip-existing beside an existing OUT/beams.json keeps
that file and its table - the one the files on disk were projected with - and only projects what is missing.  In beams.json
a beam's share of the points far from 1 / H, or many empty cells, shows a wrong --rings.
"""
import argparse
import json
import os
import os.path as osp
import sys
from glob import glob

CLOUD_EXT = (".bin", ".npy")


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m dusty_gan_amd.process_clouds", description=__doc__.split("\n\n")[1],
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--in-dir", type=str, required=True, help="holds one directory of .bin / .npy clouds per recording")
    p.add_argument("--out-dir", type=str, required=True, help="the dataset root to write (dataset.root of scan_folder)")
    p.add_argument("--rings", type=int, required=True, help="the sensor's number of beams H (1..256)")
    p.add_argument("--width", type=int, default=2048, help="azimuth columns W of the written files (1..8192)")
    p.add_argument("--beams", type=str, default="kmeans",
                   help="kmeans (clustered from the clouds), uniform (equally spaced over the field of view), or a text file "
                        "of H elevations in degrees, one per line (the datasheet's table)")
    p.add_argument("--fov-up", type=float, default=None, help="uniform: the highest beam, degrees (default: 99.9 %% quantile)")
    p.add_argument("--fov-down", type=float, default=None, help="uniform: the lowest beam, degrees (default: 0.1 %% quantile)")
    p.add_argument("--beam-range", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="only points between LO and HI metres enter the histogram (default: --min-depth --max-depth); raise "
                        "LO for a sensor whose lasers sit far off its rotation axis")
    p.add_argument("--beam-scans", type=int, default=None, metavar="K", help="histogram K evenly spaced train files only")
    p.add_argument("--train", type=str, nargs="+", default=None, metavar="DIR",
                   help="the recordings the beam table and angles.pt are made from (default: all)")
    p.add_argument("--min-depth", type=float, default=0.9)
    p.add_argument("--max-depth", type=float, default=120.0)
    p.add_argument("--chunk", type=int, default=16, help="clouds per launch")
    p.add_argument("--num-workers", type=int, default=8, help="host threads that read clouds / write .npy files")
    p.add_argument("--skip-existing", action="store_true", help="leave .npy files that already exist alone")
    args = p.parse_args(argv)
    if not 1 <= args.rings <= 256:
        p.error("--rings: 1..256")
    if not 1 <= args.width <= 8192:
        p.error("--width: 1..8192")
    if args.chunk < 1 or args.num_workers < 1:
        p.error("--chunk and --num-workers must be at least 1")
    if not 0 <= args.min_depth < args.max_depth:
        p.error("--min-depth must lie below --max-depth")
    if args.beam_range is not None and not 0 <= args.beam_range[0] < args.beam_range[1]:
        p.error("--beam-range LO HI: 0 <= LO < HI")
    if args.beam_scans is not None and args.beam_scans < 1:
        p.error("--beam-scans must be at least 1")
    if (args.fov_up is None) != (args.fov_down is None):
        p.error("--fov-up and --fov-down go together")
    if args.fov_up is not None and (args.beams != "uniform" or not -90 <= args.fov_down < args.fov_up <= 90):
        p.error("--fov-up / --fov-down: for --beams uniform, -90 <= down < up <= 90 degrees")
    if args.beams not in ("kmeans", "uniform") and not osp.isfile(args.beams):
        p.error(f"--beams: kmeans, uniform or a table file ({args.beams!r} is no file)")
    return args


def plan(in_dir, out_dir, skip_existing=False):
    """{recording: [(cloud file, destination .npy)]}, recordings and files sorted; ValueError for two clouds of one recording
    with the same stem (the outputs are named after it)"""
    recordings = {}
    for rec_dir in sorted(d for d in glob(osp.join(in_dir, "*")) if osp.isdir(d)):
        files = sorted(f for ext in CLOUD_EXT for f in glob(osp.join(rec_dir, "**", "*" + ext), recursive=True))
        seen, pairs = {}, []
        for src in files:
            stem = osp.splitext(osp.basename(src))[0]
            if stem in seen:
                raise ValueError(f"two clouds named {stem!r} in {rec_dir}: {seen[stem]} and {src}")
            seen[stem] = src
            dst = osp.join(out_dir, "sequences", osp.basename(rec_dir), "velodyne", stem + ".npy")
            if not (skip_existing and osp.exists(dst)):
                pairs.append((src, dst))
        if files:
            recordings[osp.basename(rec_dir)] = pairs
    return recordings


def evenly_spaced(items, k):
    """k of the items at evenly spaced positions (all of them when there are no more than k)"""
    if k is None or k >= len(items):
        return list(items)
    return [items[(2 * i + 1) * len(items) // (2 * k)] for i in range(k)]


def main(argv=None):
    args = parse_args(argv)
    H, W = args.rings, args.width
    every = plan(args.in_dir, args.out_dir)
    if not every:
        raise FileNotFoundError(f"no clouds: {osp.join(args.in_dir, '*', '**', '*.bin | *.npy')} matches nothing")
    train = sorted(every) if args.train is None else [osp.basename(osp.normpath(t)) for t in args.train]
    missing = [t for t in train if t not in every]
    if missing:
        raise FileNotFoundError(f"no such recordings under {args.in_dir}: {missing}")
    import numpy as np
    import torch

    from .datasets import beams as B
    from .datasets.raw import AngleAccumulator, project_files_beams

    # pass 1: the beam table - or, with --skip-existing, the table the files already on disk were projected with
    lo, hi, NB = -np.pi / 2, np.pi / 2, B.NB_DEFAULT
    report_path = osp.join(args.out_dir, "beams.json")
    reuse = args.skip_existing and osp.isfile(report_path)
    if reuse:
        with open(report_path) as f:
            report = json.load(f)
        if (report.get("rings"), report.get("width")) != (H, W):
            raise ValueError(f"{report_path} was written for {report.get('rings')} x {report.get('width')}, not {H} x {W}: "
                             "--skip-existing would mix two projections")
        table = np.asarray(report["beams_rad"], dtype=np.float64)
        print(f"beam table of {report_path} kept ({report['method']}); beams.json is left as it is")
    else:
        d_lo, d_hi = args.beam_range if args.beam_range is not None else (args.min_depth, args.max_depth)
        sample = evenly_spaced([src for t in train for src, _ in every[t]], args.beam_scans)
        hist = B.elevation_histogram(sample, d_lo, d_hi, lo, hi, NB, chunk=args.chunk, num_workers=args.num_workers)
        table = B.estimate_beams(hist, H, lo, hi, method=args.beams, fov_up=args.fov_up, fov_down=args.fov_down)
        print(f"beam table ({args.beams}) from {int(hist.sum())} points of {len(sample)} clouds: "
              f"{np.rad2deg(table[0]):.3f} .. {np.rad2deg(table[-1]):.3f} degrees")

    # pass 2: every cloud projected; the angle grid summed over the train recordings while their projections are on the device
    todo = plan(args.in_dir, args.out_dir, args.skip_existing) if args.skip_existing else every
    pairs = [pair for name in sorted(todo) for pair in todo[name]]
    in_train = {dst for t in train for _, dst in every[t]}
    dev = torch.device("cuda", torch.cuda.current_device())
    acc = AngleAccumulator(H, W, dev, args.min_depth, args.max_depth)
    empty = torch.zeros((), dtype=torch.int64, device=dev)
    projected = 0

    def on_chunk(batch, out):
        nonlocal projected
        empty.add_((out[..., :3] == 0).all(-1).sum())
        projected += len(batch)
        keep = [j for j, (_, dst) in enumerate(batch) if dst in in_train]
        if len(keep) == len(batch):
            acc.add(out)
        elif keep:
            acc.add(out[torch.tensor(keep, device=dev)].contiguous())

    n = project_files_beams(pairs, table, W=W, chunk=args.chunk, num_workers=args.num_workers, on_chunk=on_chunk)
    print(f"projected {n} clouds into {osp.join(args.out_dir, 'sequences')}")
    if acc.total < sum(len(every[t]) for t in train):   # --skip-existing left train files alone: their angles come from disk
        from .datasets.raw import average_angles
        paths = sorted(in_train)
        angles = average_angles(paths, args.min_depth, args.max_depth, chunk=args.chunk, num_workers=args.num_workers)
    else:
        angles = acc.finish()
    os.makedirs(args.out_dir, exist_ok=True)
    torch.save(angles.cpu(), osp.join(args.out_dir, "angles.pt"))
    print(f"angles.pt: {len(in_train)} clouds of {len(train)} recordings")
    if reuse:
        return 0
    report = {"method": args.beams, "rings": H, "width": W, "beams_deg": np.rad2deg(table).tolist(),
              "beams_rad": table.tolist(), "lo": float(lo), "hi": float(hi), "NB": int(NB),
              "beam_range": [float(d_lo), float(d_hi)], "clouds_counted": len(sample), "points_counted": int(hist.sum()),
              "beam_share": B.beam_shares(hist, table, lo, hi).tolist(),
              "empty_cells": float(empty) / (projected * H * W) if projected else None,
              "train": train}
    with open(report_path, "w") as f:
        json.dump(report, f, indent=1)
    if projected:
        print(f"beams.json: {100 * report['empty_cells']:.1f} % of all cells empty")
    return 0


if __name__ == "__main__":
    sys.exit(main())
