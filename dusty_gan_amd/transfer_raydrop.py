"""Ray-drop transfer: make simulated (complete) scans look measured - G's inferred drops applied to the scans' own points.

    python -m dusty_gan_amd.transfer_raydrop --model-path <ckpt.pth> --config-path <config.yaml> --points PATH [PATH ...]
        [--labels DIR] [--realisations 1] [--drop-noise sample|fixed] [--seed 0] [--tau 2] [--batch-size 32]
        [--save-dir-path .] [--no-maps]
        [--distance l1] [--emd-points 2048] [--num-step 1000] [--num-code N --composition-layer NAME] [--corruption NAME [--corruption-seed 0]]

The use the DUSty paper trains the measurability head for (the reference's repository holds no code for it): every cloud -
files and stems as dusty_gan_amd.reconstruct takes them - is projected onto the model's angle grid, inverted through G's
unmasked depth (the inversion flags are evaluate_reconstruction's; `--corruption closing` pre-fills a sparse simulator frame),
and the measurability G predicts at the optimised latent is sampled `--realisations` times.  A pixel's drop removes the INPUT
point that stands for the pixel (the nearest of the points binned into it); points hidden behind it in the same pixel go too.
What survives are input records, unchanged bit for bit, fourth column included.  `--labels DIR` holds one SemanticKITTI
`<stem>.label` per cloud (N little-endian uint32, one per record); the labels travel with their points.
`--drop-noise fixed` applies the one mask the generator's own head showed during the inversion (one realisation); `sample`
draws fresh logistic noise per scan and realisation from Philox (`--seed`): the same scan, seed and realisation give the
same files in any batch.  Under <save-dir-path>/raydrop/ it writes
    points/<stem>_<k>.bin     the surviving input records of realisation k (KITTI N x 4 float32, metres), in row-major
                              order of their pixels
    labels/<stem>_<k>.label   their labels (with --labels)
    maps/<stem>.npy           [2 + K,H,W] float32: the projected normalised depth (1 where no point fell), the sigmoid of the
                              pixel confidence, the K keep masks (unless --no-maps)
    stats.csv                 name, input points, valid pixels, kept_<k> per realisation, drop rate (1 - mean kept / valid
                              pixels), the inversion's final loss"""
import argparse
import csv
import os
import os.path as osp

from .evaluate_reconstruction import add_inversion_arguments, check_inversion_arguments, scans_per_pass, split_distance
from .reconstruct import expand_paths


def label_path(labels_dir, stem):
    return osp.join(labels_dir, f"{stem}.label")


def read_labels(path, rows):
    """a SemanticKITTI .label file -> uint32 [rows]; ValueError naming the file when its count differs from the cloud's"""
    import numpy as np
    size = osp.getsize(path)
    if size != 4 * rows:
        raise ValueError(f"{path}: {size / 4:g} labels for a cloud of {rows} records")
    return np.fromfile(path, dtype="<u4")


def write_labels(path, labels):
    import numpy as np
    np.ascontiguousarray(labels).astype("<u4", copy=False).tofile(path)


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    add_inversion_arguments(parser, batch_size=32)
    parser.add_argument("--points", type=str, nargs="+", required=True, help="cloud files (.bin / .npy) or directories of them")
    parser.add_argument("--labels", type=str, default=None, help="directory of SemanticKITTI <stem>.label files (uint32 per record)")
    parser.add_argument("--realisations", type=int, default=1, help="drop masks sampled per scan")
    parser.add_argument("--drop-noise", choices=("sample", "fixed"), default="sample",
                        help="sample: fresh logistic noise per scan and realisation; fixed: the inversion's own fixed Gumbel noise")
    parser.add_argument("--seed", type=int, default=0, help="Philox seed of the inversion's and the drops' draws")
    parser.add_argument("--tau", type=float, default=2, help="points_to_depth's depth weight exp(-tau depth), 0..16")
    parser.add_argument("--no-maps", action="store_true")
    args = parser.parse_args(argv)
    check_inversion_arguments(parser, args)
    if not 0 <= args.tau <= 16:
        parser.error("--tau: 0..16")
    if args.batch_size < 1:
        parser.error("--batch-size must be at least 1")
    if args.realisations < 1:
        parser.error("--realisations must be at least 1")
    if args.drop_noise == "fixed" and args.realisations != 1:
        parser.error("--drop-noise fixed is one realisation: the inversion's own fixed Gumbel noise")
    from .datasets.raw import RawScanError, _cloud_rows
    from .utils.config import load_config_file
    masker = str(load_config_file(args.config_path).model.gen.arch).split("/")[0]
    if not masker.startswith("dusty"):
        parser.error(f"{args.config_path}: generator {masker!r} has no measurability head: nothing to transfer")
    try:
        args.clouds = expand_paths(args.points)
        args.rows = [_cloud_rows(path)[0] for _, path in args.clouds]
        if args.labels is not None:
            for (stem, _), rows in zip(args.clouds, args.rows):
                path = label_path(args.labels, stem)
                if not osp.isfile(path):
                    raise ValueError(f"{path}: no label file for cloud {stem!r}")
                if osp.getsize(path) != 4 * rows:
                    raise ValueError(f"{path}: {osp.getsize(path) / 4:g} labels for a cloud of {rows} records")
    except (ValueError, RawScanError) as e:
        parser.error(str(e))
    return args


def main(argv=None):
    """-> the directory written (<save-dir-path>/raydrop)"""
    args = parse_args(argv)
    import numpy as np
    import torch

    from . import raydrop, utils
    from .datasets.raw import read_clouds
    cfg, G, lidar, device = utils.setup(args.model_path, args.config_path, ema=True, fix_noise=True)
    utils.set_requires_grad(G, False)
    if lidar.angle is None:
        raise RuntimeError(f"no angle grid: {lidar.angle_file!r} does not exist (utils/lidar.py:120)")
    out_dir = osp.join(args.save_dir_path, "raydrop")
    with_labels, maps, K = args.labels is not None, not args.no_maps, args.realisations
    for sub in ["points"] + ["labels"] * with_labels + ["maps"] * maps:
        os.makedirs(osp.join(out_dir, sub), exist_ok=True)
    names = split_distance(args.distance)
    inv = dict(num_step=args.num_step, distance=names[0] if len(names) == 1 else names)   # (as evaluate_batch calls invert)
    if "emd" in names:
        inv.update(emd_points=args.emd_points)
    if args.num_code > 1:
        inv.update(num_code=args.num_code, composition_layer=args.composition_layer)
    written, table = [], []
    step = scans_per_pass(args.batch_size, args.num_code)
    for i in range(0, len(args.clouds), step):
        stems, paths = zip(*args.clouds[i:i + step])
        records, counts, raw = read_clouds(paths, lidar.max_depth, device, return_raw=True)
        labels = None
        if with_labels:
            lab = np.zeros(tuple(records.shape[:2]), dtype=np.int64)
            for b, stem in enumerate(stems):
                n = int(counts[b])
                lab[b, :n] = read_labels(label_path(args.labels, stem), n)
            labels = torch.from_numpy(lab).to(device)
        res = raydrop.transfer(G, lidar, records, counts, records_raw=raw, labels=labels, realisations=K, noise=args.drop_noise,
                               seed=args.seed, first_index=i, tau=args.tau, corruption=args.corruption,
                               corruption_seed=args.corruption_seed, **inv)
        kept = res["counts"].cpu().numpy()
        valid = res["valid"].flatten(1).sum(dim=1).cpu().numpy()
        loss = res["loss"].cpu().numpy()
        if maps:
            stack = torch.cat([res["target"], res["confidence"], res["keep"].float()], dim=1).cpu().numpy()
        for b, stem in enumerate(stems):
            for k in range(K):
                n = int(kept[b, k])
                written.append(osp.join(out_dir, "points", f"{stem}_{k}.bin"))
                res["records"][b, k, :n].cpu().contiguous().numpy().astype("<f4", copy=False).tofile(written[-1])
                if with_labels:
                    written.append(osp.join(out_dir, "labels", f"{stem}_{k}.label"))
                    write_labels(written[-1], res["labels"][b, k, :n].cpu().numpy().view(np.uint32))
            if maps:
                written.append(osp.join(out_dir, "maps", f"{stem}.npy"))
                np.save(written[-1], stack[b])
            drop = 1.0 - float(kept[b].mean()) / float(valid[b]) if valid[b] else float("nan")
            table.append([stem, int(counts[b]), int(valid[b])] + [int(v) for v in kept[b]] + [repr(drop), repr(float(loss[b]))])
    with open(osp.join(out_dir, "stats.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["name", "points", "valid_pixels"] + [f"kept_{k}" for k in range(K)] + ["drop_rate", "loss"])
        w.writerows(table)
    written.append(osp.join(out_dir, "stats.csv"))
    for path in written:
        print("wrote:", path)
    return out_dir


if __name__ == "__main__":
    main()
