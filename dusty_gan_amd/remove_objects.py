"""Remove labelled objects from LiDAR scans: mask the cars, people and cyclists, invert G against the static scene alone,
take G's measured background where the objects stood.

    python -m dusty_gan_amd.remove_objects --model-path <ckpt.pth> --config-path <config.yaml>
        (--points PATH [PATH ...] --labels DIR   |   --split test|val|train [--num-scans K])
        [--remove CLASS [CLASS ...]] [--dilate 1] [--fill-label 0] [--tau 2] [--batch-size 32] [--save-dir-path .] [--no-images]
        [--distance l1] [--emd-points 2048] [--num-step 1000] [--tol 0] [--num-code N --composition-layer NAME]

--points: clouds as dusty_gan_amd.reconstruct takes them, with DIR/<stem>.label (one uint32 SemanticKITTI word per record).
Every cloud is projected by LiDAR.points_to_depth; a pixel's class is that of its nearest point (dg_pixel_winner).
--split: the dataset's projected scans with the label images `process_kitti --labels` wrote beside them (.../velodyne/X.npy
-> .../labels/X.png), both resampled to the model's shape by the same nearest rule.
CLASS is a SemanticKITTI class name or its number 0..19; the default removes every vehicle and every person.  The label mask
takes the place of a corruption: the inversion flags are evaluate_reconstruction's, without --corruption.

Under <save-dir-path>/removal/ it writes, per scan,
    points/<stem>.bin        --points: the records whose pixel is not removed, bit for bit and in input order, then one record
                             (x, y, z, 0) per filled pixel; --split: the result's pixels as records (synthesis.export_points)
    labels/<stem>.label      one uint32 per record of points/<stem>.bin (kept records keep their word; fill: --fill-label)
    maps/<stem>.npy          [4,H,W] float32: target inverse depth, remove, source (0 empty, 1 measured, 2 generated), result
    labels_png/<stem>.png    the result's label image
    images/<stem>.png        target beside result: inverse depth, label image, bird's-eye view
and stats.csv: name, points_in, points_kept, points_filled, pixels_removed, pixels_filled, in_front, px_<class> per class.
in_front counts filled pixels whose background came out NEARER than the object measured there - impossible for a true
background, so it is reported, not hidden."""
import argparse
import csv
import os
import os.path as osp

from .evaluate_reconstruction import add_inversion_arguments, check_inversion_arguments, invert_target, scans_per_pass

DEFAULT_REMOVE = ("car", "bicycle", "motorcycle", "truck", "other-vehicle", "person", "bicyclist", "motorcyclist")
PICTURES = ("inv.png", "label.png", "bev.png")
STATS = ["name", "points_in", "points_kept", "points_filled", "pixels_removed", "pixels_filled", "in_front"]


def parse_classes(items):
    """names or numbers -> sorted class numbers; ValueError for one that is neither"""
    from .datasets.labels import CLASS_NAMES
    out = set()
    for it in items:
        if it in CLASS_NAMES:
            out.add(CLASS_NAMES.index(it))
        elif it.isdigit() and int(it) < len(CLASS_NAMES):
            out.add(int(it))
        else:
            raise ValueError(f"{it!r}: not a class (0..{len(CLASS_NAMES) - 1} or one of {', '.join(CLASS_NAMES)})")
    return sorted(out)


def parse_args(argv=None):
    parser = argparse.ArgumentParser(prog="python -m dusty_gan_amd.remove_objects")
    add_inversion_arguments(parser, batch_size=32)
    parser.add_argument("--points", type=str, nargs="+", default=None, help="cloud files (.bin / .npy) or directories of them")
    parser.add_argument("--labels", type=str, default=None, help="with --points: the directory of <stem>.label files")
    parser.add_argument("--split", type=str, choices=("test", "val", "train"), default=None,
                        help="the dataset's projected scans of this split, with their label images")
    parser.add_argument("--num-scans", type=int, default=None, help="with --split: only the first K scans")
    parser.add_argument("--remove", type=str, nargs="+", default=list(DEFAULT_REMOVE), help="class names or numbers")
    parser.add_argument("--dilate", type=int, default=1, help="grow the mask by this many pixels (0..8)")
    parser.add_argument("--fill-label", type=int, default=0, help="the class of the generated background (0..19)")
    parser.add_argument("--tau", type=float, default=2, help="points_to_depth's depth weight exp(-tau depth), 0..16")
    parser.add_argument("--no-images", action="store_true")
    args = parser.parse_args(argv)
    check_inversion_arguments(parser, args)
    if args.corruption is not None or args.corruption_seed != 0:
        parser.error("the label mask takes the place of a corruption: --corruption / --corruption-seed are not accepted")
    if (args.points is None) == (args.split is None):
        parser.error("one of --points and --split")
    if args.points is not None and args.labels is None:
        parser.error("--points needs --labels DIR")
    if args.split is not None and args.labels is not None:
        parser.error("--labels goes with --points (a split's label images lie beside its scans)")
    if args.num_scans is not None and (args.split is None or args.num_scans < 1):
        parser.error("--num-scans K >= 1 goes with --split")
    from .removal import MAX_DILATE
    if not 0 <= args.dilate <= MAX_DILATE:
        parser.error(f"--dilate: 0..{MAX_DILATE}")
    if not 0 <= args.fill_label <= 19:
        parser.error("--fill-label: 0..19")
    if not 0 <= args.tau <= 16:
        parser.error("--tau: 0..16")
    if args.batch_size < 1:
        parser.error("--batch-size must be at least 1")
    try:
        args.remove_classes = parse_classes(args.remove)
        if args.points is not None:
            from .reconstruct import expand_paths
            args.clouds = expand_paths(args.points)
            for stem, _ in args.clouds:
                if not osp.isfile(osp.join(args.labels, stem + ".label")):
                    raise ValueError(f"{osp.join(args.labels, stem + '.label')}: no label file for {stem}")
    except ValueError as e:
        parser.error(str(e))
    return args


def label_png_of(scan_path):
    """.../velodyne/X.npy -> .../labels/X.png"""
    head, tail = osp.split(scan_path)
    if osp.basename(head) != "velodyne":
        raise FileNotFoundError(f"{scan_path}: not under a velodyne/ directory, so its label image has no place")
    return osp.join(osp.dirname(head), "labels", osp.splitext(tail)[0] + ".png")


def cloud_batch(lidar, stems, paths, label_dir, tau, device):
    """cloud files + their .label files -> (item {"depth","mask","xyz"}, sem [B,H,W] uint8, cloud dict: raw records in metres,
    counts, idx, labels [B,N] int32 bits)"""
    import numpy as np
    import torch

    from .datasets.labels import project_labels, read_label_file
    from .datasets.raw import read_clouds
    from .raydrop import pixel_winner
    records, counts, raw = read_clouds(paths, lidar.max_depth, device, return_raw=True)
    B, N, _ = records.shape
    lab = np.zeros((B, N), dtype=np.uint32)
    label_paths = [osp.join(label_dir, stem + ".label") for stem in stems]
    for b, (path, n) in enumerate(zip(label_paths, counts.tolist())):
        lab[b, :n] = read_label_file(path, n)
    labels = torch.from_numpy(lab.view(np.int32)).to(device)
    depth, valid, idx = lidar.points_to_depth(records, drop_value=1, tau=tau, counts=counts, return_index=True)
    win = pixel_winner(records, idx, counts, lidar.H, lidar.W)
    # a pixel's class through dg_scan_labels and the same table: the winner's index is a z-buffer word's lower half, a
    # pixel without a point the empty word
    sem, _ = project_labels(win.to(torch.int64).reshape(-1), [b * N for b in range(B + 1)], labels.reshape(-1), lidar.H, lidar.W,
                            names=label_paths)
    mask = valid.float()
    item = {"depth": depth, "mask": mask, "xyz": lidar.inv_to_xyz(mask * lidar.invert_depth(depth))}
    return item, sem, {"raw": raw, "counts": counts, "idx": idx, "labels": labels}


def split_batch(dataset, paths, device):
    """projected scans + their label PNGs -> (item, sem [B,H,W] uint8); a missing PNG raises FileNotFoundError naming it"""
    import numpy as np
    import torch

    from .datasets.labels import read_label_png
    from .datasets.scans import scan_to_polar
    from .removal import label_resize
    scans, sems = [], []
    for p in paths:
        png = label_png_of(p)
        if not osp.isfile(png):
            raise FileNotFoundError(f"{png}: the label image of {p} is missing (python -m dusty_gan_amd.process_kitti --labels)")
        scan = np.ascontiguousarray(np.load(p), dtype=np.float32)
        sem = read_label_png(png)
        if sem.shape != scan.shape[:2]:
            raise ValueError(f"{png}: {sem.shape} labels for a {scan.shape[:2]} scan")
        scans.append(scan)
        sems.append(sem)
    item = scan_to_polar(torch.from_numpy(np.stack(scans)).to(device), dataset.shape, dataset.min_depth, dataset.max_depth,
                         want_xyz=True)
    sem = label_resize(torch.from_numpy(np.stack(sems)).to(device), *dataset.shape)
    return item, sem


def _label_picture(sem, palette_dev):
    """[B,H,W] uint8 classes -> [B,3,H,W] float colours in [0,1]"""
    return (palette_dev[sem.long()].permute(0, 3, 1, 2).float() / 255.0).contiguous()


def main(argv=None):
    """-> the directory written (<save-dir-path>/removal)"""
    args = parse_args(argv)
    import numpy as np
    import torch

    from . import removal as RM
    from . import synthesis as S
    from . import utils
    from .datasets.labels import CLASS_NAMES, palette, write_label_png
    from .reconstruct import _side_by_side
    from .synthesize import pictures_of
    from .utils.lidar import postprocess, xyz_to_normal
    cfg, G, lidar, device = utils.setup(args.model_path, args.config_path, ema=True, fix_noise=True)
    utils.set_requires_grad(G, False)
    if lidar.angle is None:
        raise RuntimeError(f"no angle grid: {lidar.angle_file!r} does not exist (utils/lidar.py:120)")
    dusty = "dusty" in str(cfg.model.gen.arch)
    if args.split is not None:
        from .datasets import define_dataset
        dataset = define_dataset(cfg.dataset, phase=args.split)
        paths_all = list(dataset.datalist)[:args.num_scans]
        if not paths_all:
            raise FileNotFoundError(f"no scans of the {args.split} split under {dataset.root}")
        scans = [(f"{i:06d}_{osp.splitext(osp.basename(p))[0]}", p) for i, p in enumerate(paths_all)]
    else:
        scans = args.clouds
    out_dir = osp.join(args.save_dir_path, "removal")
    images = not args.no_images
    for sub in ["points", "labels", "maps", "labels_png"] + ["images"] * images:
        os.makedirs(osp.join(out_dir, sub), exist_ok=True)
    if images:
        R, t = (v.to(device) for v in S.view())
        pal = torch.from_numpy(np.array(palette())).to(device)
    table = RM.class_table(args.remove_classes, device)
    written, rows = [], []
    step = scans_per_pass(args.batch_size, args.num_code)
    for i in range(0, len(scans), step):
        stems, paths = zip(*scans[i:i + step])
        if args.split is not None:
            (item, sem), cloud = split_batch(dataset, paths, device), None
        else:
            item, sem, cloud = cloud_batch(lidar, stems, paths, args.labels, args.tau, device)
        depth, mask = item["depth"], item["mask"].float()
        remove, class_pixels = RM.remove_mask(sem, mask, table, args.dilate)
        tgt_inv = mask * lidar.invert_depth(depth)
        tgt_mask = mask * (1 - remove[:, None].float())
        res = invert_target(G, lidar, tgt_mask * tgt_inv, tgt_mask, args, first_index=i)
        out = postprocess(res["out"], lidar, tol=args.tol)
        keep = out["mask"].prod(dim=1, keepdim=True) if dusty else out["depth"]
        inv_out, source, sem_out, counts = RM.compose(tgt_inv, mask, out["depth"], keep, remove, sem, keep_is_depth=not dusty,
                                                      tol=args.tol, fill_label=args.fill_label)
        filled = source == 2
        fill_rec, fill_cnt = S.export_points(inv_out * filled[:, None], lidar, tol=0.0, from_tanh=False)
        if cloud is not None:
            kept_rec, kept_lab, _, kept_cnt = RM.cloud_remove(cloud["raw"], cloud["counts"], cloud["idx"], remove, cloud["labels"])
            points_in = cloud["counts"].tolist()
        else:
            kept_rec, kept_cnt = S.export_points(inv_out * (source == 1)[:, None], lidar, tol=0.0, from_tanh=False)
            kept_lab, points_in = None, mask.flatten(1).sum(1).int().tolist()
        maps = torch.cat([tgt_inv, remove[:, None].float(), source[:, None].float(), inv_out], dim=1).cpu().numpy()
        sem_host, src_host = sem_out.cpu().numpy(), source.cpu().numpy()
        cnt, px = counts.tolist(), class_pixels[:, :len(CLASS_NAMES)].tolist()
        kept_n, fill_n = kept_cnt.tolist(), fill_cnt.tolist()
        for b, stem in enumerate(stems):
            nk, nf = kept_n[b], fill_n[b]
            rec = torch.cat([kept_rec[b, :nk], fill_rec[b, :nf]]).cpu().numpy()
            if kept_lab is not None:
                lab = kept_lab[b, :nk].cpu().numpy().view(np.uint32)
            else:   # a split's result: one record per measured pixel in row-major order, labelled by its pixel
                lab = sem_host[b][src_host[b] == 1].astype(np.uint32)
                if len(lab) != nk:
                    raise RuntimeError(f"{stem}: {nk} records exported for {len(lab)} measured pixels")
            lab = np.concatenate([lab, np.full(nf, args.fill_label, dtype=np.uint32)])
            for sub, name, data in (("points", f"{stem}.bin", rec.astype("<f4", copy=False)), ("labels", f"{stem}.label", lab.astype("<u4"))):
                written.append(osp.join(out_dir, sub, name))
                data.tofile(written[-1])
            written.append(osp.join(out_dir, "maps", f"{stem}.npy"))
            np.save(written[-1], maps[b])
            written.append(osp.join(out_dir, "labels_png", f"{stem}.png"))
            write_label_png(written[-1], sem_host[b])
            rows.append([stem, points_in[b], nk, nf] + cnt[b] + px[b])
        if images:
            from PIL import Image
            sides = []
            for inv, m, s in ((tgt_inv, mask, sem), (inv_out, (source > 0)[:, None].float(), sem_out)):
                pts = lidar.inv_to_xyz(inv)
                side = {"depth": inv, "mask": m, "points": pts, "normals": xyz_to_normal(pts)}
                pics = {name: (x, color, scale) for name, x, color, scale in pictures_of(side, R, t)}
                pics["label.png"] = (_label_picture(s, pal), False, 1.0)
                sides.append(pics)
            for b, stem in enumerate(stems):
                written.append(osp.join(out_dir, "images", f"{stem}.png"))
                Image.fromarray(_side_by_side(sides[0], sides[1], b, names=PICTURES)).save(written[-1])
    with open(osp.join(out_dir, "stats.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(STATS + [f"px_{c}" for c in CLASS_NAMES])
        w.writerows(rows)
    written.append(osp.join(out_dir, "stats.csv"))
    for path in written:
        print("wrote:", path)
    return out_dir


if __name__ == "__main__":
    main()
