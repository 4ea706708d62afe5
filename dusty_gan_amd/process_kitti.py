"""python -m dusty_gan_amd.process_kitti --root-dir ROOT

The reference's process_kitti.py (its flag, its directory layout) on the GPU:
    ROOT/dataset/sequences/XX/velodyne/NNNNNN.bin  ->  ROOT/dusty-gan/sequences/XX/velodyne/NNNNNN.npy   (64 x 2048 x 4)
    ROOT/angles.pt = the mean (elevation, azimuth) grid [2,64,2048] over the `train` split of ROOT/dusty-gan
(process_kitti.py:186-222).  With --labels the SemanticKITTI branch (:120-131) too:
    ROOT/dataset/sequences/XX/labels/NNNNNN.label  ->  ROOT/dusty-gan/sequences/XX/labels/NNNNNN.png     (64 x 2048, mode P)
for every scan that has a `.label` file: the class of the point each cell of the `.npy` holds, in the reference's palette.
"""
import argparse
import os.path as osp
import sys
from glob import glob

H, W = 64, 2048  # process_kitti.py:194


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m dusty_gan_amd.process_kitti", description=__doc__.split("\n\n")[1],
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--root-dir", type=str, required=True, help="holds dataset/sequences/*/velodyne/*.bin (KITTI odometry)")
    p.add_argument("--sequences", type=str, nargs="+", default=None, help="only these sequences (e.g. 00 03 8); default: all")
    p.add_argument("--chunk", type=int, default=16, help="scans per launch")
    p.add_argument("--num-workers", type=int, default=8, help="host threads that read .bin / write .npy files")
    p.add_argument("--skip-existing", action="store_true", help="leave .npy (and, with --labels, .png) files that already exist alone")
    p.add_argument("--labels", action="store_true",
                   help="also write the label image of every scan that has a SemanticKITTI .label file (labels/NNNNNN.label)")
    p.add_argument("--angles-only", action="store_true", help="no projection: recompute angles.pt from the existing .npy files")
    args = p.parse_args(argv)
    if args.chunk < 1 or args.num_workers < 1:
        p.error("--chunk and --num-workers must be at least 1")
    return args


def destination(point_path):
    """process_kitti.py:77,116: where the projection of a raw scan goes"""
    head, tail = osp.splitext(point_path.replace("dataset/sequences", "dusty-gan/sequences"))
    return head + ".npy" if tail == ".bin" else head + tail + ".npy"


def label_paths(point_path):
    """process_kitti.py:121-122,127: (the scan's `.label` file, where its label image goes)"""
    src = osp.splitext(point_path.replace("/velodyne", "/labels"))[0] + ".label"
    return src, osp.splitext(src.replace("dataset/sequences", "dusty-gan/sequences"))[0] + ".png"


def plan(root_dir, sequences=None, skip_existing=False, labels=False):
    """[(source .bin, destination .npy)] in the reference's order (sequence directories sorted, files sorted; :193-197).
    labels: -> (that list, [None or (source .label, destination .png)] beside it) for the scans that have a `.label` file;
    with skip_existing a destination that exists is None, and a scan with nothing left to write is not listed"""
    seq_root = osp.join(root_dir, "dataset/sequences")
    split_dirs = sorted(glob(osp.join(seq_root, "*")))
    if sequences is not None:
        want = {str(s).zfill(2) for s in sequences}
        missing = want - {osp.basename(d) for d in split_dirs}
        if missing:
            raise FileNotFoundError(f"no such sequences under {seq_root}: {sorted(missing)}")
        split_dirs = [d for d in split_dirs if osp.basename(d) in want]
    pairs, label_pairs = [], []
    for split_dir in split_dirs:
        for src in sorted(glob(osp.join(split_dir, "velodyne", "*.bin"))):
            dst = destination(src)
            lp = label_paths(src) if labels else None
            if lp is not None and not osp.exists(lp[0]):
                lp = None
            if skip_existing:
                dst = None if osp.exists(dst) else dst
                lp = None if lp is not None and osp.exists(lp[1]) else lp
            if dst is not None or lp is not None:
                pairs.append((src, dst))
                label_pairs.append(lp)
    return (pairs, label_pairs) if labels else pairs


def main(argv=None):
    args = parse_args(argv)
    root = args.root_dir
    if not args.angles_only:
        pairs, label_pairs = plan(root, args.sequences, args.skip_existing, labels=True) if args.labels else \
            (plan(root, args.sequences, args.skip_existing), None)
        if not pairs and not plan(root, args.sequences):
            raise FileNotFoundError(f"no raw scans: {osp.join(root, 'dataset/sequences', '*', 'velodyne', '*.bin')} matches nothing")
        from .datasets.raw import project_files
        n = project_files(pairs, W=W, chunk=args.chunk, num_workers=args.num_workers, label_pairs=label_pairs)
        print(f"projected {n} scans into {osp.join(root, 'dusty-gan/sequences')}")
        if label_pairs is not None:
            print(f"label images: {sum(lp is not None for lp in label_pairs)}")
    # average angles over the train split (:207-222)
    import torch

    from .datasets.raw import average_angles
    from .datasets.scans import KITTIOdometry
    dataset = KITTIOdometry(root=osp.join(root, "dusty-gan"), split="train", shape=(H, W))
    if len(dataset) == 0:
        if args.angles_only:
            raise FileNotFoundError(f"no projected scans of the train split under {dataset.root}")
        print(f"no scans of the train split under {dataset.root}: angles.pt not written")
        return 0
    angles = average_angles(dataset, chunk=args.chunk, num_workers=args.num_workers)
    torch.save(angles.cpu(), osp.join(root, "angles.pt"))
    print(f"angles.pt: {len(dataset)} scans of the train split")
    return 0


if __name__ == "__main__":
    sys.exit(main())
