"""Reconstruction evaluation by GAN inversion -- reference: evaluate_reconstruction.py (same flags, same CSV).

    python -m dusty_gan_amd.evaluate_reconstruction --model-path <ckpt.pth> --config-path <config.yaml>
        [--save-dir-path .] [--tol 0] [--batch-size 512] [--distance l1|l2|chamfer|emd|l1+emd|...] [--emd-points 2048]
        [--num-step 1000]
        [--num-code N --composition-layer NAME] [--corruption NAME [--corruption-seed 0]]

Every test scan is reconstructed by optimising the latent of the EMA generator (dusty_gan_amd.inversion.invert), then
scored per scan: Chamfer distance of the point clouds, depth accuracy / error, and the drop ratios.
--num-code N > 1 (beyond the reference's command: the multi-code mode of its demo, mGANprior, demo.py:353-366) optimises N
latents per scan, composed at --composition-layer (0..3, or a module name such as backbone.2: inversion.composition_layers);
a pass then takes min(batch size, 4096 // N) scans.  The CSV is the same.
--corruption NAME (beyond the reference's command: the restoration experiment of its demo, demo.py:126-137, 385-397) degrades
every target - "additive noise", "low resolution", "dropout" or "closing" (dusty_gan_amd.corruption) - and inverts against the
degraded scan; every column is still scored against the FULL scan.  Same columns, same file name."""
import argparse
import csv
import datetime
import os
import os.path as osp

COLUMNS = ["cd", "accuracy_1", "accuracy_2", "accuracy_3", "rmse", "rmse_log", "abs_rel", "sq_rel", "tol", "drop_gen",
           "drop_ref"]


TERMS = ("l1", "l2", "chamfer", "emd")


def split_distance(text):
    """"l1+chamfer" -> ("l1", "chamfer"): the terms of the inversion loss, summed (demo.py:509-519)"""
    return tuple(text.split("+"))


def _distance_arg(text):
    names = split_distance(text)
    if any(n not in TERMS for n in names):
        raise argparse.ArgumentTypeError(f"{text!r}: '+'-joined terms out of {', '.join(TERMS)}")
    return text


def _corruption_arg(text):
    from .corruption import canonical
    try:
        return canonical(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def add_inversion_arguments(parser, batch_size=512):
    """the flags every inversion command shares (this one and dusty_gan_amd.reconstruct)"""
    parser.add_argument("--model-path", type=str, required=True)
    parser.add_argument("--config-path", type=str, required=True)
    parser.add_argument("--save-dir-path", type=str, default=".")
    parser.add_argument("--tol", type=float, default=0)
    parser.add_argument("--batch-size", type=int, default=batch_size)
    parser.add_argument("--distance", default="l1", type=_distance_arg,
                        help="the inversion loss: l1 or l2 (the reference's command), or - beyond the reference's command, "
                             "which offers those two only - chamfer (the third loss of the reference's demo, demo.py:508-519) "
                             "emd (the earth mover's distance of the evaluation on --emd-points furthest-point-sampled rays "
                             "of the target) and '+'-joined sums such as l1+chamfer or l1+emd")
    parser.add_argument("--emd-points", type=int, default=2048,
                        help="with emd in --distance: the rays sampled per scan, 1..3200 and at most H W; every scan needs that "
                             "many points beyond about 3.8 m (at a max depth of 120 m)")
    parser.add_argument("--num-step", type=int, default=1000)
    parser.add_argument("--num-code", type=int, default=1,
                        help="latents per scan; above 1 (up to 64) the multi-code inversion of the reference's demo (mGANprior, "
                             "demo.py:353-366), which needs --composition-layer")
    parser.add_argument("--composition-layer", type=str, default=None,
                        help="with --num-code > 1: the feature map the codes are composed at - 0..3 (the output of Proj, Up1, "
                             "Up2, Up3) or its module name, e.g. backbone.2")
    parser.add_argument("--corruption", type=_corruption_arg, default=None,
                        help="corrupt every target before the inversion (the restoration experiment of the reference's demo, "
                             "demo.py:126-137): 'additive noise', 'low resolution', 'dropout' or 'closing' (additive_noise and "
                             "low_resolution are accepted too); the scores are against the full scan")
    parser.add_argument("--corruption-seed", type=int, default=0,
                        help="Philox seed of the corruption's draws (scan i of the dataset draws the same numbers in any batch)")


def check_inversion_arguments(parser, args):
    from .inversion import EMD_MAX_POINTS, MAX_CODES, parse_composition_layer
    if not 1 <= args.emd_points <= EMD_MAX_POINTS:
        parser.error(f"--emd-points: 1..{EMD_MAX_POINTS}")
    if not 1 <= args.num_code <= MAX_CODES:
        parser.error(f"--num-code: 1..{MAX_CODES}")
    if (args.num_code > 1) != (args.composition_layer is not None):
        parser.error("--num-code above 1 and --composition-layer go together")
    if args.composition_layer is not None:
        try:
            parse_composition_layer(args.composition_layer)
        except NotImplementedError as e:
            parser.error(str(e))


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    add_inversion_arguments(parser)
    args = parser.parse_args(argv)
    check_inversion_arguments(parser, args)
    return args


def scans_per_pass(batch_size, num_code):
    """scans of one invert call: the batch size, capped so that scans x codes stays within the lower batch's limit"""
    from .inversion import MAX_LOWER
    return batch_size if num_code == 1 else max(1, min(batch_size, MAX_LOWER // num_code))


def flatten(t):
    """utils.flatten (utils/__init__.py:213-214): [B,C,H,W] -> [B,HW,C]"""
    return t.flatten(2).permute(0, 2, 1).contiguous()


def invert_target(G, lidar, tgt_ref, tgt_mask, args, **keyed):
    """inversion.invert against (tgt_ref, tgt_mask) under a command's inversion flags (add_inversion_arguments): the one call
    evaluate_batch and remove_objects share; keyed: further arguments of invert (remove_objects keys the draws by first_index)"""
    from .inversion import invert
    names = split_distance(args.distance)
    multi = dict(num_code=args.num_code, composition_layer=args.composition_layer) if args.num_code > 1 else {}
    return invert(G, tgt_ref, tgt_mask, num_step=args.num_step, distance=names[0] if len(names) == 1 else names,
                  lidar=lidar if ("chamfer" in names or "emd" in names) else None,
                  **({"emd_points": args.emd_points} if "emd" in names else {}), **multi, **keyed)


def evaluate_batch(G, lidar, arch, item, args, first_index=0, outputs=None):
    """one batch of the reference's loop body (:80-152) -> {column: list}.  With args.corruption the latent is optimised
    against the corrupted (depth, mask) - the Chamfer term's reference points included - and every column is scored against
    the full scan (demo.py:385-397); first_index: the dataset index of the batch's first scan (keys the corruption's draws);
    outputs: a dict that receives the postprocessed generator outputs ("depth", "points", "normals", ...), the optimised
    inverse depth "inv_gen" and the inversion's target "target_inv" / "target_mask" (dusty_gan_amd.reconstruct)"""
    from .utils.lidar import postprocess
    from .utils.metrics.depth import depth_metrics
    from .utils.metrics.distance import compute_cd
    xyz, depth, mask = item["xyz"], item["depth"], item["mask"].float()
    inv = lidar.invert_depth(depth)
    inv_ref = mask * inv + (1 - mask) * 0.0   # preprocess_reals (:63-69)
    tgt_ref, tgt_mask = inv_ref, mask
    corruption = getattr(args, "corruption", None)
    if corruption is not None:
        from .corruption import apply_corruption
        dep_c, tgt_mask = apply_corruption(depth, mask, corruption, seed=getattr(args, "corruption_seed", 0), first_index=first_index)
        inv_c = lidar.invert_depth(dep_c)
        tgt_ref = tgt_mask * inv_c + (1 - tgt_mask) * 0.0   # demo.py:396-397
    res = invert_target(G, lidar, tgt_ref, tgt_mask, args)
    out = postprocess(res["out"], lidar, tol=args.tol)
    if outputs is not None:
        outputs.update(out, inv_gen=res["inv_gen"], target_inv=tgt_ref, target_mask=tgt_mask)
    cd = compute_cd(flatten(xyz.float()), flatten(out["points"]))
    if "dusty" in arch:
        keep, keep_is_depth = out["mask"], False
    else:
        keep, keep_is_depth = out["depth"], True
    m = depth_metrics(inv_ref, res["inv_gen"], mask, lidar.min_depth, lidar.max_depth, keep=keep,
                      keep_is_depth=keep_is_depth, tol=args.tol)
    B = inv_ref.shape[0]
    cols = {"cd": cd.tolist(), "tol": [args.tol] * B}
    for k in COLUMNS:
        if k not in cols:
            cols[k] = m[k].tolist()
    return cols


def write_csv(path, results):
    """pandas.DataFrame(results).to_csv(path)'s layout: an unnamed index column, then the columns in order"""
    n = len(results[COLUMNS[0]])
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow([""] + COLUMNS)
        for i in range(n):
            w.writerow([i] + [repr(float(results[k][i])) for k in COLUMNS])


def main(argv=None):
    args = parse_args(argv)
    from . import utils
    from .datasets import ScanLoader, define_dataset
    cfg, G, lidar, device = utils.setup(args.model_path, args.config_path, ema=True, fix_noise=True)
    utils.set_requires_grad(G, False)
    dataset = define_dataset(cfg.dataset, phase="test")
    loader = ScanLoader(dataset, scans_per_pass(args.batch_size, args.num_code), device, shuffle=False, drop_last=False, want_xyz=True,
                        num_workers=min(4, int(getattr(cfg, "num_workers", 4) or 1)))
    results = {k: [] for k in COLUMNS}
    for item in loader:
        for k, v in evaluate_batch(G, lidar, str(cfg.model.gen.arch), item, args, first_index=len(results["cd"])).items():
            results[k] += v
    os.makedirs(args.save_dir_path, exist_ok=True)
    save_path = osp.join(args.save_dir_path, f"{datetime.datetime.now().isoformat()}.csv")
    write_csv(save_path, results)
    print(f"Saved: {save_path}")
    return save_path


if __name__ == "__main__":
    main()
