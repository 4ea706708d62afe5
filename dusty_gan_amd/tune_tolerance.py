"""Tolerance search -- reference: tune_tolerance.py (its objective, its search lattice, its best_config.json), without
ray / hyperopt: a deterministic sweep.

    python -m dusty_gan_amd.tune_tolerance --model-path <ckpt.pth> --config-path <config.yaml>
        [--num-test -1] [--num-points 2048] [--num-samples 100 | --tols T [T ...]] [--save-dir-path .] [--cache-dir data]

`tol` is the threshold under which a generated pixel counts as dropped when the depth image becomes a point cloud
(LiDAR.inv_to_xyz); the value found is what evaluate_synthesis takes as --tol.  Computed once: the `val` real set (the
cache of evaluate_synthesis), the generated inverse-depth images and the real-against-real Chamfer matrix.  Per
candidate: projection with that tolerance, furthest point sampling on the point map, the two matrices that involve the
generated clouds, COV / MMD / 1-NNA and JSD.
The reference samples `tune.qloguniform(1e-3, 1e-1, 5e-4)` 100 times under hyperopt; here the candidates are a fixed
log-spaced walk over the same lattice (multiples of 5e-4 in [1e-3, 1e-1]), so two runs try the same values."""
import argparse
import json
import os
import os.path as osp

TOL_LO, TOL_HI, TOL_Q = 1e-3, 1e-1, 5e-4   # tune.qloguniform(1e-3, 1e-1, 5e-4) (:175)


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--model-path", type=str, required=True)
    parser.add_argument("--config-path", type=str, required=True)
    parser.add_argument("--num-test", type=int, default=-1)
    parser.add_argument("--num-points", type=int, default=2048)
    parser.add_argument("--num-samples", type=int, default=100, help="candidates, log-spaced over the lattice (:180)")
    parser.add_argument("--tols", type=float, nargs="+", default=None, help="an explicit candidate list instead")
    parser.add_argument("--save-dir-path", type=str, default=".")
    parser.add_argument("--cache-dir", type=str, default="data")
    return parser.parse_args(argv)


def candidates(num_samples):
    """numpy.geomspace(1e-3, 1e-1, num_samples) rounded to the nearest lattice point: ascending, without repeats"""
    import numpy as np
    steps = np.rint(np.geomspace(TOL_LO, TOL_HI, num_samples) / TOL_Q).astype(np.int64)
    steps = np.clip(steps, int(round(TOL_LO / TOL_Q)), int(round(TOL_HI / TOL_Q)))
    return [float(round(int(s) * TOL_Q, 10)) for s in sorted(set(steps.tolist()))]


def weighted(scores):
    """the reference's objective (:52-57), minimised"""
    return (1.0 * scores["1-nn-accuracy-cd"] + 100 * scores["mmd-cd"] + -1.0 * scores["cov-cd"] + 10 * scores["jsd"])


def evaluation(config, fakes_2d, reals_3d, lidar, M_rr=None):
    """one trial (:21-59): config {"tol", "num_points", "batch_size"} -> the scores with "weighted", and the generated clouds"""
    from .evaluate_synthesis import project_2d_to_3d
    from .utils.metrics import compute_cov_mmd_1nna, compute_jsd
    fakes_3d = project_2d_to_3d(lidar, fakes_2d, config["tol"], config["num_points"], config["batch_size"])
    scores = compute_cov_mmd_1nna(fakes_3d, reals_3d, 512, ("cd",), verbose=False, M_rr=M_rr)
    scores["jsd"] = compute_jsd(fakes_3d / 2.0, reals_3d / 2.0)
    scores["#points"] = config["num_points"]
    scores["weighted"] = weighted(scores)
    return scores, fakes_3d


def main(argv=None, return_data=False):
    """-> the path of best_config.json; with return_data also {"ref", "gen-2d", "gen-3d": {tol: clouds}}"""
    args = parse_args(argv)
    from . import utils
    from .evaluate_synthesis import load_reals, synthetic_2d
    from .utils.metrics.distance import chamfer_distance_matrix
    cfg, G, lidar, device = utils.setup(args.model_path, args.config_path, ema=True, fix_noise=True)
    utils.set_requires_grad(G, False)
    reals = load_reals(cfg, lidar, device, "val", args)
    fakes_2d = synthetic_2d(cfg, G, device, len(reals["2d"]))
    M_rr = chamfer_distance_matrix(reals["3d"], reals["3d"])
    out_dir = osp.join(args.save_dir_path, "tol_tuning")
    os.makedirs(out_dir, exist_ok=True)
    best, data = None, {"ref": reals, "gen-2d": fakes_2d, "gen-3d": {}}
    for tol in (args.tols if args.tols is not None else candidates(args.num_samples)):
        config = {"tol": float(tol), "num_points": args.num_points, "batch_size": int(cfg.solver.batch_size)}
        scores, fakes_3d = evaluation(config, fakes_2d, reals["3d"], lidar, M_rr)
        if return_data:
            data["gen-3d"][float(tol)] = fakes_3d
        with open(osp.join(out_dir, "trials.jsonl"), "a") as f:
            f.write(json.dumps({"config": config, **scores}, sort_keys=True) + "\n")
        print(f"tol {tol:g}: weighted {scores['weighted']:.6f}")
        if best is None or scores["weighted"] < best[0]:
            best = (scores["weighted"], config)
    print("Best config: ", best[1])
    path = osp.join(out_dir, "best_config.json")
    with open(path, "w") as f:
        json.dump(best[1], f, ensure_ascii=False, indent=4, sort_keys=True)
    return (path, data) if return_data else path


if __name__ == "__main__":
    main()
