"""Synthesis evaluation -- reference: evaluate_synthesis.py (same flags, same JSON keys, same file names).

    python -m dusty_gan_amd.evaluate_synthesis --model-path <ckpt.pth> --config-path <config.yaml>
        [--save-dir-path .] [--num-test 5000] [--num-points 2048] [--tol 0] [--compute-gt] [--cache-dir data]

Generated scans of the EMA generator against the real test scans: SWD on the inverse-depth images, JSD on the halved
point clouds, COV / MMD / 1-NNA (Chamfer) on clouds of `--num-points` points.  Every cloud is downsampled where its
point map lies (utils.sampling.downsample_point_map): the real scans' own "xyz" maps and the generated depth's
projection (LiDAR.inv_to_xyz with `--tol`).  The real sets are cached per (dataset, subset, num_points).
Two deviations from the reference: the `train` set is read only under --compute-gt (the reference builds it always and
uses it only there), and --cache-dir names the cache directory (the reference's "data" is the default)."""
import argparse
import datetime
import json
import os
import os.path as osp
import pprint


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--model-path", type=str, required=True)
    parser.add_argument("--config-path", type=str, required=True)
    parser.add_argument("--save-dir-path", type=str, default=".")
    parser.add_argument("--num-test", type=int, default=5000)
    parser.add_argument("--num-points", type=int, default=2048)
    parser.add_argument("--tol", type=float, default=0)
    parser.add_argument("--compute-gt", action="store_true")
    parser.add_argument("--cache-dir", type=str, default="data",
                        help="where cache_{dataset}_{subset}_{num_points}.pt is kept (created if missing)")
    return parser.parse_args(argv)


def subsample(t, num_test):
    """the reference's time-series rule (:102-110): every `skip`-th item from `skip` on, `num_test` of them; -1: all"""
    if num_test == -1:
        return t
    if len(t) < num_test:
        raise ValueError(f"the set holds {len(t)} items, fewer than --num-test {num_test}")
    skip = len(t) // num_test
    return t[skip:skip * num_test + 1:skip]


def real_2d(lidar, depth, mask, drop_const):
    """preprocess_reals (:49-57): normalised depth -> inverse depth in [-1,1], dropped pixels = drop_const"""
    from .utils import sigmoid_to_tanh
    mask = mask.float()
    inv = sigmoid_to_tanh(lidar.invert_depth(depth))
    return mask * inv + (1 - mask) * drop_const


def cache_path(cfg, subset, num_points, cache_dir):
    return osp.join(cache_dir, f"cache_{cfg.dataset.name}_{subset}_{num_points}.pt")


def real_sets(cfg, lidar, device, subset, num_points, cache_dir="data"):
    """{"2d" [N,1,H,W], "3d" [N,num_points,3]} of a dataset split, CPU tensors (:69-97): read from the cache file when
    there is one, else built from the split's scans and cached"""
    import torch

    from . import datasets
    from .utils.sampling import downsample_point_map
    path = cache_path(cfg, subset, num_points, cache_dir)
    if osp.exists(path):
        reals = torch.load(path, map_location="cpu")
        print("loaded:", path)
        return reals
    loader = datasets.ScanLoader(datasets.define_dataset(cfg.dataset, phase=subset), int(cfg.solver.batch_size), device,
                                 shuffle=False, drop_last=False, want_xyz=True,
                                 num_workers=min(4, int(getattr(cfg, "num_workers", 4) or 1)))
    reals = {"2d": [], "3d": []}
    for item in loader:
        reals["2d"].append(real_2d(lidar, item["depth"], item["mask"], float(cfg.model.gen.drop_const)).cpu())
        reals["3d"].append(downsample_point_map(item["xyz"], num_points).cpu())
    reals = {k: torch.cat(v, dim=0) for k, v in reals.items()}
    os.makedirs(cache_dir, exist_ok=True)
    torch.save(reals, path)
    print("cached:", path)
    return reals


def load_reals(cfg, lidar, device, subset, args):
    """a split's real sets, subsampled to --num-test, on the device"""
    reals = real_sets(cfg, lidar, device, subset, args.num_points, args.cache_dir)
    reals = {mode: subsample(t, args.num_test).to(device) for mode, t in reals.items()}
    for mode, t in reals.items():
        print("real", subset, mode, tuple(t.shape))
    return reals


def synthetic_2d(cfg, G, device, n, latents=None, seed=0):
    """n generated inverse-depth images [n,1,H,W] (:149-163): `solver.batch_size` latents per call from the engine's Philox
    stream, or the rows of `latents` [>= n, in_ch] in batches of that size"""
    import torch

    from .utils.rng import Philox
    B, nz = int(cfg.solver.batch_size), int(cfg.model.gen.in_ch)
    rng = Philox(seed, device) if latents is None else None
    out = []
    for i in range(0, n, B):
        if latents is None:
            latent = rng.normal(B * nz).view(B, nz)
        else:   # every call is a full batch, as above: a short last slice is filled up with zeros, cut off again below
            latent = torch.zeros(B, nz, device=device)
            latent[:len(latents[i:i + B])] = latents[i:i + B]
        # (the generator returns views of its persistent workspace: keep a copy, not the view)
        out.append(G(latent=latent)["depth"].clone())
    return torch.cat(out, dim=0)[:n]


def project_2d_to_3d(lidar, inv, tol, num_points, batch_size):
    """generated inverse depth [N,1,H,W] in [-1,1] -> [N,num_points,3] (:59-64), a batch at a time: the point map with
    pixels under `tol` dropped, sampled where it lies"""
    import torch

    from .utils.sampling import downsample_point_map
    return torch.cat([downsample_point_map(lidar.inv_to_xyz(inv[i:i + batch_size], tol, from_tanh=True), num_points)
                      for i in range(0, len(inv), batch_size)], dim=0)


def synthetic_sets(cfg, G, lidar, device, n, num_points, tol, latents=None, seed=0):
    """{"2d" [n,1,H,W], "3d" [n,num_points,3]} of generated scans, on the device"""
    inv = synthetic_2d(cfg, G, device, n, latents=latents, seed=seed)
    return {"2d": inv, "3d": project_2d_to_3d(lidar, inv, tol, num_points, int(cfg.solver.batch_size))}


def compute_scores(gen, ref, num_test, num_points, swd_rand=None):
    """the reference's score dict (:168-186) of a generated (or train) set against a real one"""
    from .utils.metrics import compute_cov_mmd_1nna, compute_jsd, compute_swd
    scores = {}
    scores.update(compute_swd(gen["2d"], ref["2d"], rand=swd_rand))
    scores["jsd"] = compute_jsd(gen["3d"] / 2.0, ref["3d"] / 2.0)
    scores.update(compute_cov_mmd_1nna(gen["3d"], ref["3d"], 512, ("cd",)))
    scores["#test"] = num_test
    scores["#points"] = num_points
    return scores


def write_scores(scores, path):
    with open(path, "w") as f:
        json.dump(scores, f, ensure_ascii=False, indent=4, sort_keys=True)


def main(argv=None, swd_rand=None, return_data=False):
    """-> the path written; with return_data also the sets that were scored, {"gen": {"2d","3d"}, "ref": {...}}.
    `swd_rand`: compute_swd's draws, for tests (as Trainer.validation)"""
    args = parse_args(argv)
    from . import utils
    cfg, G, lidar, device = utils.setup(args.model_path, args.config_path, ema=True, fix_noise=True)
    utils.set_requires_grad(G, False)
    test = load_reals(cfg, lidar, device, "test", args)
    timestamp = datetime.datetime.now().isoformat()
    if args.compute_gt:
        print("training set only")
        gen = load_reals(cfg, lidar, device, "train", args)
        scores = compute_scores(gen, test, args.num_test, args.num_points, swd_rand)
        pprint.pprint(scores)
        gt_dir = f"outputs/logs/dataset={cfg.dataset.name}/gt/evaluation/tol=0"
        os.makedirs(gt_dir, exist_ok=True)
        save_path = osp.join(gt_dir, f"{timestamp}.json")
        write_scores(scores, save_path)
        return (save_path, {"gen": gen, "ref": test}) if return_data else save_path
    gen = synthetic_sets(cfg, G, lidar, device, len(test["2d"]), args.num_points, args.tol)
    scores = compute_scores(gen, test, args.num_test, args.num_points, swd_rand)
    pprint.pprint(scores)
    os.makedirs(args.save_dir_path, exist_ok=True)
    save_path = osp.join(args.save_dir_path, f"{timestamp}.csv")   # (JSON under the reference's own extension)
    write_scores(scores, save_path)
    print(f"Saved: {save_path}")
    return (save_path, {"gen": gen, "ref": test}) if return_data else save_path


if __name__ == "__main__":
    main()
