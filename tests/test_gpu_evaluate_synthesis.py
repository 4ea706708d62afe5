"""The synthesis evaluation and the tolerance sweep end to end on the MI355X (dusty_gan_amd/evaluate_synthesis.py,
dusty_gan_amd/tune_tolerance.py): a seeded full-width dusty2 generator at 64x1024, a few .npy scans per split, batches
of 4 (a full and a ragged one), clouds of 64 points."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NUM_POINTS = 64


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """scans (train 00: 7, val 08: 5, test 11: 7), config.yaml and model.pth -> paths and the loaded setup"""
    from dusty_gan_amd import utils
    from dusty_gan_amd.models import define_G
    from dusty_gan_amd.utils.config import dump_config, load_config
    from tests.test_gpu_data import write_kitti_tree
    tmp = tmp_path_factory.mktemp("synthesis")
    root = str(tmp / "kitti")
    write_kitti_tree(root, 64, 2048, {0: 7, 8: 5, 11: 7})
    cfg = load_config(["model=dusty2_dcgan_eqlr", "dataset=kitti_odometry", f"dataset.root={root}",
                       "dataset.shape=[64,1024]", "solver.batch_size=4", "enable_amp=true"])
    cfg_path, ckpt = str(tmp / "config.yaml"), str(tmp / "model.pth")
    dump_config(cfg, cfg_path)
    torch.manual_seed(0)
    cfg.model.gen.shape = cfg.dataset.shape
    sd = define_G(cfg).state_dict()
    # A freshly initialised generator's inverse depths stay within 0.5 +- 0.2: every point then lies inside the 3.8 m
    # (|p|^2 < 1e-3 in unit space) that furthest point sampling skips, and no pixel is near either tolerance.  The depth
    # head is scaled and shifted so that the depths spread from a few metres to the far end.
    sd["backbone.4.heads.depth.1.module.weight"] *= 10.0
    sd["backbone.4.heads.depth.1.module.bias"] -= 1.5
    torch.save({"step": 0, "G_ema": sd}, ckpt)
    cfg, G, lidar, device = utils.setup(ckpt, cfg_path, ema=True, fix_noise=True)
    return {"tmp": tmp, "argv": ["--model-path", ckpt, "--config-path", cfg_path, "--num-points", str(NUM_POINTS)],
            "cfg": cfg, "G": G, "lidar": lidar, "device": device}


def test_real_sets_and_their_cache(world, monkeypatch):
    from dusty_gan_amd import datasets
    from dusty_gan_amd import evaluate_synthesis as E
    from dusty_gan_amd.utils import sigmoid_to_tanh
    from dusty_gan_amd.utils.sampling import downsample_point_clouds
    cfg, lidar, device = world["cfg"], world["lidar"], world["device"]
    cache = str(world["tmp"] / "cache_a")
    got = E.real_sets(cfg, lidar, device, "test", NUM_POINTS, cache)
    want2d, want3d, sizes = [], [], []
    for item in datasets.ScanLoader(datasets.define_dataset(cfg.dataset, phase="test"), 4, device, shuffle=False,
                                    drop_last=False, want_xyz=True):
        mask = item["mask"].float()
        inv = sigmoid_to_tanh(lidar.invert_depth(item["depth"]))
        want2d.append((mask * inv + (1 - mask) * cfg.model.gen.drop_const).cpu())
        want3d.append(downsample_point_clouds(item["xyz"].flatten(2).transpose(1, 2).contiguous(), NUM_POINTS).cpu())
        sizes.append(len(mask))
    assert sizes == [4, 3]
    assert set(got) == {"2d", "3d"} and not got["2d"].is_cuda and not got["3d"].is_cuda
    assert got["2d"].shape == (7, 1, 64, 1024) and got["3d"].shape == (7, NUM_POINTS, 3)
    assert torch.equal(got["2d"], torch.cat(want2d)) and torch.equal(got["3d"], torch.cat(want3d))
    dropped = got["2d"] == cfg.model.gen.drop_const
    assert 0 < int(dropped.sum()) < dropped.numel()
    path = os.path.join(cache, f"cache_{cfg.dataset.name}_test_{NUM_POINTS}.pt")
    assert os.path.exists(path) and E.cache_path(cfg, "test", NUM_POINTS, cache) == path
    assert set(torch.load(path)) == {"2d", "3d"}   # loads under torch.load's safe default

    def no_dataset(*a, **k):
        raise AssertionError("the cache was not used")
    monkeypatch.setattr(datasets, "define_dataset", no_dataset)
    again = E.real_sets(cfg, lidar, device, "test", NUM_POINTS, cache)
    assert torch.equal(again["2d"], got["2d"]) and torch.equal(again["3d"], got["3d"])
    with pytest.raises(AssertionError):
        E.real_sets(cfg, lidar, device, "val", NUM_POINTS, cache)   # no cache for that split: it would read the scans


def test_synthetic_sets_equal_the_packed_path(world):
    from dusty_gan_amd import evaluate_synthesis as E
    from dusty_gan_amd.utils.sampling import downsample_point_clouds
    cfg, G, lidar, device = world["cfg"], world["G"], world["lidar"], world["device"]
    latents = torch.randn(7, int(cfg.model.gen.in_ch), generator=torch.Generator().manual_seed(5))
    sets = {}
    for tol in (0.0, 0.05):
        s = sets[tol] = E.synthetic_sets(cfg, G, lidar, device, 7, NUM_POINTS, tol, latents=latents)
        assert s["2d"].shape == (7, 1, 64, 1024) and s["3d"].shape == (7, NUM_POINTS, 3)
        xyz = lidar.inv_to_xyz(s["2d"], tol, from_tanh=True)
        want = downsample_point_clouds(xyz.flatten(2).transpose(1, 2).contiguous(), NUM_POINTS)
        assert torch.equal(s["3d"], want), tol
        assert float(s["3d"].abs().amax(dim=(1, 2)).min()) > 0.0   # every cloud has points beyond the skipped origin
    assert torch.equal(sets[0.0]["2d"], sets[0.05]["2d"])
    assert len({float(sets[0.0]["2d"][i].sum()) for i in range(7)}) == 7   # copies, not 7 views of one workspace
    assert not torch.equal(sets[0.0]["3d"], sets[0.05]["3d"])
    own = E.synthetic_2d(cfg, G, device, 7)     # the engine's own latents: seeded, so repeatable
    assert own.shape == (7, 1, 64, 1024) and torch.equal(own, E.synthetic_2d(cfg, G, device, 7))
    assert not torch.equal(own, sets[0.0]["2d"])


def swd_draws(H, W, levels):
    from oracle import metrics_oracle as MO
    g = torch.Generator().manual_seed(11)
    one = [torch.randperm(c, generator=g)[:128] for c in MO.swd_patch_counts(H, W, levels)]
    return {"inds": [[one, one]], "dirs": [[torch.randn(49, 128, generator=g) for _ in range(4)] for _ in range(levels)]}


def check_scores(path, data, rand, num_test):
    from dusty_gan_amd.utils.metrics import compute_cov_mmd_1nna, compute_jsd, compute_swd
    gen, ref = data["gen"], data["ref"]
    assert gen["2d"].shape == ref["2d"].shape == (3, 1, 64, 1024) and gen["3d"].shape == ref["3d"].shape == (3, NUM_POINTS, 3)
    swd = compute_swd(gen["2d"], ref["2d"], rand=rand)
    cov = compute_cov_mmd_1nna(gen["3d"], ref["3d"], 512, ("cd",))
    want = {**swd, **cov, "jsd": compute_jsd(gen["3d"] / 2.0, ref["3d"] / 2.0), "#test": num_test, "#points": NUM_POINTS}
    got = json.load(open(path))
    assert set(got) == set(swd) | set(cov) | {"jsd", "#test", "#points"}
    assert all(np.isfinite(v) for v in got.values())
    assert got == want
    text = open(path).read()
    assert text == json.dumps(got, ensure_ascii=False, indent=4, sort_keys=True)
    return got


def test_main_writes_the_reference_scores(world, monkeypatch):
    from dusty_gan_amd import evaluate_synthesis as E
    tmp = world["tmp"]
    monkeypatch.chdir(tmp)
    rand = swd_draws(64, 1024, 3)
    out_dir, cache = str(tmp / "out"), str(tmp / "cache_b")
    argv = world["argv"] + ["--num-test", "3", "--cache-dir", cache]
    path, data = E.main(argv + ["--save-dir-path", out_dir, "--tol", "0.05"], swd_rand=rand, return_data=True)
    assert os.path.dirname(path) == out_dir and path.endswith(".csv")
    got = check_scores(path, data, rand, 3)
    assert {"swd-16", "swd-32", "swd-64", "swd-mean", "jsd", "cov-cd", "mmd-cd", "1-nn-accuracy-cd"} <= set(got)
    assert os.listdir(cache) == [f"cache_{world['cfg'].dataset.name}_test_{NUM_POINTS}.pt"]   # `train` was not built
    # the test set is items 2, 4, 6 of the split (skip = 7 // 3)
    full = E.real_sets(world["cfg"], world["lidar"], world["device"], "test", NUM_POINTS, cache)
    assert torch.equal(data["ref"]["3d"].cpu(), full["3d"][[2, 4, 6]])
    path, data = E.main(argv + ["--compute-gt"], swd_rand=rand, return_data=True)
    gt_dir = os.path.join("outputs", "logs", f"dataset={world['cfg'].dataset.name}", "gt", "evaluation", "tol=0")
    assert os.path.dirname(path) == gt_dir and path.endswith(".json") and os.path.exists(tmp / path)
    check_scores(path, data, rand, 3)
    train = E.real_sets(world["cfg"], world["lidar"], world["device"], "train", NUM_POINTS, cache)
    assert torch.equal(data["gen"]["3d"].cpu(), train["3d"][[2, 4, 6]])
    plain = E.main(argv + ["--save-dir-path", out_dir])   # as the command calls it: the path alone, --tol 0
    assert isinstance(plain, str) and os.path.exists(plain) and plain != path
    with pytest.raises(ValueError):
        E.main(world["argv"] + ["--num-test", "8", "--cache-dir", cache])


def test_tune_tolerance_sweep(world):
    from dusty_gan_amd import tune_tolerance as T
    from dusty_gan_amd.utils.metrics import compute_cov_mmd_1nna, compute_jsd
    tmp = world["tmp"]
    out_dir, cache = str(tmp / "tune"), str(tmp / "cache_c")
    path, data = T.main(world["argv"] + ["--tols", "0.001", "0.05", "--save-dir-path", out_dir, "--cache-dir", cache],
                        return_data=True)
    assert path == os.path.join(out_dir, "tol_tuning", "best_config.json")
    trials = [json.loads(line) for line in open(os.path.join(out_dir, "tol_tuning", "trials.jsonl"))]
    assert [t["config"]["tol"] for t in trials] == [0.001, 0.05]
    ref = data["ref"]["3d"]
    assert ref.shape == (5, NUM_POINTS, 3)   # --num-test -1: the whole val split
    for t in trials:
        gen = data["gen-3d"][t["config"]["tol"]]
        want = compute_cov_mmd_1nna(gen, ref, 512, ("cd",), verbose=False)   # without M_rr: the reuse changes nothing
        for k, v in want.items():
            assert t[k] == v, k
        assert t["jsd"] == compute_jsd(gen / 2.0, ref / 2.0) and t["#points"] == NUM_POINTS
        assert t["weighted"] == T.weighted(t) and np.isfinite(t["weighted"])
        assert t["config"] == {"tol": t["config"]["tol"], "num_points": NUM_POINTS, "batch_size": 4}
    best = json.load(open(path))
    assert set(best) == {"tol", "num_points", "batch_size"}
    assert best == min(trials, key=lambda t: t["weighted"])["config"]
    assert not torch.equal(data["gen-3d"][0.001], data["gen-3d"][0.05])
