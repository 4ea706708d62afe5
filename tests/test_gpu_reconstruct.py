"""python -m dusty_gan_amd.reconstruct on the GPU: cloud files in, scores / projected targets / reconstructed clouds /
pictures out.  The clouds are the generator's own outputs for known latents, written as KITTI .bin files of different
length, one of them with its records shuffled."""
import csv
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_synthesis import make_world

pytestmark = pytest.mark.gpu
STEMS = ["scan_a", "scan_b", "scan_c"]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from dusty_gan_amd import synthesis as S
    from dusty_gan_amd import utils
    tmp = tmp_path_factory.mktemp("reconstruct")
    argv = make_world(tmp, "dusty2_dcgan_eqlr", "dusty2")
    cfg, G, lidar, device = utils.setup(argv[1], argv[3], ema=True, fix_noise=True)
    out = S.synthesize(cfg, G, lidar, S.sample_latents(cfg, device, 3, "random", 3), normals=False)
    records, counts = S.export_points(out["depth"], lidar, tol=0.0, from_tanh=False)
    clouds = tmp / "clouds"
    clouds.mkdir()
    rng = np.random.default_rng(2)
    rows = []
    for b, stem in enumerate(STEMS):
        rec = records[b, :int(counts[b])].cpu().numpy()
        if b == 1:
            rec = rec[: int(0.6 * len(rec))]          # a shorter cloud: the batch is padded
        if b == 2:
            rec = rec[rng.permutation(len(rec))]      # no point order
        rec.tofile(clouds / f"{stem}.bin")
        rows.append(len(rec))
    assert len(set(rows)) == 3 and min(rows) > 1000
    return {"tmp": tmp, "argv": argv, "lidar": lidar, "device": device, "clouds": clouds, "rows": rows}


def read_scores(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def check_scores_and_targets(world, out_dir, tau=2.0):
    from dusty_gan_amd.datasets.raw import read_clouds
    from dusty_gan_amd.evaluate_reconstruction import COLUMNS
    lidar = world["lidar"]
    table = read_scores(os.path.join(out_dir, "scores.csv"))
    assert table[0] == ["name"] + COLUMNS and [r[0] for r in table[1:]] == STEMS
    assert all(np.isfinite([float(v) for v in r[1:]]).all() for r in table[1:])
    for stem, rows in zip(STEMS, world["rows"]):
        got = np.load(os.path.join(out_dir, "targets", f"{stem}.npy"))
        assert got.shape == (2, 64, 1024) and got.dtype == np.float32
        rec, counts = read_clouds([world["clouds"] / f"{stem}.bin"], lidar.max_depth, world["device"])   # alone: no padding
        assert counts.tolist() == [rows]
        depth, valid = lidar.points_to_depth(rec, drop_value=1, tau=tau, counts=counts)
        want = torch.cat([depth, valid.float()], dim=1)[0].cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), stem
        # every record came from a pixel of its own, so every record lights one pixel, in any order
        assert int(got[1].sum()) == rows and (got[0][got[1] == 0] == 1.0).all()
    return table


def test_plain_run_writes_scores_targets_clouds_and_pictures(world, monkeypatch):
    from PIL import Image

    from dusty_gan_amd import reconstruct
    from dusty_gan_amd import synthesis as S
    exported = []   # what export_points handed the writer: (records, counts) of the one batch
    real_export = S.export_points
    monkeypatch.setattr(S, "export_points", lambda *a, **k: exported.append(real_export(*a, **k)) or exported[-1])
    save = str(world["tmp"] / "plain")
    out_dir = reconstruct.main(world["argv"] + ["--points", str(world["clouds"]), "--save-dir-path", save, "--num-step", "20"])
    assert out_dir == os.path.join(save, "reconstruction")
    assert sorted(os.listdir(out_dir)) == ["images", "points", "scores.csv", "targets"]
    for sub, ext in (("images", ".png"), ("points", ".bin"), ("targets", ".npy")):
        assert sorted(os.listdir(os.path.join(out_dir, sub))) == [s + ext for s in STEMS]
    table = check_scores_and_targets(world, out_dir)
    lidar = world["lidar"]
    assert len(exported) == 1 and exported[0][1].shape == (3,)
    for b, stem in enumerate(STEMS):
        size = os.path.getsize(os.path.join(out_dir, "points", f"{stem}.bin"))
        rec = np.fromfile(os.path.join(out_dir, "points", f"{stem}.bin"), np.float32).reshape(-1, 4)
        assert size % 16 == 0 and 0 < len(rec) <= 64 * 1024 and np.isfinite(rec).all() and (rec[:, 3] == 0).all()
        k = int(exported[0][1][b])
        assert len(rec) == k and np.array_equal(rec.view(np.int32), exported[0][0][b, :k].cpu().numpy().view(np.int32)), stem
        assert float(np.linalg.norm(rec[:, :3], axis=1).max()) <= lidar.max_depth * 1.001
        img = np.asarray(Image.open(os.path.join(out_dir, "images", f"{stem}.png")))
        # three rows (inverse depth, mask, bird's-eye view) of target beside reconstruction
        assert img.shape == (2 * (64 + 2) + 2 * 2 + 512 + 2 + 2, 2 * (1024 + 2) + 2, 3) and img.max() > 0
    # the drop ratio of the target is what the file covers
    col = table[0].index("drop_ref")
    for r, stem in zip(table[1:], STEMS):
        target = np.load(os.path.join(out_dir, "targets", f"{stem}.npy"))
        assert abs(float(r[col]) - (1.0 - target[1].astype(np.float64).mean())) < 1e-6


def test_restoration_run_without_pictures_and_clouds(world):
    from dusty_gan_amd import reconstruct
    save = str(world["tmp"] / "restore")
    files = [str(world["clouds"] / f"{s}.bin") for s in STEMS]
    out_dir = reconstruct.main(world["argv"] + ["--points"] + files + ["--save-dir-path", save, "--num-step", "20", "--corruption",
                                                                       "dropout", "--distance", "l1+chamfer", "--no-images", "--no-bins"])
    assert sorted(os.listdir(out_dir)) == ["scores.csv", "targets"]
    check_scores_and_targets(world, out_dir)   # the targets on file are the full projections, not the corrupted ones


def test_baseline_checkpoint(tmp_path):
    from dusty_gan_amd import reconstruct
    argv = make_world(tmp_path, "dcgan_eqlr", "none")
    rng = np.random.default_rng(4)
    ray = rng.normal(size=(5000, 3))
    ray[:, 2] = -np.abs(ray[:, 2]) * 0.2
    pts = ray / np.linalg.norm(ray, axis=1, keepdims=True) * rng.uniform(3.0, 80.0, (5000, 1))
    np.save(tmp_path / "sim.npy", pts.astype(np.float32))     # an N x 3 .npy from no sensor at all
    out_dir = reconstruct.main(argv + ["--points", str(tmp_path / "sim.npy"), "--save-dir-path", str(tmp_path), "--num-step", "5"])
    table = read_scores(os.path.join(out_dir, "scores.csv"))
    assert [r[0] for r in table[1:]] == ["sim"] and np.isfinite([float(v) for v in table[1][1:]]).all()
    for rel in ("targets/sim.npy", "points/sim.bin", "images/sim.png"):
        assert os.path.getsize(os.path.join(out_dir, rel)) > 0
