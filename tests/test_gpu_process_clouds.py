"""python -m dusty_gan_amd.process_clouds end to end on the GPU: shuffled clouds of a synthetic 32-beam sensor in, a
`dataset=scan_folder` tree out - and that tree through the dataset, the angle grid, the trainer and `reconstruct`."""
import json
import os

import numpy as np
import pytest
import torch

from tests import beam_ref as R

pytestmark = pytest.mark.gpu
H, W, W0 = 32, 64, 128
J = 1.0e-3                     # elevation jitter of the synthetic sensor, radians
DELTA = np.pi / 8192           # the command's bin width
RECORDINGS = {"drive_a": 3, "drive_b": 3}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from dusty_gan_amd import process_clouds
    tmp = tmp_path_factory.mktemp("process_clouds")
    beams = R.uniform_beams(H)
    assert np.min(-np.diff(beams)) >= 4 * J + 4 * DELTA     # tests/test_beams_cpu.py: the recovery bound's condition
    clouds = {}
    for r, (rec, n) in enumerate(RECORDINGS.items()):
        os.makedirs(tmp / "in" / rec / "lidar")
        for i in range(n):
            pts = R.synthetic_sensor(beams, W0, seed=1000 + 10 * r + i, jitter=J, drop=0.1)
            path = tmp / "in" / rec / "lidar" / (f"{i:04d}.bin" if i != 1 else f"{i:04d}.npy")
            if i == 1:
                np.save(path, pts[:, :3])                    # an N x 3 .npy beside the .bin files
            else:
                pts.tofile(path)
            clouds[(rec, f"{i:04d}")] = (str(path), pts)
    rc = process_clouds.main(["--in-dir", str(tmp / "in"), "--out-dir", str(tmp / "out"), "--rings", str(H), "--width", str(W),
                              "--train", "drive_a", "--chunk", "2", "--num-workers", "2"])
    assert rc == 0
    return {"tmp": tmp, "out": str(tmp / "out"), "beams": beams, "clouds": clouds}


def test_files_grid_and_report(tree):
    from dusty_gan_amd.datasets.raw import project_clouds_beams
    from dusty_gan_amd.utils.lidar import LiDAR
    out = tree["out"]
    with open(os.path.join(out, "beams.json")) as f:
        rep = json.load(f)
    assert {"method", "beams_deg", "lo", "hi", "NB", "points_counted", "beam_share", "empty_cells", "beams_rad"} <= set(rep)
    table = np.asarray(rep["beams_rad"])
    assert np.allclose(np.deg2rad(rep["beams_deg"]), table, rtol=0, atol=1e-12)
    assert rep["method"] == "kmeans" and rep["NB"] == 8192 and table.shape == (H,) and np.all(np.diff(table) < 0)
    assert np.abs(table - tree["beams"]).max() <= J + DELTA / 2                     # the recovery bound
    train_points = sum(len(p) for (rec, _), (_, p) in tree["clouds"].items() if rec == "drive_a")
    assert rep["points_counted"] == train_points                                   # --train drive_a: pass 1 saw only it
    assert len(rep["beam_share"]) == H and abs(sum(rep["beam_share"]) - 1) < 1e-9
    assert max(abs(s - 1 / H) for s in rep["beam_share"]) < 0.2 / H
    assert 0 <= rep["empty_cells"] < 0.05
    for (rec, stem), (_, pts) in tree["clouds"].items():
        got = np.load(os.path.join(out, "sequences", rec, "velodyne", stem + ".npy"))
        assert got.shape == (H, W, 4) and got.dtype == np.float32
        if stem == "0001":
            pts = np.concatenate([pts[:, :3], np.zeros((len(pts), 1), np.float32)], 1)
        want = project_clouds_beams(torch.from_numpy(pts), [0, len(pts)], table, W=W)[0].cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (rec, stem)
        assert R.near_midpoint(pts, table).size == 0 and R.near_column_edge(pts, W).size == 0
        assert np.array_equal(want.view(np.uint32), R.project(pts, table, W)[0].view(np.uint32))
    assert sorted(os.listdir(os.path.join(out, "sequences"))) == sorted(RECORDINGS)
    angles = torch.load(os.path.join(out, "angles.pt"))
    assert angles.shape == (2, H, W) and angles.dtype == torch.float32 and not torch.isnan(angles).any()
    # every point lies within J of its beam, so does a row's mean elevation (float32 rounding is far below DELTA / 2)
    assert float((angles[0].double().mean(1) - torch.from_numpy(tree["beams"])).abs().max()) <= J + DELTA / 2
    lidar = LiDAR(H, W, 0.9, 120.0, angle_file=os.path.join(out, "angles.pt")).to("cuda")
    assert lidar.angle is not None and tuple(lidar.angle.shape[-2:]) == (H, W)


def test_skip_existing_keeps_the_table_the_files_were_projected_with(tree):
    """a second run with --skip-existing and another --train: beams.json stays byte for byte, the one missing file comes back
    as it was (projected with the kept table, not a new one), and a run at another --rings is refused"""
    from dusty_gan_amd import process_clouds
    out, tmp = tree["out"], tree["tmp"]
    report = open(os.path.join(out, "beams.json"), "rb").read()
    gone = os.path.join(out, "sequences", "drive_b", "velodyne", "0000.npy")
    kept = os.path.join(out, "sequences", "drive_a", "velodyne", "0000.npy")
    before, stamp = np.load(gone), os.stat(kept).st_mtime_ns
    os.remove(gone)
    argv = ["--in-dir", str(tmp / "in"), "--out-dir", out, "--width", str(W), "--train", "drive_b", "--skip-existing"]
    assert process_clouds.main(argv + ["--rings", str(H)]) == 0
    assert open(os.path.join(out, "beams.json"), "rb").read() == report
    assert np.array_equal(np.load(gone).view(np.uint32), before.view(np.uint32)) and os.stat(kept).st_mtime_ns == stamp
    assert tuple(torch.load(os.path.join(out, "angles.pt")).shape) == (2, H, W)
    with pytest.raises(ValueError, match="mix two projections"):
        process_clouds.main(argv + ["--rings", str(H // 2)])
    assert process_clouds.main(["--in-dir", str(tmp / "in"), "--out-dir", out, "--rings", str(H), "--width", str(W), "--train",
                                "drive_a", "--chunk", "2"]) == 0     # (the tree as the other tests expect it)


def test_dataset_trainer_and_reconstruct(tree):
    from dusty_gan_amd import reconstruct
    from dusty_gan_amd.datasets import ScanFolder, define_dataset
    from dusty_gan_amd.trainers.dcgan_amp import Trainer
    from dusty_gan_amd.utils.config import dump_config, load_config
    tmp = tree["tmp"]
    cfg = load_config(["model=dusty2_dcgan_eqlr", "dataset=scan_folder", f"dataset.root={tree['out']}",
                       f"dataset.shape=[{H},{W}]", "dataset.split={train: [drive_a, drive_b], val: [drive_b], test: []}",
                       "model.gen.in_ch=8", "model.gen.ch_base=4", "model.gen.ch_max=16", "model.dis.ch_base=4",
                       "model.dis.ch_max=16", "solver.batch_size=2", "enable_amp=false"])
    assert [len(define_dataset(cfg.dataset, p)) for p in ("train", "val", "test")] == [6, 3, 0]
    tr = Trainer(cfg, {"gpu": 0, "ngpus": 1, "batch_size": 2, "num_workers": 2})
    assert isinstance(tr.dataset, ScanFolder) and len(tr.dataset) == 6
    for i in range(3):   # two eager warm-up steps, then the captured step's first replay
        s = tr.step(i)
        assert all(np.isfinite(v) for v in s.values()), (i, dict(s.items()))
    assert tr._graph is not None
    ckpt = tr.save_models("scan_folder", 3, directory=str(tmp / "models"))
    dump_config(cfg, str(tmp / "config.yaml"))
    cloud = tree["clouds"][("drive_b", "0002")][0]
    out_dir = reconstruct.main(["--model-path", ckpt, "--config-path", str(tmp / "config.yaml"), "--points", cloud,
                                "--save-dir-path", str(tmp), "--num-step", "5", "--no-images"])
    target = np.load(os.path.join(out_dir, "targets", "0002.npy"))
    assert target.shape == (2, H, W) and target[1].mean() > 0.5
    assert os.path.getsize(os.path.join(out_dir, "points", "0002.bin")) > 0
    with open(os.path.join(out_dir, "scores.csv")) as f:
        rows = f.read().strip().split("\n")
    assert len(rows) == 2 and rows[1].startswith("0002,") and np.isfinite([float(v) for v in rows[1].split(",")[1:]]).all()
