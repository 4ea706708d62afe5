"""The host side of training on any spinning LiDAR (dusty_gan_amd/datasets/beams.py, datasets/scans.py ScanFolder,
dusty_gan_amd/process_clouds.py) and the reference the GPU tests rest on (tests/beam_ref.py).  No GPU."""
import os

import numpy as np
import pytest

from tests import beam_ref as R

LO, HI = -np.pi / 2, np.pi / 2


# ------------------------------------------------------------------------------------------------ estimate_beams
def test_kmeans_recovers_a_non_uniform_sensor_within_the_derived_bound():
    """8 beams, equal populations, jitter j, bin width delta, spacing >= 4 j + 4 delta.  Every point lies within j of its beam
    and every bin centre within delta / 2 of its points, so a cluster's weighted mean lies within j + delta / 2 of its beam
    once the bins are assigned correctly; the quantile starts lie inside their clusters (equal populations), where the next
    cluster's start is at least spacing - 2 j - delta >= 2 j + 3 delta away: further than the cluster's own extent."""
    from dusty_gan_amd.datasets.beams import estimate_beams
    NB, j = 8192, 1.0e-3
    delta = (HI - LO) / NB
    beams = np.deg2rad([2.0, 0.5, -1.0, -3.0, -5.5, -8.0, -12.0, -16.0])
    assert np.min(-np.diff(beams)) >= 4 * j + 4 * delta
    pts = R.synthetic_sensor(beams, 512, seed=11, jitter=j)
    u = R.elevation(pts)
    assert np.abs(u[:, None] - beams[None, :]).min(1).max() <= j            # every point within j of a beam ...
    assert np.bincount(R.nearest_beam(u, beams), minlength=8).tolist() == [512] * 8   # ... in equal numbers
    hist = R.histogram(pts, 0.9, 120.0, LO, HI, NB)
    assert hist.sum() == len(pts)
    got = estimate_beams(hist, 8, LO, HI)
    assert got.dtype == np.float64 and got.shape == (8,) and np.all(np.diff(got) < 0)
    assert np.abs(got - beams).max() <= j + delta / 2, np.abs(got - beams).max()


def test_uniform_mode_and_table_file(tmp_path):
    from dusty_gan_amd.datasets.beams import beam_shares, estimate_beams
    hist = R.histogram(R.synthetic_sensor(R.uniform_beams(16), 256, seed=3, jitter=2e-4), 0.9, 120.0, LO, HI, 4096)
    got = estimate_beams(hist, 16, LO, HI, method="uniform", fov_up=3.0, fov_down=-25.0)
    assert np.allclose(got, np.deg2rad(np.linspace(3.0, -25.0, 16)), rtol=0, atol=1e-15)
    # without a field of view: the 99.9 % and 0.1 % mass quantiles, bin centres within a bin of the outermost beams
    auto = estimate_beams(hist, 16, LO, HI, method="uniform")
    delta = (HI - LO) / 4096
    assert abs(auto[0] - np.deg2rad(3.0)) <= 2e-4 + delta and abs(auto[-1] - np.deg2rad(-25.0)) <= 2e-4 + delta
    assert np.allclose(np.diff(auto), (auto[-1] - auto[0]) / 15)
    # the datasheet's table, in any order, degrees
    table = tmp_path / "vlp16.txt"
    deg = [-15, 1, -13, 3, -11, 5, -9, 7, -7, 9, -5, 11, -3, 13, -1, 15]
    table.write_text("\n".join(str(d) for d in deg) + "\n")
    got = estimate_beams(hist, 16, LO, HI, method=str(table))
    assert np.allclose(got, np.deg2rad(sorted(deg, reverse=True)), rtol=0, atol=1e-15)
    shares = beam_shares(hist, R.uniform_beams(16), LO, HI)
    assert shares.shape == (16,) and np.allclose(shares, 1 / 16)


def test_the_three_value_errors(tmp_path):
    from dusty_gan_amd.datasets.beams import estimate_beams
    hist = np.zeros(1024, dtype=np.int64)
    hist[[100, 101, 500]] = [5, 7, 9]
    with pytest.raises(ValueError, match="populated bins"):
        estimate_beams(hist, 4, LO, HI)                         # 3 populated bins, 4 beams
    hist = np.zeros(1024, dtype=np.int64)
    hist[[100, 101, 500, 900]] = [1, 1, 10000, 1]
    with pytest.raises(ValueError, match="ended empty"):
        estimate_beams(hist, 4, LO, HI)                         # one bin holds every equal-mass quantile: three centres have none
    table = tmp_path / "twice.txt"
    table.write_text("1.0\n-1.0\n1.0\n")
    with pytest.raises(ValueError, match="monotonic"):
        estimate_beams(np.ones(64), 3, LO, HI, method=str(table))
    with pytest.raises(ValueError):
        estimate_beams(np.ones(64), 4, LO, HI, method=str(table))   # 3 lines for 4 beams
    with pytest.raises(ValueError):
        estimate_beams(np.ones(64), 3, LO, HI, method="no_such_method")


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_checks_pass_and_fail_under_each_defect():
    R.self_check()
    for defect in ("tie_upper", "ascending"):
        with pytest.raises(AssertionError):
            R.self_check(defect)


@pytest.mark.parametrize("name", list(R.GPU_CASES))
def test_no_gpu_case_has_a_point_near_a_discontinuity(name):
    beams, W, clouds = R.gpu_case(name)
    for pts in clouds:
        assert R.near_midpoint(pts, beams).size == 0 and R.near_column_edge(pts, W).size == 0
        _, cell = R.project(pts, beams, W)
        assert (cell >= 0).all() and len(np.unique(cell // W)) == len(beams)
    if name != "64x2048":
        assert any(len(np.unique(R.project(pts, beams, W)[1])) < len(pts) for pts in clouds)   # cells are contested
    else:
        assert 110_000 < len(clouds[0]) < 131_072


def test_no_histogram_case_has_a_point_near_a_bin_edge():
    for pts in R.hist_clouds():
        assert (~R.takes_part(pts)).sum() == (4 if len(pts) else 0)
        for NB in (64, 8192, 16384):
            assert R.near_bin_edge(pts, 1.0, 120.0, LO, HI, NB).size == 0
            assert R.near_bin_edge(pts, 1.0, 120.0, -0.4, 0.1, NB).size == 0
        if len(pts):   # both limits are strict: the points exactly on them are not counted, and some lie beyond either
            d = R.range64(pts)
            assert (d == 1.0).any() and (d == 120.0).any() and (d < 1.0).any() and (d > 120.0).any()
            assert R.histogram(pts, 1.0, 120.0, LO, HI, 64).sum() == ((d > 1.0) & (d < 120.0)).sum()


# ------------------------------------------------------------------------------------------------ dataset and command
def test_scan_folder_lists_files_per_split_from_the_config(tmp_path):
    from dusty_gan_amd.datasets import ScanFolder, define_dataset
    from dusty_gan_amd.utils.config import load_config
    made = {}
    for rec, n in (("drive_a", 3), ("drive_b", 2), ("08", 4), ("night", 1)):
        d = tmp_path / "sequences" / rec / "velodyne"
        d.mkdir(parents=True)
        made[rec] = []
        for i in reversed(range(n)):
            np.save(d / f"{i:04d}.npy", np.zeros((4, 8, 4), np.float32))
            made[rec].append(str(d / f"{i:04d}.npy"))
        (d / "notes.txt").write_text("not a scan")
    cfg = load_config(["dataset=scan_folder", f"dataset.root={tmp_path}", "dataset.shape=[4,8]",
                       'dataset.split={train: [drive_b, drive_a], val: ["08"], test: [night]}']).dataset
    assert cfg.name == "scan_folder" and cfg.resident is False and list(cfg.shape) == [4, 8]
    train = define_dataset(cfg, "train")
    assert isinstance(train, ScanFolder)
    assert train.datalist == sorted(made["drive_b"]) + sorted(made["drive_a"])     # the table's order, files sorted
    assert len(define_dataset(cfg, "val")) == 4 and len(define_dataset(cfg, "test")) == 1
    assert define_dataset(cfg, "val").datalist == sorted(made["08"])
    assert train.read(0).shape == (4, 8, 4)
    cfg.split = {"train": ["drive_a"]}
    assert len(define_dataset(cfg, "train")) == 3 and len(define_dataset(cfg, "val")) == 0   # a phase not named is empty
    default = load_config(["dataset=scan_folder"]).dataset
    assert set(default.split) == {"train", "val", "test"} and len(define_dataset(default, "train")) == 0
    cfg.name = "nuscenes"
    with pytest.raises(NotImplementedError):
        define_dataset(cfg, "train")


def test_process_clouds_arguments_and_plan(tmp_path):
    from dusty_gan_amd import process_clouds as P
    base = ["--in-dir", str(tmp_path / "in"), "--out-dir", str(tmp_path / "out")]
    a = P.parse_args(base + ["--rings", "32"])
    assert (a.rings, a.width, a.beams, a.min_depth, a.max_depth, a.chunk, a.num_workers) == (32, 2048, "kmeans", 0.9, 120.0, 16, 8)
    assert a.train is None and a.beam_range is None and a.beam_scans is None and not a.skip_existing
    a = P.parse_args(base + ["--rings", "16", "--width", "1024", "--beams", "uniform", "--fov-up", "15", "--fov-down", "-15",
                             "--beam-range", "5", "60", "--beam-scans", "100", "--train", "a", "b/", "--skip-existing"])
    assert (a.beams, a.fov_up, a.fov_down, a.beam_range, a.beam_scans, a.train) == ("uniform", 15.0, -15.0, [5.0, 60.0], 100,
                                                                                   ["a", "b/"])
    for bad in (["--rings", "0"], ["--rings", "257"], ["--rings", "32", "--width", "8193"], ["--rings", "32", "--chunk", "0"],
                ["--rings", "32", "--beams", str(tmp_path / "missing.txt")], ["--rings", "32", "--fov-up", "3"],
                ["--rings", "32", "--fov-up", "3", "--fov-down", "-25"], ["--rings", "32", "--beam-range", "60", "5"], []):
        with pytest.raises(SystemExit):
            P.parse_args(base + bad)
    for rel in ("in/b/x/0002.bin", "in/b/0001.npy", "in/a/0000.bin", "in/a/readme.txt"):
        os.makedirs(tmp_path / os.path.dirname(rel), exist_ok=True)
        (tmp_path / rel).write_bytes(b"")
    os.makedirs(tmp_path / "in" / "empty_dir")
    plan = P.plan(str(tmp_path / "in"), str(tmp_path / "out"))
    out = str(tmp_path / "out" / "sequences")
    assert plan == {"a": [(str(tmp_path / "in/a/0000.bin"), os.path.join(out, "a", "velodyne", "0000.npy"))],
                    "b": [(str(tmp_path / "in/b/0001.npy"), os.path.join(out, "b", "velodyne", "0001.npy")),
                          (str(tmp_path / "in/b/x/0002.bin"), os.path.join(out, "b", "velodyne", "0002.npy"))]}
    (tmp_path / "in/b/x/0001.bin").write_bytes(b"")
    with pytest.raises(ValueError, match="0001"):
        P.plan(str(tmp_path / "in"), str(tmp_path / "out"))
    assert P.evenly_spaced(list(range(10)), 2) == [2, 7] and P.evenly_spaced([1, 2], 5) == [1, 2]
