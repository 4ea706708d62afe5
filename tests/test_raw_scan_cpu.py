"""Raw-scan projection, the parts that need no GPU: the fixture's own conditions (tests/golden/raw_scan.npz, made by
tests/golden/make_raw_scan_golden.py from the reference's process_kitti.py), the `.bin` -> `.npy` path plan and the command
line of `python -m dusty_gan_amd.process_kitti`."""
import os

import numpy as np
import pytest

from tests import raw_scan_util as U


def test_fixture_cases():
    """the cases the projection tests rest on are all in the fixture"""
    g = U.load()
    names = U.scan_names(g)
    by = {n: U.scan(g, n) for n in names}
    pts, W, winner, row, col = by["ring64_w2048"]
    assert W == 2048 and row.min() == 0 and row.max() == 63 and len(np.unique(row)) == 64
    assert {by[n][1] for n in names} >= {256, 512, 2048}
    assert any(len(by[n][0]) % 64 for n in names)
    # points in front of the first ring start: row 0, and the ring that follows them is row 0 too (64 starts)
    pts, W, winner, row, col = by["prefix_w256"]
    q = lambda p: np.where(p[:, 0] >= 0, np.where(p[:, 1] >= 0, 0, 3), np.where(p[:, 1] >= 0, 1, 2))
    quad = q(pts)
    starts = np.flatnonzero((np.roll(quad, 1) == 3) & (quad == 0))
    assert len(starts) == 64 and starts[0] > 0 and (row[:starts[0]] == 0).all() and row[starts[0]] == 0
    # fewer than 64 rings: the top rows stay empty
    pts, W, winner, row, col = by["rings50_w512"]
    assert row.min() == 14 and (winner[:14] < 0).all()
    # 65-70 rings: negative rows, which numpy wraps
    pts, W, winner, row, col = by["rings67_w256"]
    assert row.min() == -3 and row.max() == 63
    first = np.flatnonzero(row < 0)
    assert (winner[61:] >= 0).any() and set(np.unique(row[first] % U.H)) == {61, 62, 63}
    ang = [str(n) for n in g["meta/angle_scans"]]
    assert len(ang) >= 16 and set(ang) <= set(names)
    never = g["angles/never"]
    assert 0 < never.sum() and not never.all(0).any() and not never.all(1).any()
    assert g["angles/ref"].shape == (2, 64, 64) and not np.isnan(g["angles/ref"]).any()
    assert 0 < float(g["angles/e_ref"]) < 1e-5
    assert os.path.getsize(U.GOLDEN) < 1 << 20


def test_fixture_excluded_set_cap():
    """the cap of the GPU parity test, from the fixture alone: per scan the excluded set is at most 1 % of the non-empty
    cells, and no point ties in depth with the winner of its cell"""
    g = U.load()
    for name in U.scan_names(g):
        pts, W, winner, row, col = U.scan(g, name)
        n_ex, filled = U.check_cap(pts, W, winner, row, col)
        assert filled > 0 and n_ex <= U.EXCLUDED_CAP * filled, name
        # the recorded winners are each cell's nearest point (the reference writes far-to-near, later writes win)
        d = U.depth32(pts)
        best = np.full(winner.shape, np.inf, dtype=np.float32)
        np.minimum.at(best, (row % U.H, col), d)
        assert np.array_equal(best[winner >= 0], d[winner[winner >= 0]]), name
        assert np.isinf(best[winner < 0]).all(), name


def test_fixture_angles_within_their_own_error():
    g = U.load()
    e_ref = float(g["angles/e_ref"])
    assert np.abs(g["angles/ref"].astype(np.float64) - g["angles/f64"]).max() == e_ref


def _touch(path, data=b""):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)


def test_path_plan(tmp_path):
    from dusty_gan_amd import process_kitti as P
    root = str(tmp_path)
    for seq, names in (("01", ["000001", "000000"]), ("00", ["000003"]), ("08", ["000000"])):
        for n in names:
            _touch(os.path.join(root, "dataset/sequences", seq, "velodyne", n + ".bin"))
    _touch(os.path.join(root, "dataset/sequences/00/velodyne/notes.txt"))
    _touch(os.path.join(root, "dataset/sequences/00/calib.txt"))
    pairs = P.plan(root)
    rel = [(os.path.relpath(a, root), os.path.relpath(b, root)) for a, b in pairs]
    assert rel == [("dataset/sequences/00/velodyne/000003.bin", "dusty-gan/sequences/00/velodyne/000003.npy"),
                   ("dataset/sequences/01/velodyne/000000.bin", "dusty-gan/sequences/01/velodyne/000000.npy"),
                   ("dataset/sequences/01/velodyne/000001.bin", "dusty-gan/sequences/01/velodyne/000001.npy"),
                   ("dataset/sequences/08/velodyne/000000.bin", "dusty-gan/sequences/08/velodyne/000000.npy")]
    assert [os.path.relpath(a, root) for a, _ in P.plan(root, sequences=["8", "00"])] == [
        "dataset/sequences/00/velodyne/000003.bin", "dataset/sequences/08/velodyne/000000.bin"]
    with pytest.raises(FileNotFoundError, match="05"):
        P.plan(root, sequences=["05"])
    _touch(pairs[1][1])
    assert P.plan(root, skip_existing=True) == [pairs[0], pairs[2], pairs[3]]


def test_argument_parsing():
    from dusty_gan_amd import process_kitti as P
    a = P.parse_args(["--root-dir", "/data/kitti"])   # the reference's only flag
    assert a.root_dir == "/data/kitti" and a.sequences is None and not a.skip_existing and not a.angles_only
    assert a.chunk >= 1 and a.num_workers >= 1
    a = P.parse_args(["--root-dir", "r", "--sequences", "00", "3", "--chunk", "5", "--num-workers", "2", "--skip-existing",
                      "--angles-only"])
    assert (a.sequences, a.chunk, a.num_workers, a.skip_existing, a.angles_only) == (["00", "3"], 5, 2, True, True)
    for bad in ([], ["--root-dir", "r", "--chunk", "0"], ["--root-dir", "r", "--num-workers", "0"]):
        with pytest.raises(SystemExit):
            P.parse_args(bad)


def test_empty_root_is_an_error(tmp_path):
    from dusty_gan_amd import process_kitti as P
    with pytest.raises(FileNotFoundError, match="no raw scans"):
        P.main(["--root-dir", str(tmp_path)])
    os.makedirs(tmp_path / "dataset/sequences/00/velodyne")
    with pytest.raises(FileNotFoundError, match="no raw scans"):
        P.main(["--root-dir", str(tmp_path)])
    assert not os.path.exists(tmp_path / "angles.pt") and not os.path.exists(tmp_path / "dusty-gan")


def test_offsets_are_checked():
    from dusty_gan_amd.datasets import raw
    with pytest.raises(ValueError):
        raw._check_offsets([0, 5, 3, 10], 10)
    with pytest.raises(ValueError):
        raw._check_offsets([0, 5], 10)
    with pytest.raises(ValueError):
        raw._check_offsets([1, 10], 10)
    assert raw._check_offsets([0, 0, 4, 10], 10).tolist() == [0, 0, 4, 10]


def test_npy_writer_matches_numpy(tmp_path):
    """write_npy's file is np.save's: v1.0, C order, float32 - what ScanLoader's fast path reads"""
    from dusty_gan_amd.datasets import raw
    arr = np.random.default_rng(0).random((64, 32, 4)).astype(np.float32)
    a, b = str(tmp_path / "a.npy"), str(tmp_path / "b.npy")
    raw.write_npy(a, arr)
    np.save(b, arr)
    assert open(a, "rb").read() == open(b, "rb").read()
    assert not os.path.exists(a + ".part")
