"""The label image's host side (dusty_gan_amd/datasets/labels.py) and the tests' own restatement (tests/label_util.py)
against what the reference's process_kitti.py wrote (tests/golden/label_image.npz).  No GPU."""
import os

import numpy as np
import pytest

from tests import label_util as LU
from tests import raw_scan_util as U


@pytest.fixture(scope="module")
def g():
    return LU.load()


@pytest.fixture(scope="module")
def raw():
    return U.load()


def _golden_lut(g):
    lut = np.full(65536, 255, dtype=np.uint8)
    lut[g["table/ids"]] = g["table/classes"]
    return lut


@pytest.mark.parametrize("name", LU.SCANS)
def test_restatement_reproduces_the_reference(g, raw, name):
    """label_util's far-to-near scatter, from the reference's recorded (row, column) grid, gives the PNG the reference wrote"""
    pts, W, winner, row, col = U.scan(raw, name)
    labels = g[f"scan/{name}/labels"]
    assert labels.dtype == np.uint32 and len(labels) == len(pts) and (labels >> 16).any()
    sem, inst = LU.label_images(row % LU.H, col, LU.depth32(pts), labels, _golden_lut(g), LU.H, W)
    assert np.array_equal(sem, g[f"scan/{name}/sem"])
    assert np.array_equal(LU.winner_image(row % LU.H, col, LU.depth32(pts), LU.H, W), winner)
    assert np.array_equal(inst[winner >= 0], (labels[winner[winner >= 0]] >> 16).astype(np.uint16)) and not inst[winner < 0].any()


def test_restatement_tie_rule():
    """two points of one cell at the same range: the lower index wins, wherever it stands"""
    row, col, depth = np.array([1, 1, 1]), np.array([2, 2, 2]), np.array([5.0, 3.0, 3.0], dtype=np.float32)
    assert LU.winner_image(row, col, depth, 4, 4)[1, 2] == 1
    assert LU.winner_image(row, col, depth[::-1].copy(), 4, 4)[1, 2] == 0


def test_table_is_the_references(g):
    from dusty_gan_amd.datasets import labels as LB
    lut = LB.SEMANTIC_KITTI_LUT
    assert lut.shape == (65536,) and lut.dtype == np.uint8
    ids, classes = g["table/ids"], g["table/classes"]
    assert len(ids) == 34 and sorted(set(classes.tolist())) == list(range(20))
    assert np.array_equal(lut[ids], classes)
    rest = np.ones(65536, dtype=bool)
    rest[ids] = False
    assert (lut[rest] == 255).all()
    assert len(LB.CLASS_NAMES) == 20 and len(set(LB.CLASS_NAMES)) == 20 and LB.CLASS_NAMES[0] == "unlabeled"
    assert LB.CLASS_NAMES[1] == "car" and LB.CLASS_NAMES[6] == "person" and LB.CLASS_NAMES[19] == "traffic-sign"


def test_palette_is_the_references(g):
    from dusty_gan_amd.datasets import labels as LB
    pal = LB.palette()
    assert pal.shape == (20, 3) and pal.dtype == np.uint8
    assert np.array_equal(pal.reshape(-1), g["palette"])


def test_png_round_trip(tmp_path, g):
    from dusty_gan_amd.datasets import labels as LB
    rng = np.random.default_rng(3)
    sem = rng.integers(0, 20, (5, 37)).astype(np.uint8)
    path = str(tmp_path / "a.png")
    LB.write_label_png(path, sem)
    assert os.listdir(tmp_path) == ["a.png"]
    back, pal = LB.read_label_png(path, return_palette=True)
    assert back.dtype == np.uint8 and np.array_equal(back, sem)
    assert np.array_equal(pal[:20].reshape(-1), g["palette"])
    assert np.array_equal(LB.read_label_png(path), sem)
    # and what the reference wrote reads back as it is
    from PIL import Image
    ref = g["scan/prefix_w256/sem"]
    img = Image.frombytes("P", (ref.shape[1], ref.shape[0]), ref.tobytes())
    img.putpalette(g["palette"].tolist())
    img.save(str(tmp_path / "ref.png"))
    assert np.array_equal(LB.read_label_png(str(tmp_path / "ref.png")), ref)


def test_label_file_length(tmp_path):
    from dusty_gan_amd.datasets import labels as LB
    from dusty_gan_amd.datasets.raw import RawScanError
    p = str(tmp_path / "x.label")
    np.arange(7, dtype=np.uint32).tofile(p)
    assert np.array_equal(LB.read_label_file(p, 7), np.arange(7, dtype=np.uint32))
    with pytest.raises(RawScanError, match="x.label"):
        LB.read_label_file(p, 8)


def test_process_kitti_plan_with_labels(tmp_path):
    from dusty_gan_amd import process_kitti as P
    root = str(tmp_path)
    for sub in ("velodyne", "labels"):
        os.makedirs(os.path.join(root, "dataset/sequences/00", sub))
    for k in range(3):
        open(os.path.join(root, "dataset/sequences/00/velodyne", f"{k:06d}.bin"), "wb").close()
    for k in (0, 2):
        open(os.path.join(root, "dataset/sequences/00/labels", f"{k:06d}.label"), "wb").close()
    pairs, lps = P.plan(root, labels=True)
    assert pairs == P.plan(root) and len(lps) == 3 and lps[1] is None
    assert lps[0] == (os.path.join(root, "dataset/sequences/00/labels/000000.label"),
                      os.path.join(root, "dusty-gan/sequences/00/labels/000000.png"))
    # --skip-existing: a scan whose .npy exists is planned for its missing PNG alone; with both present it is not planned
    os.makedirs(os.path.join(root, "dusty-gan/sequences/00/velodyne"))
    os.makedirs(os.path.join(root, "dusty-gan/sequences/00/labels"))
    for k in range(3):
        open(os.path.join(root, "dusty-gan/sequences/00/velodyne", f"{k:06d}.npy"), "wb").close()
    open(lps[2][1], "wb").close()
    pairs2, lps2 = P.plan(root, skip_existing=True, labels=True)
    assert pairs2 == [(pairs[0][0], None)] and lps2 == [lps[0]]
    assert P.parse_args(["--root-dir", root, "--labels"]).labels and not P.parse_args(["--root-dir", root]).labels
