"""python -m dusty_gan_amd.remove_objects: its arguments, and the tests' restatement of the removal mask on a case written out
by hand.  No GPU."""
import numpy as np
import pytest

from tests import label_util as LU

BASE = ["--model-path", "g.pth", "--config-path", "g.yaml"]


def test_classes_by_name_and_number():
    from dusty_gan_amd.remove_objects import DEFAULT_REMOVE, parse_args
    args = parse_args(BASE + ["--split", "test", "--remove", "car", "6", "traffic-sign", "1"])
    assert args.remove_classes == [1, 6, 19]
    default = parse_args(BASE + ["--split", "val", "--num-scans", "4"])
    assert default.remove_classes == [1, 2, 3, 4, 5, 6, 7, 8] and len(DEFAULT_REMOVE) == 8
    assert default.dilate == 1 and default.fill_label == 0 and default.batch_size == 32 and default.tau == 2


@pytest.mark.parametrize("argv, message", [
    (["--split", "test", "--remove", "wagon"], "not a class"),
    (["--split", "test", "--remove", "20"], "not a class"),
    (["--points", "clouds"], "--points needs --labels"),
    (["--split", "test", "--dilate", "9"], "--dilate"),
    (["--split", "test", "--dilate", "-1"], "--dilate"),
    (["--split", "test", "--labels", "dir"], "--labels goes with --points"),
    ([], "one of --points and --split"),
    (["--split", "test", "--corruption", "dropout"], "takes the place of a corruption"),
    (["--split", "test", "--fill-label", "20"], "--fill-label"),
    (["--points", "clouds", "--labels", "dir", "--num-scans", "2"], "--num-scans"),
])
def test_refused_arguments(argv, message, capsys):
    from dusty_gan_amd.remove_objects import parse_args
    with pytest.raises(SystemExit) as e:
        parse_args(BASE + argv)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_missing_label_file_is_named(tmp_path, capsys):
    from dusty_gan_amd.remove_objects import parse_args
    (tmp_path / "clouds").mkdir()
    (tmp_path / "labels").mkdir()
    for stem in ("a", "b"):
        np.zeros((3, 4), np.float32).tofile(tmp_path / "clouds" / f"{stem}.bin")
    np.zeros(3, np.uint32).tofile(tmp_path / "labels" / "a.label")
    with pytest.raises(SystemExit):
        parse_args(BASE + ["--points", str(tmp_path / "clouds"), "--labels", str(tmp_path / "labels")])
    assert "b.label" in capsys.readouterr().err
    np.zeros(3, np.uint32).tofile(tmp_path / "labels" / "b.label")
    args = parse_args(BASE + ["--points", str(tmp_path / "clouds"), "--labels", str(tmp_path / "labels")])
    assert [s for s, _ in args.clouds] == ["a", "b"]


def test_label_png_path():
    from dusty_gan_amd.remove_objects import label_png_of
    assert label_png_of("/d/dusty-gan/sequences/08/velodyne/000123.npy") == "/d/dusty-gan/sequences/08/labels/000123.png"
    with pytest.raises(FileNotFoundError, match="velodyne"):
        label_png_of("/d/scans/000123.npy")


def test_remove_mask_by_hand():
    """4 x 8, r = 1, class 1 removed.  Flagged: (0, 0) - row 0, column 0 - and (2, 7) - column 7: each grows over the seam.
    (3, 3) is a car that was not measured, (1, 4) a measured pixel of another class: neither is flagged"""
    sem = np.zeros((1, 4, 8), dtype=np.uint8)
    valid = np.zeros((1, 4, 8), dtype=np.float32)
    sem[0, 0, 0], valid[0, 0, 0] = 1, 1
    sem[0, 2, 7], valid[0, 2, 7] = 1, 1
    sem[0, 3, 3], valid[0, 3, 3] = 1, 0
    sem[0, 1, 4], valid[0, 1, 4] = 9, 1
    table = np.zeros(256, dtype=np.uint8)
    table[1] = 1
    want = np.array([[1, 1, 0, 0, 0, 0, 0, 1],     # (0, 0): rows 0..1 (no row -1), columns 7, 0, 1
                     [1, 1, 0, 0, 0, 0, 1, 1],     # both: (0, 0)'s row 1 and (2, 7)'s row 1 (columns 6, 7, 0)
                     [1, 0, 0, 0, 0, 0, 1, 1],     # (2, 7): columns 6, 7 and, across the seam, 0
                     [1, 0, 0, 0, 0, 0, 1, 1]], dtype=np.uint8)
    remove, counts = LU.remove_mask(sem, valid, table, 1)
    assert np.array_equal(remove[0], want)
    assert counts.shape == (1, 256) and counts[0, 1] == 2 and counts[0, 9] == 1 and counts[0, 0] == 0 and counts.sum() == 3
    r0, _ = LU.remove_mask(sem, valid, table, 0)
    assert r0.sum() == 2 and r0[0, 0, 0] == 1 and r0[0, 2, 7] == 1


def test_compose_and_cloud_remove_restatements():
    tgt = np.array([[[0.5, 0.25, 0.75, 0.1]]], dtype=np.float32)
    gen = np.array([[[0.4, 0.5, 0.6, 0.7]]], dtype=np.float32)
    valid = np.array([[[1, 1, 0, 0]]], dtype=np.float32)
    remove = np.array([[[0, 1, 1, 0]]], dtype=np.uint8)
    keep = np.array([[[1, 1, 0, 1]]], dtype=np.float32)
    sem = np.array([[[13, 1, 1, 9]]], dtype=np.uint8)
    inv, source, sem_out, counts = LU.compose(tgt, valid, gen, keep, False, 0.0, remove, sem, 4)
    assert inv.tolist() == [[[0.5, 0.5, 0.0, 0.0]]] and source.tolist() == [[[1, 2, 0, 0]]] and sem_out.tolist() == [[[13, 4, 0, 0]]]
    assert counts.tolist() == [[1, 1, 1]]                       # pixel 1: removed, filled, and nearer than the car (0.5 > 0.25)
    rec = np.arange(24, dtype=np.float32).reshape(1, 6, 4)
    idx = np.array([[0, 1, -1, 2, 1, 3]], dtype=np.int32)
    (words, labels, index), = LU.cloud_remove(rec, [5], idx, remove.reshape(1, 1, 4), np.arange(6)[None] + 100)
    assert index.tolist() == [0, 2] and labels.tolist() == [100, 102] and np.array_equal(words.view(np.float32), rec[0, [0, 2]])
