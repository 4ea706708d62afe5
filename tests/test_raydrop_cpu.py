"""The ray-drop transfer without a GPU: the NumPy restatements of its three kernels (tests/raydrop_util.py) on hand-made
cases against literal expected arrays, the command's argument checks, and the .label round trip."""
import numpy as np
import pytest

from tests import raydrop_util as R


def cloud(*points):
    return np.asarray(points, dtype=np.float32)[None]


# ---- winner -------------------------------------------------------------------------------------------------------------------------
def test_winner_nearest_of_two_points_in_one_pixel():
    rec = cloud([0.5, 0, 0], [0.25, 0, 0], [0, 0.75, 0])
    idx = np.array([[2, 2, 0]])
    assert R.winner(rec, idx, None, 4).tolist() == [[2, -1, 1, -1]]


def test_winner_exact_tie_takes_the_lowest_index():
    rec = cloud([0, 0.5, 0], [0.25, 0, 0], [0, 0, 0.25], [0.25, 0, 0], [0.5, 0, 0])   # points 1, 2, 3 at range 0.25
    idx = np.array([[1, 1, 1, 1, 1]])
    assert R.winner(rec, idx, None, 2).tolist() == [[-1, 1]]
    assert R.winner(rec[:, ::-1], idx, None, 2).tolist() == [[-1, 1]]   # reversed: 3, 2, 1 hold the tie, index 1 again


def test_winner_tie_after_rounding_to_float32():
    """two ranges that differ in double and round to the same float32: still a tie, the lower index wins"""
    a, b = np.float32(0.5), np.nextafter(np.float32(0.5), np.float32(1))
    rec = cloud([b, 2.0 ** -30, 0], [b, 0, 0], [a, 0, 0])
    assert R.ranges(rec)[0].tolist() == [float(b), float(b), 0.5]
    assert R.winner(rec[:, :2], np.array([[0, 0]]), None, 1).tolist() == [[0]]
    assert R.winner(rec, np.array([[0, 0, 0]]), None, 1).tolist() == [[2]]


def test_winner_empty_pixel_idle_point_and_truncated_cloud():
    rec = cloud([0.5, 0, 0], [0.125, 0, 0], [0.25, 0, 0], [0.0625, 0, 0])
    idx = np.array([[0, -1, 3, 0]])
    assert R.winner(rec, idx, None, 4).tolist() == [[3, -1, -1, 2]]            # point 1 took no part; pixels 1, 2 are empty
    assert R.winner(rec, idx, np.array([3]), 4).tolist() == [[0, -1, -1, 2]]   # counts = 3: point 3 is not read
    assert R.winner(rec, idx, np.array([0]), 4).tolist() == [[-1, -1, -1, -1]]


# ---- keep ---------------------------------------------------------------------------------------------------------------------------
def test_keep_two_realisations_with_different_masks():
    conf = np.array([[[[1.0, -1.0, 0.5, 2.0]]]], dtype=np.float32)               # [1,1,1,4]
    win = np.array([[0, 1, -1, 2]])
    noise = np.array([[[[[0.0, 2.0, 0.0, -3.0]]], [[[-2.0, 0.0, 0.0, 0.0]]]]], dtype=np.float32)   # [1,2,1,1,4]
    assert R.keep(conf, win, noise).tolist() == [[[[1, 1, 0, 0]], [[0, 0, 0, 1]]]]


def test_keep_image_logit_sign_and_a_scan_dropped_whole():
    conf = np.array([[[[1.0, 1.0, 1.0]], [[0.5, -0.5, 0.0]]],                    # scan 0: h2 = 0 is NOT kept (strict)
                     [[[1.0, 1.0, 1.0]], [[-1.0, -1.0, -1.0]]]], dtype=np.float32)
    win = np.array([[0, 1, 2], [0, 1, 2]])
    noise = np.zeros((2, 1, 1, 1, 3), dtype=np.float32)
    got = R.keep(conf, win, noise)
    assert got.tolist() == [[[[1, 0, 0]]], [[[0, 0, 0]]]]
    out = R.gather(np.zeros((2, 3, 3), np.float32), win, got)
    assert len(out[1, 0][0]) == 0 and out[1, 0][2].tolist() == []                # count 0
    assert out[0, 0][2].tolist() == [0]


# ---- gather -------------------------------------------------------------------------------------------------------------------------
def test_gather_row_major_with_labels_and_payload():
    rec = np.array([[[1, 2, 3, 10], [4, 5, 6, 11], [7, 8, 9, 12]]], dtype=np.float32)
    lab = np.array([[2 ** 32 - 1, 40, 0x00050007]], dtype=np.int64)
    win = np.array([[2, -1, 0, 1]])
    keep = np.array([[[[1, 1], [0, 1]], [[1, 0], [1, 0]]]], dtype=np.uint8)      # [1,2,2,2]; pixel 1 kept but empty
    out = R.gather(rec, win, keep, lab)
    assert out[0, 0][0].tolist() == [[7, 8, 9, 12], [4, 5, 6, 11]] and out[0, 0][2].tolist() == [2, 1]
    assert out[0, 0][1].tolist() == [0x00050007, 40] and out[0, 0][1].dtype == np.uint32
    assert out[0, 1][0].tolist() == [[7, 8, 9, 12], [1, 2, 3, 10]] and out[0, 1][1].tolist() == [0x00050007, 2 ** 32 - 1]
    out3 = R.gather(rec[:, :, :3].copy(), win, keep)
    assert out3[0, 1][0].tolist() == [[7, 8, 9, 0], [1, 2, 3, 0]] and out3[0, 1][1] is None


def test_gather_copies_bits():
    rec = np.zeros((1, 2, 4), dtype=np.float32)
    rec.view(np.int32)[0, 1] = [0x7FC01234, -2 ** 31, 1, 0x7F800001]             # NaN payloads, -0.0, a denormal
    out = R.gather(rec, np.array([[1]]), np.ones((1, 1, 1, 1), np.uint8))
    assert R.bits(out[0, 0][0]).tolist() == [[0x7FC01234, -2 ** 31, 1, 0x7F800001]]


def test_quantised_ranges_are_exact_in_double():
    """raydrop_util's argument: on the lattice x x + y y + z z is exact, so a fused multiply-add changes nothing"""
    from fractions import Fraction
    rng = np.random.default_rng(0)
    q = R.quantise(rng.uniform(-1, 1, (2000, 3)))
    assert np.array_equal(q * np.float32(R.LATTICE), np.round(q * np.float32(R.LATTICE)))
    x = q.astype(np.float64)
    s = (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]
    for row, got in zip(q[:200], s[:200]):
        assert sum(Fraction(float(v)) ** 2 for v in row) == Fraction(float(got))


# ---- the command's arguments ----------------------------------------------------------------------------------------------------------
@pytest.fixture()
def files(tmp_path):
    from dusty_gan_amd.utils.config import dump_config, load_config
    cfgs = {}
    for name, model in (("dusty1", "dusty1_dcgan_eqlr"), ("none", "dcgan_eqlr")):
        cfgs[name] = str(tmp_path / f"{name}.yaml")
        dump_config(load_config([f"model={model}", "dataset=synthetic", "dataset.shape=[64,1024]"]), cfgs[name])
    clouds, labels = tmp_path / "clouds", tmp_path / "labels"
    clouds.mkdir()
    labels.mkdir()
    rng = np.random.default_rng(1)
    for stem, n in (("a", 7), ("b", 5)):
        rng.normal(size=(n, 4)).astype(np.float32).tofile(clouds / f"{stem}.bin")
        np.arange(n, dtype="<u4").tofile(labels / f"{stem}.label")
    base = ["--model-path", str(tmp_path / "g.pth"), "--points", str(clouds)]
    return {"cfg": cfgs, "clouds": clouds, "labels": labels, "base": base}


def refused(argv, capsys):
    from dusty_gan_amd.transfer_raydrop import parse_args
    with pytest.raises(SystemExit) as e:
        parse_args(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_arguments_accepted(files):
    from dusty_gan_amd.transfer_raydrop import parse_args
    args = parse_args(files["base"] + ["--config-path", files["cfg"]["dusty1"], "--labels", str(files["labels"]), "--realisations", "3",
                                       "--corruption", "closing"])
    assert [s for s, _ in args.clouds] == ["a", "b"] and args.rows == [7, 5]
    assert (args.realisations, args.drop_noise, args.seed, args.corruption, args.no_maps) == (3, "sample", 0, "closing", False)


def test_missing_label_file_is_named(files, capsys):
    (files["labels"] / "b.label").unlink()
    err = refused(files["base"] + ["--config-path", files["cfg"]["dusty1"], "--labels", str(files["labels"])], capsys)
    assert str(files["labels"] / "b.label") in err


def test_label_count_mismatch_is_named(files, capsys):
    np.arange(6, dtype="<u4").tofile(files["labels"] / "b.label")
    err = refused(files["base"] + ["--config-path", files["cfg"]["dusty1"], "--labels", str(files["labels"])], capsys)
    assert str(files["labels"] / "b.label") in err and "6 labels" in err and "5 records" in err


def test_fixed_noise_is_one_realisation(files, capsys):
    err = refused(files["base"] + ["--config-path", files["cfg"]["dusty1"], "--drop-noise", "fixed", "--realisations", "2"], capsys)
    assert "--drop-noise fixed" in err


def test_baseline_config_is_refused(files, capsys):
    err = refused(files["base"] + ["--config-path", files["cfg"]["none"]], capsys)
    assert "no measurability head" in err and "nothing to transfer" in err


def test_read_clouds_returns_the_files_records_on_request(tmp_path):
    """return_raw: the records in metres as the files hold them, bit for bit, padded like the unit-space records; the default
    result is the pair it was"""
    from dusty_gan_amd.datasets.raw import read_clouds
    rng = np.random.default_rng(3)
    a = (rng.normal(size=(6, 4)) * 30).astype(np.float32)
    a.view(np.int32)[2, 3] = 0x7FC01234                                         # a payload that arithmetic would not keep
    b = (rng.normal(size=(4, 3)) * 30).astype(np.float32)
    a.tofile(tmp_path / "a.bin")
    np.save(tmp_path / "b.npy", b)
    paths = [tmp_path / "a.bin", tmp_path / "b.npy"]
    pair = read_clouds(paths, 120.0, "cpu")
    rec, counts, raw = read_clouds(paths, 120.0, "cpu", return_raw=True)
    assert len(pair) == 2 and np.array_equal(R.bits(pair[0].numpy()), R.bits(rec.numpy())) and counts.tolist() == [6, 4]
    assert tuple(raw.shape) == (2, 6, 4) and np.array_equal(R.bits(raw[0].numpy()), R.bits(a))
    assert np.array_equal(R.bits(raw[1, :4, :3].numpy()), R.bits(b)) and not raw[1, :, 3].any() and not raw[1, 4:].any()
    assert np.array_equal(rec[0, :, :3].numpy(), a[:, :3] / np.float32(120.0))


def test_label_round_trip(tmp_path):
    from dusty_gan_amd.transfer_raydrop import read_labels, write_labels
    lab = np.array([0, 1, 0x00050007, 2 ** 32 - 1, 40], dtype=np.uint32)
    path = str(tmp_path / "x.label")
    write_labels(path, lab)
    assert (tmp_path / "x.label").read_bytes() == lab.astype("<u4").tobytes()
    got = read_labels(path, 5)
    assert got.dtype == np.dtype("<u4") and np.array_equal(got, lab)
    with pytest.raises(ValueError, match="x.label"):
        read_labels(path, 4)
