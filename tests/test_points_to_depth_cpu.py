"""points_to_depth without a GPU: the numpy restatement (tests/points_to_depth_util.py) against what the reference's own
Coordinate.points_to_depth produced (tests/golden/points_to_depth.npz), the tie rule, the host logic of
datasets.raw.read_clouds and the reconstruct command's argument handling."""
import os

import numpy as np
import pytest

from tests import points_to_depth_util as PU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    return PU.load_golden()


def meta(g):
    return float(g["meta/min_depth"]), float(g["meta/max_depth"]), float(g["meta/tau"])


def test_fixture_is_what_the_tests_assume(g):
    assert g["grid"].shape == (2, 16, 64) and g["xyz"].shape == (2, 1500, 3) and g["xyz"].dtype == np.float32
    frac = g["weightless"].mean()
    assert 0.07 < frac < 0.13
    lit = g["f64/valid"].mean()
    assert 0.70 < lit < 0.82          # ~20 % of the pixels receive nothing, a few more only weightless points
    assert 1e-8 < float(g["e_ref"]) < 1e-6
    hits = np.bincount(g["f64/ids"][0][~g["weightless"][0]], minlength=1024)
    assert hits.max() >= 3 and (hits == 2).any()   # pixels with several points


def test_restatement_reproduces_the_reference(g):
    lo, hi, tau = meta(g)
    depth, valid, ids = PU.points_to_depth(g["xyz"], g["grid"], lo, hi, tau)
    part = ~g["weightless"]
    assert np.array_equal(ids[part], g["f64/ids"][part]) and (ids[~part] == -1).all()
    assert np.array_equal(valid, g["f64/valid"])
    worst = float(np.abs(depth - g["f64/depth"]).max())
    print(f"restatement vs reference (float64): {worst:.3e}")
    assert worst <= 1e-12
    assert (depth[~valid] == 1.0).all()
    # the nominal grid is separable, and the split search finds the same pixels
    assert PU.separable(g["grid"])
    d2, v2, i2 = PU.points_to_depth(g["xyz"], g["grid"], lo, hi, tau, split=True)
    assert np.array_equal(i2, ids) and np.array_equal(v2, valid) and np.array_equal(d2, depth)
    # float32 arithmetic decides the same (the asserted margin) and stays within a few e_ref
    d32, v32, i32 = PU.points_to_depth(g["xyz"], g["grid"], lo, hi, tau, dtype=np.float32)
    assert np.array_equal(i32, ids) and np.array_equal(v32, valid)
    assert float(np.abs(d32 - depth).max()) <= 4 * float(g["e_ref"])


def test_a_tie_goes_to_the_lower_index(g):
    lo, hi, tau = meta(g)
    tie = g["tie/grid"]
    assert np.array_equal(tie[:, 5], tie[:, 4]) and not np.array_equal(tie[:, 6], tie[:, 4])
    depth, valid, ids = PU.points_to_depth(g["tie/xyz"], tie, lo, hi, tau)
    assert np.array_equal(ids, g["tie/ids"]) and ((ids // 64) == 4).all()
    assert np.array_equal(valid, g["tie/valid"]) and not valid[0, 5].any()
    assert float(np.abs(depth - g["tie/depth"]).max()) <= 1e-12


def test_counts_and_weightless_points():
    grid = PU.load_golden()["grid"]
    u, v = float(grid[0, 3, 7]), float(grid[1, 3, 7])
    ray = np.array([np.cos(u) * np.cos(v), np.cos(u) * np.sin(v), np.sin(u)])
    pts = np.stack([ray * 0.5, ray * 0.25, ray * 0.0, ray * 1.5, ray * (0.9 / 120.0) * 0.5, [np.nan, 0.1, 0.1]])[None]
    depth, valid, ids = PU.points_to_depth(pts, grid, 0.9, 120.0, 2.0)
    assert ids.tolist() == [[3 * 64 + 7, 3 * 64 + 7, -1, -1, -1, -1]] and valid.sum() == 1
    w = np.exp(-2.0 * np.array([0.5, 0.25]))
    want = ((w * np.array([60.0, 30.0])).sum() / (w.sum() + 1e-8) - 0.9) / 119.1
    assert abs(depth[0, 3, 7] - want) < 1e-14
    depth, valid, ids = PU.points_to_depth(pts, grid, 0.9, 120.0, 2.0, counts=[1])
    want = (w[0] * 60.0 / (w[0] + 1e-8) - 0.9) / 119.1     # (the 1e-8 of the denominator is part of the value)
    assert ids.tolist() == [[3 * 64 + 7, -1, -1, -1, -1, -1]] and abs(depth[0, 3, 7] - want) < 1e-14
    depth, valid, ids = PU.points_to_depth(pts, grid, 0.9, 120.0, 2.0, counts=[0], drop_value=0.0)
    assert not valid.any() and (depth == 0.0).all()


# ------------------------------------------------------------------------------------------------ read_clouds
def test_read_clouds_pads_and_counts(tmp_path):
    from dusty_gan_amd.datasets.raw import read_clouds
    rng = np.random.default_rng(0)
    a = rng.normal(size=(7, 4)).astype(np.float32) * 30
    b = rng.normal(size=(12, 3)).astype(np.float32) * 30
    c = rng.normal(size=(5, 4)) * 30                      # float64 .npy: converted
    a.tofile(tmp_path / "a.bin")
    np.save(tmp_path / "b.npy", b)
    np.save(tmp_path / "c.npy", c)
    np.save(tmp_path / "d.npy", a)                        # float32 N x 4 .npy: the straight read
    rec, counts = read_clouds([tmp_path / "a.bin", tmp_path / "b.npy", tmp_path / "c.npy", tmp_path / "d.npy"], 120.0, "cpu")
    assert rec.shape == (4, 12, 4) and rec.dtype.is_floating_point and rec.element_size() == 4
    assert counts.tolist() == [7, 12, 5, 7] and str(counts.dtype) == "torch.int32"
    rec = rec.numpy()
    assert np.array_equal(rec[0, :7, :3], a[:, :3] / np.float32(120.0)) and np.array_equal(rec[0, :7, 3], a[:, 3])
    assert np.array_equal(rec[1, :, :3], b / np.float32(120.0)) and (rec[1, :, 3] == 0).all()
    assert np.array_equal(rec[2, :5, :3], c.astype(np.float32)[:, :3] / np.float32(120.0))
    assert np.array_equal(rec[3], rec[0])
    assert (rec[0, 7:] == 0).all() and (rec[2, 5:] == 0).all()   # the padding


def test_read_clouds_refuses_bad_files(tmp_path):
    from dusty_gan_amd.datasets.raw import RawScanError, read_clouds
    good = tmp_path / "good.bin"
    np.ones((3, 4), np.float32).tofile(good)
    (tmp_path / "empty.bin").write_bytes(b"")
    (tmp_path / "odd.bin").write_bytes(b"\0" * 40)
    np.save(tmp_path / "empty.npy", np.zeros((0, 4), np.float32))
    np.save(tmp_path / "wide.npy", np.zeros((3, 5), np.float32))
    np.save(tmp_path / "flat.npy", np.zeros(12, np.float32))
    (tmp_path / "junk.npy").write_bytes(b"not a numpy file")
    for name in ("empty.bin", "odd.bin", "empty.npy", "wide.npy", "flat.npy", "junk.npy"):
        with pytest.raises(RawScanError) as e:
            read_clouds([good, tmp_path / name], 120.0, "cpu")
        assert name in str(e.value) and e.value.names == [str(tmp_path / name)]
    with pytest.raises(FileNotFoundError):
        read_clouds([], 120.0, "cpu")
    # the earlier meaning of the exception is unchanged
    assert "ring starts" in str(RawScanError(["x"]))


# ------------------------------------------------------------------------------------------------ the command's arguments
def test_reconstruct_expands_directories_in_sorted_order(tmp_path):
    from dusty_gan_amd.reconstruct import expand_paths, parse_args
    d = tmp_path / "clouds"
    d.mkdir()
    for name in ("b.bin", "a.npy", "c.bin", "notes.txt"):
        (d / name).write_bytes(b"")
    single = tmp_path / "z.bin"
    single.write_bytes(b"")
    got = expand_paths([single, d])
    assert got == [("z", str(single)), ("a", str(d / "a.npy")), ("b", str(d / "b.bin")), ("c", str(d / "c.bin"))]
    args = parse_args(["--model-path", "m.pth", "--config-path", "c.yaml", "--points", str(d), str(single)])
    assert [s for s, _ in args.clouds] == ["a", "b", "c", "z"]
    assert args.batch_size == 32 and args.tau == 2 and args.distance == "l1" and args.num_step == 1000 and args.tol == 0
    assert not args.no_images and not args.no_bins and args.corruption is None and args.num_code == 1


def test_reconstruct_refuses_duplicate_stems_and_bad_arguments(tmp_path, capsys):
    from dusty_gan_amd.reconstruct import expand_paths, parse_args
    d = tmp_path / "clouds"
    d.mkdir()
    (d / "scan.bin").write_bytes(b"")
    (d / "scan.npy").write_bytes(b"")
    with pytest.raises(ValueError, match="two clouds named 'scan'"):
        expand_paths([d])
    with pytest.raises(ValueError, match="no such file"):
        expand_paths([tmp_path / "missing.bin"])
    empty = tmp_path / "none"
    empty.mkdir()
    with pytest.raises(ValueError, match="no \\*.bin or \\*.npy"):
        expand_paths([empty])
    base = ["--model-path", "m.pth", "--config-path", "c.yaml"]
    (tmp_path / "one.bin").write_bytes(b"")
    one = str(tmp_path / "one.bin")
    for bad in (base + ["--points", str(d)], base, base + ["--points", one, "--tau", "-1"], base + ["--points", one, "--tau", "17"],
                base + ["--points", one, "--num-code", "4"], base + ["--points", one, "--distance", "l3"]):
        with pytest.raises(SystemExit):
            parse_args(bad)
    capsys.readouterr()
    # the inversion flags are evaluate_reconstruction's own
    from dusty_gan_amd import evaluate_reconstruction as ER
    a, b = parse_args(base + ["--points", one, "--corruption", "low resolution", "--distance", "l1+chamfer"]), \
        ER.parse_args(base + ["--corruption", "low resolution", "--distance", "l1+chamfer"])
    for k, v in vars(b).items():
        assert k == "batch_size" or getattr(a, k) == v, k


def test_header_and_binding_declare_the_entry_point():
    from dusty_gan_amd import _lib
    h = open(os.path.join(ROOT, "include", "dusty_gan_hip.h")).read()
    assert "int dg_points_to_depth(" in h and len(_lib.PROTOTYPES["dg_points_to_depth"]) == 18
    sig = h[h.index("int dg_points_to_depth("):]
    assert sig[:sig.index(";")].count(",") == 17
