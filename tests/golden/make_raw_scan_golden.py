"""Generate tests/golden/raw_scan.npz from the REFERENCE's own process_kitti.py.

Runs only where the reference's sources are at hand (DUSTY_REFERENCE, default /root/reference):
    python tests/golden/make_raw_scan_golden.py
process_kitti.py is loaded by path.  Its imports that the two functions taken from it never use - numba (`jit` = identity:
`scatter` then runs as the plain Python loop it is), joblib, matplotlib (`cm.turbo` is called once at import, for the label
palette), tqdm (identity) - are empty stand-ins; `datasets.kitti` is the reference's own file, loaded with a torchvision
placeholder the way make_golden.py does, because KITTIOdometry.preprocess builds the batches for compute_avg_angles.
`process_point_clouds` and `compute_avg_angles` are called unmodified; the module's `projection` is wrapped only to RECORD the
(row, column) grid and the far-to-near order it is handed, from which the winner of every cell follows.

Seeded synthetic raw scans (rings swept counter-clockwise from quadrant 0, like a Velodyne's; coordinates on a 1/256 m
lattice so the file compresses), W per scan:
    ring64_w2048   64 rings, W = 2048, a point count that is no multiple of 64
    prefix_w256    a partial ring BEFORE the first ring start (row 0), then 64 rings, W = 256
    rings50_w512   fewer than 64 rings, W = 512
    rings67_w256   67 rings: the first three get rows -3..-1, which numpy wraps onto rows 61..63
    ang00..ang19   20 scans at W = 64 for the angle grid; one sector of ten rings is always empty (never-valid pixels), some
                   points lie outside the depth range
Contents:
    meta/scans, meta/angle_scans (names), meta/min_depth, meta/max_depth, meta/numpy, meta/torch
    scan/<name>/points [N,4] f32, W, winner [64,W] i32 (-1 = empty), row [N] i16 (negative = wrapped), col [N] i16
    angles/ref  [2,64,64] f32  compute_avg_angles' result      angles/f64  the same formulae in float64
    angles/e_ref = max |ref - f64|                              angles/never [64,64] bool  pixels valid in no scan
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

REF = os.environ.get("DUSTY_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import raw_scan_util as U  # noqa: E402

MIN_DEPTH, MAX_DEPTH = 0.9, 120.0


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    for name in ("numba", "joblib", "matplotlib", "matplotlib.cm", "tqdm", "torchvision", "torchvision.transforms",
                 "torchvision.transforms.functional", "datasets"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["numba"].jit = lambda f: f
    sys.modules["tqdm"].tqdm = lambda it, *a, **k: it
    sys.modules["matplotlib"].cm = sys.modules["matplotlib.cm"]
    sys.modules["matplotlib.cm"].turbo = lambda a: np.zeros((len(a), 4))
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.modules["torchvision.transforms"].functional = sys.modules["torchvision.transforms.functional"]
    kitti = _load(os.path.join(REF, "datasets", "kitti.py"), "datasets.kitti")
    sys.modules["datasets"].kitti = kitti
    return _load(os.path.join(REF, "process_kitti.py"), "ref_process_kitti"), kitti


def make_scan(rng, rings, per_ring, prefix=False, hole=False, out_of_range=0.0):
    """a raw scan [N,4] f32: `rings` sweeps of the azimuth from just above 0 to just below 2 pi (quadrants 0, 1, 2, 3), top
    ring first; prefix: the tail of one more sweep in front, starting in quadrant 1"""
    elev = np.deg2rad(np.linspace(2.0, -24.8, rings))
    parts = []
    sweeps = ([(elev[0] + 0.004, True)] if prefix else []) + [(e, False) for e in elev]
    for k, (e, partial) in enumerate(sweeps):
        n = per_ring + int(rng.integers(-4, 5))
        th = np.sort(rng.uniform(0.01, 2 * np.pi - 0.01, n))
        if partial:
            th = th[th > 2.0]
        if hole and 40 <= k < 50:
            th = th[(th < 1.0) | (th > 1.6)]
        r = rng.uniform(2.0, 80.0, th.size)
        u = rng.random(th.size)
        r = np.where(u < out_of_range / 2, rng.uniform(0.3, 0.85, th.size), r)
        r = np.where(u > 1 - out_of_range / 2, rng.uniform(121.0, 140.0, th.size), r)
        phi = e + rng.normal(0, 5e-4, th.size)
        xyz = np.stack([r * np.cos(phi) * np.cos(th), r * np.cos(phi) * np.sin(th), r * np.sin(phi)], -1)
        xyz = np.rint(xyz * 256.0) / 256.0
        refl = rng.integers(0, 100, th.size) / 100.0
        parts.append(np.concatenate([xyz, refl[:, None]], -1))
    pts = np.concatenate(parts).astype(np.float32)
    if len(pts) % 64 == 0:
        pts = pts[:-1]
    return pts


def reference_projection(ref, pts, W, tmp, tag):
    """process_point_clouds on a .bin written here -> (projection [64,W,4], winner [64,W], row [N], col [N])"""
    d = os.path.join(tmp, tag, "dataset/sequences/00/velodyne")
    os.makedirs(d)
    path = os.path.join(d, "000000.bin")
    pts.tofile(path)
    seen = {}
    inner = ref.projection

    def recording(source, grid, order, H, W_):
        seen["grid"], seen["order"] = np.array(grid), np.array(order)
        return inner(source, grid, order, H, W_)

    ref.projection = recording
    try:
        ref.process_point_clouds(path, 64, W)
    finally:
        ref.projection = inner
    proj = np.load(path.replace("dataset/sequences", "dusty-gan/sequences").replace(".bin", ".npy"))
    grid, order = seen["grid"], seen["order"]
    winner = np.full((64, W), -1, dtype=np.int64)
    for i in order:                      # `scatter`: later writes win
        winner[grid[i, 0], grid[i, 1]] = i
    assert proj.dtype == np.float32 and proj.shape == (64, W, 4)
    assert np.array_equal(proj, U.expected_image(pts, winner))
    return proj, winner, grid[:, 0], grid[:, 1]


def angles_f64(xyz, max_depth):
    """compute_avg_angles' formulae (process_kitti.py:143-183) in float64 on the same unit-space batches [S,3,H,W]"""
    x, y, z = (xyz[:, c].astype(np.float64) for c in range(3))
    valid = np.sqrt(x ** 2 + y ** 2 + z ** 2) * max_depth > 1e-8
    cnt = valid.sum(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        pitch = (np.arctan2(z, np.sqrt(x ** 2 + y ** 2)) * valid).sum(0) / cnt
        yaw = (np.arctan2(y, x) * valid).sum(0) / cnt
    never = cnt == 0
    row_mean = np.nanmean(pitch, axis=1, keepdims=True)
    col_mean = np.nanmean(yaw, axis=0, keepdims=True)
    pitch = np.where(never, row_mean, pitch)
    yaw = np.where(never, col_mean, yaw)
    return np.stack([pitch, yaw]), never


def main():
    ref, kitti = load_reference()
    rng = np.random.default_rng(20261016)
    cases = [("ring64_w2048", 2048, dict(rings=64, per_ring=150)),
             ("prefix_w256", 256, dict(rings=64, per_ring=90, prefix=True)),
             ("rings50_w512", 512, dict(rings=50, per_ring=110)),
             ("rings67_w256", 256, dict(rings=67, per_ring=70))]
    ang_names = [f"ang{k:02d}" for k in range(20)]
    cases += [(n, 64, dict(rings=64, per_ring=20, hole=True, out_of_range=0.06)) for n in ang_names]
    d = {"meta/scans": np.array([c[0] for c in cases]), "meta/angle_scans": np.array(ang_names),
         "meta/min_depth": np.array(MIN_DEPTH), "meta/max_depth": np.array(MAX_DEPTH),
         "meta/numpy": np.array(np.__version__), "meta/torch": np.array(torch.__version__)}
    projs = {}
    with tempfile.TemporaryDirectory() as tmp:
        ds = kitti.KITTIOdometry(tmp, "val", shape=(64, 64), min_depth=MIN_DEPTH, max_depth=MAX_DEPTH)  # (an empty datalist)
        for name, W, kw in cases:
            pts = make_scan(rng, **kw)
            proj, winner, row, col = reference_projection(ref, pts, W, tmp, name)
            n_ex, filled = U.check_cap(pts, W, winner, row, col)   # both parts of the cap (tests/raw_scan_util.py)
            print(f"{name}: {len(pts)} points, {filled} cells, {n_ex} excluded, rows {row.min()}..{row.max()}")
            assert len(pts) % 64
            p = f"scan/{name}/"
            d[p + "points"], d[p + "W"] = pts, np.array(W)
            d[p + "winner"], d[p + "row"], d[p + "col"] = winner.astype(np.int32), row.astype(np.int16), col.astype(np.int16)
            projs[name] = proj
        assert d["scan/prefix_w256/row"][0] == 0 and (np.diff(d["scan/prefix_w256/row"].astype(int)) >= 0).all()
        assert d["scan/rings50_w512/row"].min() == 14 and d["scan/rings67_w256/row"].min() == -3
        # the batches compute_avg_angles sees: __getitem__ (datasets/kitti.py:79-88) without the resize - preprocess at the
        # native shape, then to_tensor's HWC -> CHW
        items = []
        for n in ang_names:
            out = ds.preprocess({"xyz": projs[n][..., :3].copy()})
            items.append(torch.from_numpy(np.ascontiguousarray(out["xyz"].transpose(2, 0, 1))))
        batch = torch.stack(items)
        loader = [{"xyz": batch}]                                   # one batch of 20 (the reference's batch size is 64)
        loader = type("Loader", (list,), {"dataset": ds})(loader)
        angles, mean_valid = ref.compute_avg_angles(loader)
    a64, never = angles_f64(batch.numpy(), MAX_DEPTH)
    assert np.array_equal(never, mean_valid[0].numpy() == 0) and 0 < never.sum() < never.size // 8
    assert not never.all(0).any() and not never.all(1).any()
    e_ref = float(np.abs(angles.numpy().astype(np.float64) - a64).max())
    print(f"angles: {never.sum()} never-valid pixels, e_ref = {e_ref:.3e}")
    d["angles/ref"], d["angles/f64"], d["angles/e_ref"], d["angles/never"] = angles.numpy(), a64, np.array(e_ref), never
    path = os.path.join(HERE, "raw_scan.npz")
    np.savez_compressed(path, **d)
    print("wrote", path, f"{os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
