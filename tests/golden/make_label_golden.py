"""Generate tests/golden/label_image.npz from the REFERENCE's own process_kitti.py.

Runs only where the reference's sources are at hand (DUSTY_REFERENCE, default /root/reference), on the CPU:
    python tests/golden/make_label_golden.py
process_kitti.py is loaded by path and `process_point_clouds` is called unmodified on three scans of raw_scan.npz
(prefix_w256, rings50_w512, rings67_w256), each written as a `.bin` beside a seeded `.label` file in a temporary SemanticKITTI
tree.  The module's imports that the function never uses are the stand-ins of make_raw_scan_golden.py - numba (`jit` =
identity: `scatter` runs as the plain Python loop it is), joblib, tqdm, datasets.kitti - while matplotlib is the REAL one:
`cm.turbo` makes the reference's palette at import.

Labels: one uint32 per point; the lower half a raw id drawn from the reference's own table, the upper half a random instance
id.  (The scans contain no two points of one cell with the same float32 range - make_raw_scan_golden.py asserts it - so the
reference's unstable argsort leaves nothing open.)
Contents:
    meta/scans                 the three names
    table/ids, table/classes   the reference's labelmap as two integer arrays
    palette                    the first 60 bytes of the PNGs' palette (the same in all three)
    scan/<name>/labels [N] u32     scan/<name>/sem [64,W] u8 = the decoded PNG indices
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image

REF = os.environ.get("DUSTY_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import label_util as LU  # noqa: E402
from tests import raw_scan_util as U  # noqa: E402


def load_reference():
    import matplotlib.cm  # noqa: F401  (the real one)
    for name in ("numba", "joblib", "tqdm", "datasets", "datasets.kitti"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["numba"].jit = lambda f: f
    sys.modules["tqdm"].tqdm = lambda it, *a, **k: it
    sys.modules["datasets"].kitti = sys.modules["datasets.kitti"]
    sys.modules["datasets.kitti"].KITTIOdometry = None
    spec = importlib.util.spec_from_file_location("ref_process_kitti", os.path.join(REF, "process_kitti.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_process_kitti"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference()
    raw = U.load()
    rng = np.random.default_rng(20261021)
    ids = np.array(sorted(ref.labelmap), dtype=np.int64)
    d = {"meta/scans": np.array(LU.SCANS), "table/ids": ids.astype(np.int32),
         "table/classes": np.array([ref.labelmap[int(i)] for i in ids], dtype=np.int32)}
    palettes = []
    with tempfile.TemporaryDirectory() as tmp:
        for k, name in enumerate(LU.SCANS):
            pts, W, winner, row, col = U.scan(raw, name)
            labels = (rng.choice(ids, len(pts)).astype(np.uint32) | (rng.integers(0, 1 << 16, len(pts)).astype(np.uint32) << 16))
            seq = os.path.join(tmp, "dataset/sequences", f"{k:02d}")
            os.makedirs(os.path.join(seq, "velodyne"))
            os.makedirs(os.path.join(seq, "labels"))
            point_path = os.path.join(seq, "velodyne", "000000.bin")
            pts.tofile(point_path)
            labels.tofile(os.path.join(seq, "labels", "000000.label"))
            ref.process_point_clouds(point_path, 64, W)
            png = os.path.join(tmp, "dusty-gan/sequences", f"{k:02d}", "labels", "000000.png")
            with Image.open(png) as img:
                assert img.mode == "P"
                sem = np.array(img, dtype=np.uint8)
                palettes.append(np.array(img.getpalette()[:60], dtype=np.uint8))
            assert sem.shape == (64, W)
            # the recorded winners of raw_scan.npz explain the image: same scatter, same order
            lut = np.full(65536, 255, dtype=np.uint8)
            lut[ids] = d["table/classes"]
            want = np.zeros((64, W), dtype=np.uint8)
            want[winner >= 0] = lut[labels[winner[winner >= 0]] & 0xFFFF]
            assert np.array_equal(sem, want)
            print(f"{name}: {len(pts)} points, W = {W}, {int((winner >= 0).sum())} cells, classes {np.unique(sem).tolist()}")
            d[f"scan/{name}/labels"], d[f"scan/{name}/sem"] = labels, sem
    assert all(np.array_equal(p, palettes[0]) for p in palettes)
    d["palette"] = palettes[0]
    path = os.path.join(HERE, "label_image.npz")
    np.savez_compressed(path, **d)
    print("wrote", path, f"{os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
