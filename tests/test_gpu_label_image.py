"""Label images on the GPU (csrc/label_image.hip, dusty_gan_amd/datasets/labels.py, process_kitti --labels) against what the
reference's process_kitti.py wrote (tests/golden/label_image.npz) and against tests/label_util.py.  Integer work: every
comparison is exact."""
import os

import numpy as np
import pytest
import torch

from tests import beam_ref as BR
from tests import label_util as LU
from tests import raw_scan_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from dusty_gan_amd import _lib
    _lib.lib()
    from dusty_gan_amd.datasets import labels as LB
    from dusty_gan_amd.datasets import raw as R
    return R, LB


@pytest.fixture(scope="module")
def g():
    return LU.load()


@pytest.fixture(scope="module")
def raw_g():
    return U.load()


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _check_scan(out, cells, sem, inst, pts, labels, winner, want_sem, LB):
    """one scan's images against the golden PNG indices, the golden winners and the projection's own `out`"""
    W = winner.shape[1]
    assert sem.shape == (LU.H, W) and sem.dtype == np.uint8 and inst.dtype == np.uint16
    assert np.array_equal(sem, want_sem)
    on = winner >= 0
    assert np.array_equal(inst[on], (labels[winner[on]] >> 16).astype(np.uint16)) and not inst[~on].any() and not sem[~on].any()
    # the label of every non-empty cell is the label of the record `out` holds there
    assert np.array_equal(out.view(np.uint32)[on], pts.view(np.uint32)[winner[on]])
    assert np.array_equal(sem[on], LB.SEMANTIC_KITTI_LUT[labels[winner[on]] & 0xFFFF])


@pytest.mark.parametrize("name", LU.SCANS)
def test_golden_scan_alone(mods, g, raw_g, name):
    R, LB = mods
    pts, W, winner, _, _ = U.scan(raw_g, name)
    labels = g[f"scan/{name}/labels"]
    out, cells, keys = R.project_scans(torch.from_numpy(pts), [0, len(pts)], W=W, return_cells=True, return_keys=True)
    sem, inst = LB.project_labels(keys, [0, len(pts)], labels, LU.H, W)
    assert sem.dtype == torch.uint8 and tuple(sem.shape) == (1, LU.H, W)
    _check_scan(out[0].cpu().numpy(), cells.cpu().numpy(), sem[0].cpu().numpy(), _u16(inst[0]), pts, labels, winner,
                g[f"scan/{name}/sem"], LB)
    # without the instance image, straight at the entry point: the same classes
    from dusty_gan_amd import _lib as L
    dev = keys.device
    offs = torch.tensor([0, len(pts)], device=dev)
    lab = torch.from_numpy(labels.view(np.int32).copy()).to(dev)
    sem2 = torch.empty(1, LU.H, W, dtype=torch.uint8, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    lut = LB.device_lut(dev)
    args = (L.ptr(keys), L.ptr(offs), L.ptr(lab), L.ptr(lut), 1, LU.H, W, L.ptr(sem2), None, L.ptr(st), L.stream_ptr())
    assert L.lib().dg_scan_labels(*args) == L.DG_OK
    assert torch.equal(sem2, sem) and int(st[0]) == 0
    for k in (0, 1, 2, 3, 7, 9):   # a NULL pointer other than inst
        bad = list(args)
        bad[k] = None
        assert L.lib().dg_scan_labels(*bad) == L.DG_EINVAL, k
    bad = list(args)
    bad[4] = 0
    assert L.lib().dg_scan_labels(*bad) == L.DG_EINVAL


def test_golden_scans_in_one_call(mods, g, raw_g):
    """S = 3 in one call; the scans' golden widths differ, so one width at a time: all three scans at that W, compared where
    the golden image is of that W (the others must still equal their own single-scan result)"""
    R, LB = mods
    scans = [U.scan(raw_g, n) for n in LU.SCANS]
    labels = [g[f"scan/{n}/labels"] for n in LU.SCANS]
    pts = np.concatenate([s[0] for s in scans])
    lab = np.concatenate(labels)
    offs = np.concatenate([[0], np.cumsum([len(s[0]) for s in scans])])
    checked = 0
    for W in sorted({s[1] for s in scans}):
        out, cells, keys = R.project_scans(torch.from_numpy(pts), offs, W=W, return_cells=True, return_keys=True)
        sem, inst = LB.project_labels(keys, offs, lab, LU.H, W)
        assert tuple(sem.shape) == (3, LU.H, W)
        for k, (name, s) in enumerate(zip(LU.SCANS, scans)):
            if s[1] == W:
                _check_scan(out[k].cpu().numpy(), None, sem[k].cpu().numpy(), _u16(inst[k]), s[0], labels[k], s[2],
                            g[f"scan/{name}/sem"], LB)
                checked += 1
            o1, k1 = R.project_scans(torch.from_numpy(s[0]), [0, len(s[0])], W=W, return_keys=True)
            s1, i1 = LB.project_labels(k1, [0, len(s[0])], labels[k], LU.H, W)
            assert torch.equal(s1[0], sem[k]) and torch.equal(i1[0], inst[k])
    assert checked == 3


def test_beam_projection_shuffled_cloud(mods):
    """an 8-beam sensor, W = 32, about 600 shuffled points, three to a cell: through project_clouds_beams"""
    R, LB = mods
    beams, W = BR.uniform_beams(8), 32
    jitter = 0.15 * np.deg2rad(28.0) / 7
    pts = BR.synthetic_sensor(beams, 96, seed=77, jitter=jitter, drop=0.2)
    assert 550 <= len(pts) <= 680
    assert BR.near_column_edge(pts, W).size == 0 and BR.near_midpoint(pts, beams).size == 0
    rng = np.random.default_rng(78)
    ids = np.flatnonzero(LB.SEMANTIC_KITTI_LUT != 255)
    labels = rng.choice(ids, len(pts)).astype(np.uint32) | (rng.integers(0, 1 << 16, len(pts)).astype(np.uint32) << 16)
    image, cell = BR.project(pts, beams, W)
    assert (cell >= 0).all() and len(np.unique(cell)) < len(pts)          # cells with more than one point
    want_sem, want_inst = LU.label_images(cell // W, cell % W, BR.range64(pts).astype(np.float32), labels,
                                          LB.SEMANTIC_KITTI_LUT, 8, W)
    out, cells, keys = R.project_clouds_beams(torch.from_numpy(pts), [0, len(pts)], beams, W=W, return_cells=True, return_keys=True)
    assert np.array_equal(cells.cpu().numpy(), cell) and np.array_equal(out[0].cpu().numpy().view(np.uint32), image.view(np.uint32))
    sem, inst = LB.project_labels(keys, [0, len(pts)], labels, 8, W)
    assert np.array_equal(sem[0].cpu().numpy(), want_sem) and np.array_equal(_u16(inst[0]), want_inst)
    assert len(np.unique(want_sem)) > 10


def test_tie_lower_index_wins(mods):
    """two points with identical coordinates and different labels: the lower index's label, in either order"""
    R, LB = mods
    beams, W = BR.uniform_beams(4), 16
    p = np.array([[10.0, 3.0, 0.1, 0.5]], dtype=np.float32)
    far = np.array([[20.0, 6.0, 0.2, 0.5]], dtype=np.float32)    # the same ray, farther: never the winner
    pts = np.concatenate([far, p, p])
    for first, second in ((10, 30), (30, 10)):
        labels = np.array([40, first | (5 << 16), second | (9 << 16)], dtype=np.uint32)
        out, cells, keys = R.project_clouds_beams(torch.from_numpy(pts), [0, 3], beams, W=W, return_cells=True, return_keys=True)
        c = cells.cpu().numpy()
        assert c[0] == c[1] == c[2] >= 0
        sem, inst = LB.project_labels(keys, [0, 3], labels, 4, W)
        sem, inst = sem[0].cpu().numpy().reshape(-1), _u16(inst[0]).reshape(-1)
        assert sem[c[1]] == LB.SEMANTIC_KITTI_LUT[first] and inst[c[1]] == 5
        assert np.count_nonzero(sem) == 1


def test_unknown_id_is_named(mods, raw_g):
    R, LB = mods
    pts, W, winner, _, _ = U.scan(raw_g, "rings50_w512")
    labels = np.full(len(pts), 40, dtype=np.uint32)
    w = int(winner[winner >= 0][17])
    labels[w] = 77 | (3 << 16)                       # no such SemanticKITTI id, on a point that wins its cell
    both = np.concatenate([pts, pts])
    offs = [0, len(pts), 2 * len(pts)]
    _, keys = R.project_scans(torch.from_numpy(both), offs, W=W, return_keys=True)
    with pytest.raises(R.RawScanError, match="77") as e:
        LB.project_labels(keys, offs, np.concatenate([np.full(len(pts), 40, dtype=np.uint32), labels]), LU.H, W,
                          names=["a.label", "b.label"])
    assert "b.label" in str(e.value) and "a.label" not in str(e.value)
    assert len(e.value.names) == 1 and "[77]" in e.value.names[0]


def _kitti_scan(rng, W, per_ring=40):
    """64 rings swept counter-clockwise from quadrant 0, every point near the middle of a column of a W-wide image"""
    parts = []
    for e in np.deg2rad(np.linspace(2.0, -24.8, 64)):
        k = np.sort(rng.choice(W, per_ring, replace=True))                   # (a column may be hit twice: a winner to pick)
        # column of azimuth th: ((-(-th') / pi + 1) / 2) W with th' in (-pi, pi]; th in (0, 2 pi) sweeps columns W/2 .. W-1, 0 .. W/2-1
        th = (k + 0.5 + rng.uniform(-0.2, 0.2, per_ring)) * (2 * np.pi / W)
        th = np.sort(th)
        r = rng.uniform(3.0, 70.0, per_ring)
        parts.append(np.stack([r * np.cos(e) * np.cos(th), r * np.cos(e) * np.sin(th), r * np.sin(e), rng.random(per_ring)], -1))
    return np.concatenate(parts).astype(np.float32)


def test_process_kitti_labels_end_to_end(mods, tmp_path, monkeypatch):
    R, LB = mods
    from dusty_gan_amd import process_kitti as P
    monkeypatch.setattr(P, "W", 64)
    root = str(tmp_path)
    rng = np.random.default_rng(21)
    ids = np.flatnonzero(LB.SEMANTIC_KITTI_LUT != 255)
    vel, lab_dir = os.path.join(root, "dataset/sequences/00/velodyne"), os.path.join(root, "dataset/sequences/00/labels")
    os.makedirs(vel)
    os.makedirs(lab_dir)
    scans = []
    for k in range(3):
        pts = _kitti_scan(rng, 64)
        labels = rng.choice(ids, len(pts)).astype(np.uint32) | (rng.integers(0, 1 << 16, len(pts)).astype(np.uint32) << 16)
        pts.tofile(os.path.join(vel, f"{k:06d}.bin"))
        if k < 2:                                      # the third scan has no .label file: no PNG for it
            labels.tofile(os.path.join(lab_dir, f"{k:06d}.label"))
        scans.append((pts, labels))
    assert P.main(["--root-dir", root, "--labels", "--chunk", "2", "--num-workers", "3"]) == 0
    out_lab = os.path.join(root, "dusty-gan/sequences/00/labels")
    assert sorted(os.listdir(out_lab)) == ["000000.png", "000001.png"]
    assert len(os.listdir(os.path.join(root, "dusty-gan/sequences/00/velodyne"))) == 3
    for k in range(2):
        pts, labels = scans[k]
        row, col = LU.kitti_grid(pts, 64)
        assert len(np.unique(row * 64 + col)) < len(pts)
        want, _ = LU.label_images(row, col, LU.depth32(pts), labels, LB.SEMANTIC_KITTI_LUT, 64, 64)
        got, pal = LB.read_label_png(os.path.join(out_lab, f"{k:06d}.png"), return_palette=True)
        assert got.shape == (64, 64) and np.array_equal(got, want) and len(np.unique(want)) > 10
        assert np.array_equal(pal[:20], LB.palette())
        # and it labels the very records of the scan's .npy
        npy = np.load(os.path.join(root, "dusty-gan/sequences/00/velodyne", f"{k:06d}.npy"))
        win = LU.winner_image(row, col, LU.depth32(pts), 64, 64)
        assert np.array_equal(npy.view(np.uint32)[win >= 0], pts.view(np.uint32)[win[win >= 0]])
    # a second run with --skip-existing writes nothing
    files = [os.path.join(d, f) for d, _, fs in os.walk(os.path.join(root, "dusty-gan")) for f in fs]
    before = {f: os.stat(f).st_mtime_ns for f in files}
    assert len(before) == 5
    assert P.main(["--root-dir", root, "--labels", "--skip-existing"]) == 0
    after = [os.path.join(d, f) for d, _, fs in os.walk(os.path.join(root, "dusty-gan")) for f in fs]
    assert {f: os.stat(f).st_mtime_ns for f in after} == before
    # a missing PNG alone is made again, its .npy left alone
    os.remove(os.path.join(out_lab, "000001.png"))
    assert P.main(["--root-dir", root, "--labels", "--skip-existing"]) == 0
    assert {f: os.stat(f).st_mtime_ns for f in before if not f.endswith("000001.png")} == \
        {f: t for f, t in before.items() if not f.endswith("000001.png")}
    assert np.array_equal(LB.read_label_png(os.path.join(out_lab, "000001.png")),
                          LU.label_images(*LU.kitti_grid(scans[1][0], 64), LU.depth32(scans[1][0]), scans[1][1],
                                          LB.SEMANTIC_KITTI_LUT, 64, 64)[0])
