"""python -m dusty_gan_amd.remove_objects on the GPU, on the tiny seeded checkpoint the reconstruction tests use: three
synthetic clouds with labels in, kept records + generated background out; and a two-scan dataset written by
process_kitti --labels through --split."""
import csv
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_synthesis import make_world

pytestmark = pytest.mark.gpu
STEMS = ["scan_a", "scan_b", "scan_c"]
SUBS = {"images": ".png", "labels": ".label", "labels_png": ".png", "maps": ".npy", "points": ".bin"}
RUN = ["--num-step", "5", "--dilate", "1"]
CAR, ROAD, PERSON = 10, 40, 30      # raw SemanticKITTI ids


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """the generator's own outputs for three latents as clouds; a band of columns is labelled car / person, the rest road"""
    from dusty_gan_amd import synthesis as S
    from dusty_gan_amd import utils
    tmp = tmp_path_factory.mktemp("remove_objects")
    argv = make_world(tmp, "dusty2_dcgan_eqlr", "dusty2")
    cfg, G, lidar, device = utils.setup(argv[1], argv[3], ema=True, fix_noise=True)
    out = S.synthesize(cfg, G, lidar, S.sample_latents(cfg, device, 3, "random", 3), normals=False)
    records, counts = S.export_points(out["depth"], lidar, tol=0.0, from_tanh=False)
    clouds, labels = tmp / "clouds", tmp / "labels"
    clouds.mkdir()
    labels.mkdir()
    rng = np.random.default_rng(2)
    rows, labs = [], []
    for b, stem in enumerate(STEMS):
        rec = records[b, :int(counts[b])].cpu().numpy().copy()
        if b == 1:
            rec = rec[: int(0.6 * len(rec))]          # a shorter cloud: the batch is padded
        if b == 2:
            rec = rec[rng.permutation(len(rec))]      # no point order
        rec[:, 3] = np.arange(len(rec), dtype=np.float32)   # the payload: a record's row in its file
        az = np.arctan2(rec[:, 1], rec[:, 0])
        lab = np.full(len(rec), ROAD, dtype=np.uint32)
        lab[(az > 0.3) & (az < 0.6)] = CAR
        lab[(az > -2.0) & (az < -1.9) & (rec[:, 2] < 0)] = PERSON
        lab |= rng.integers(0, 1 << 16, len(rec)).astype(np.uint32) << 16
        rec.tofile(clouds / f"{stem}.bin")
        lab.astype("<u4").tofile(labels / f"{stem}.label")
        rows.append(rec)
        labs.append(lab)
    del G
    return {"tmp": tmp, "argv": argv, "clouds": clouds, "labels": labels, "rows": rows, "labs": labs}


def run(world, save, *extra):
    from dusty_gan_amd import remove_objects
    out_dir = remove_objects.main(world["argv"] + ["--points", str(world["clouds"]), "--labels", str(world["labels"]),
                                                   "--save-dir-path", str(save)] + RUN + list(extra))
    assert out_dir == os.path.join(str(save), "removal")
    return out_dir


@pytest.fixture(scope="module")
def whole_batch(world):
    return run(world, world["tmp"] / "whole", "--batch-size", "3")


def read_stats(out_dir):
    with open(os.path.join(out_dir, "stats.csv"), newline="") as f:
        return list(csv.reader(f))


def test_files_kept_records_and_fill(world, whole_batch):
    from dusty_gan_amd import utils
    from dusty_gan_amd.datasets.labels import CLASS_NAMES, read_label_png
    from dusty_gan_amd.datasets.raw import read_clouds
    out_dir = whole_batch
    assert sorted(os.listdir(out_dir)) == sorted(list(SUBS) + ["stats.csv"])
    for sub, ext in SUBS.items():
        assert sorted(os.listdir(os.path.join(out_dir, sub))) == [s + ext for s in STEMS], sub
    table = read_stats(out_dir)
    assert table[0] == ["name", "points_in", "points_kept", "points_filled", "pixels_removed", "pixels_filled", "in_front"] + \
        [f"px_{c}" for c in CLASS_NAMES]
    assert [r[0] for r in table[1:]] == STEMS
    cfg, G, lidar, device = utils.setup(world["argv"][1], world["argv"][3], ema=True, fix_noise=True)
    H, W = lidar.H, lidar.W
    for b, stem in enumerate(STEMS):
        src, src_lab = world["rows"][b], world["labs"][b]
        stats = dict(zip(table[0][1:], (int(v) for v in table[b + 1][1:])))
        maps = np.load(os.path.join(out_dir, "maps", f"{stem}.npy"))
        assert maps.shape == (4, H, W) and maps.dtype == np.float32
        tgt_inv, remove, source, inv_out = maps
        rec = np.fromfile(os.path.join(out_dir, "points", f"{stem}.bin"), np.float32).reshape(-1, 4)
        lab = np.fromfile(os.path.join(out_dir, "labels", f"{stem}.label"), np.uint32)
        nk, nf = stats["points_kept"], stats["points_filled"]
        assert stats["points_in"] == len(src) and len(rec) == len(lab) == nk + nf
        # the kept part: a bit-exact, order-preserving subset of the input, labels with it
        kept = rec[:nk]
        rows = kept[:, 3].astype(np.int64)
        assert (np.diff(rows) > 0).all()
        assert np.array_equal(kept.view(np.uint32), src[rows].view(np.uint32)) and np.array_equal(lab[:nk], src_lab[rows])
        # no kept record's pixel is in `remove`, and every record that left was in one
        unit, counts = read_clouds([world["clouds"] / f"{stem}.bin"], lidar.max_depth, device)
        _, valid, idx = lidar.points_to_depth(unit, drop_value=1, tau=2, counts=counts, return_index=True)
        idx = idx[0].cpu().numpy()
        in_removed = (idx >= 0) & (remove.reshape(-1)[np.maximum(idx, 0)] != 0)
        assert not in_removed[rows].any()
        gone = np.setdiff1d(np.arange(len(src)), rows)
        assert in_removed[gone].all() and len(gone) > 0
        # the appended records: label fill, land only on pixels the generator filled
        fill = rec[nk:]
        assert (lab[nk:] == 0).all() and (fill[:, 3] == 0).all()
        if nf:
            f_unit = torch.from_numpy(fill.copy()).to(device)[None]
            f_unit[..., :3] /= lidar.max_depth
            _, _, f_idx = lidar.points_to_depth(f_unit, drop_value=1, tau=2, return_index=True)
            f_idx = f_idx[0].cpu().numpy()
            assert (f_idx >= 0).all() and (source.reshape(-1)[f_idx] == 2).all()
        # stats against the maps
        mask = valid[0, 0].cpu().numpy()
        assert stats["pixels_removed"] == int(((remove != 0) & mask).sum())
        assert stats["pixels_filled"] == int((source == 2).sum()) and nf <= stats["pixels_filled"]
        assert stats["in_front"] == int(((source == 2) & mask & (inv_out > tgt_inv)).sum())
        assert np.array_equal(inv_out.view(np.uint32)[source == 1], tgt_inv.view(np.uint32)[source == 1])
        assert not (source[remove != 0] == 1).any() and not inv_out[source == 0].any()
        assert stats["px_car"] > 0 and stats["px_road"] > 0 and sum(stats[f"px_{c}"] for c in CLASS_NAMES) == int(mask.sum())
        sem_out = read_label_png(os.path.join(out_dir, "labels_png", f"{stem}.png"))
        assert sem_out.shape == (H, W) and not np.isin(sem_out[source == 1], [1, 6]).any() and not sem_out[source != 1].any()
        assert set(np.unique(sem_out)) <= {0, 9}
    removed = [int(r[table[0].index("pixels_removed")]) for r in table[1:]]
    filled = [int(r[table[0].index("pixels_filled")]) for r in table[1:]]
    print("pixels_removed", removed, "pixels_filled", filled)
    assert max(removed) > 0 and max(filled) > 0


def test_files_do_not_depend_on_the_batch(world, whole_batch):
    one = run(world, world["tmp"] / "one", "--batch-size", "1")
    differ = []
    for sub in SUBS:
        for name in sorted(os.listdir(os.path.join(whole_batch, sub))):
            if open(os.path.join(one, sub, name), "rb").read() != open(os.path.join(whole_batch, sub, name), "rb").read():
                differ.append((sub, name))
    if open(os.path.join(one, "stats.csv"), "rb").read() != open(os.path.join(whole_batch, "stats.csv"), "rb").read():
        differ.append("stats.csv")
    print("files that differ:", differ)
    assert not differ


def test_split_of_a_dataset_written_by_process_kitti(world, tmp_path, monkeypatch):
    """two raw 64-ring scans with labels -> process_kitti --labels -> remove_objects --split test"""
    from dusty_gan_amd import process_kitti as P
    from dusty_gan_amd import remove_objects
    from dusty_gan_amd.utils.config import dump_config, load_config
    from tests.test_gpu_label_image import _kitti_scan
    monkeypatch.setattr(P, "W", 256)
    root = str(tmp_path / "kitti")
    rng = np.random.default_rng(31)
    for seq in ("00", "11"):                       # 00: of the train split (angles.pt); 11: of the test split
        vel, lab_dir = os.path.join(root, "dataset/sequences", seq, "velodyne"), os.path.join(root, "dataset/sequences", seq, "labels")
        os.makedirs(vel)
        os.makedirs(lab_dir)
        for k in range(2):
            pts = _kitti_scan(rng, 256, per_ring=200)
            lab = np.full(len(pts), ROAD, dtype=np.uint32)
            az = np.arctan2(pts[:, 1], pts[:, 0])
            lab[(az > 0.3) & (az < 0.6)] = CAR
            pts.tofile(os.path.join(vel, f"{k:06d}.bin"))
            lab.tofile(os.path.join(lab_dir, f"{k:06d}.label"))
    assert P.main(["--root-dir", root, "--labels"]) == 0
    import shutil
    shutil.copy(os.path.join(root, "angles.pt"), os.path.join(root, "dusty-gan", "angles.pt"))   # where the config's root looks
    split = "test"
    cfg = load_config(["model=dusty2_dcgan_eqlr", "dataset=kitti_odometry", f"dataset.root={os.path.join(root, 'dusty-gan')}",
                       "dataset.shape=[64,1024]", "solver.batch_size=4", "enable_amp=true"])
    cfg_path = str(tmp_path / "kitti.yaml")
    dump_config(cfg, cfg_path)
    out_dir = remove_objects.main(["--model-path", world["argv"][1], "--config-path", cfg_path, "--split", split,
                                   "--save-dir-path", str(tmp_path)] + RUN)
    assert sorted(os.listdir(out_dir)) == sorted(list(SUBS) + ["stats.csv"])
    for sub, ext in SUBS.items():
        assert sorted(os.listdir(os.path.join(out_dir, sub))) == [f"{i:06d}_{i:06d}{ext}" for i in range(2)], sub
    table = read_stats(out_dir)
    for r in table[1:]:
        stats = dict(zip(table[0][1:], (int(v) for v in r[1:])))
        maps = np.load(os.path.join(out_dir, "maps", r[0] + ".npy"))
        rec = np.fromfile(os.path.join(out_dir, "points", r[0] + ".bin"), np.float32).reshape(-1, 4)
        lab = np.fromfile(os.path.join(out_dir, "labels", r[0] + ".label"), np.uint32)
        assert stats["pixels_removed"] > 0 and stats["px_car"] > 0
        assert len(rec) == len(lab) == stats["points_kept"] + stats["points_filled"]
        assert stats["points_kept"] == int((maps[2] == 1).sum()) and not (maps[2][maps[1] != 0] == 1).any()
    # a missing label image is an error that names the file
    os.remove(os.path.join(root, "dusty-gan/sequences/11/labels/000001.png"))
    with pytest.raises(FileNotFoundError, match="000001.png"):
        remove_objects.main(["--model-path", world["argv"][1], "--config-path", cfg_path, "--split", split, "--save-dir-path",
                             str(tmp_path / "again")] + RUN)
