"""The ray-drop transfer through the model (64 x 1024, 20 inversion steps): raydrop.transfer tied to the generator's own head
kernel, and python -m dusty_gan_amd.transfer_raydrop on three labelled clouds - the generator's own outputs for known latents,
one shorter, one shuffled, the fourth column carrying each record's row number."""
import csv
import os

import numpy as np
import pytest
import torch

from tests import raydrop_util as R
from tests.test_gpu_synthesis import make_world

pytestmark = pytest.mark.gpu
STEMS = ["sim_a", "sim_b", "sim_c"]
STEPS = ["--num-step", "20"]
K = 2


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from dusty_gan_amd import synthesis as S
    from dusty_gan_amd import utils
    tmp = tmp_path_factory.mktemp("raydrop")
    argv = {m: make_world(tmp, f"{m}_dcgan_eqlr", m) for m in ("dusty1", "dusty2")}
    cfg, G, lidar, device = utils.setup(argv["dusty2"][1], argv["dusty2"][3], ema=True, fix_noise=True)
    out = S.synthesize(cfg, G, lidar, S.sample_latents(cfg, device, 3, "random", 3), normals=False)
    records, counts = S.export_points(out["depth"], lidar, tol=0.0, from_tanh=False)
    clouds, labels = tmp / "clouds", tmp / "labels"
    clouds.mkdir()
    labels.mkdir()
    rng = np.random.default_rng(2)
    rows, labs = [], []
    for b, stem in enumerate(STEMS):
        rec = records[b, :int(counts[b])].cpu().numpy()
        if b == 1:
            rec = rec[: int(0.6 * len(rec))]          # a shorter cloud: the batch is padded
        if b == 2:
            rec = rec[rng.permutation(len(rec))]      # no point order
        rec[:, 3] = np.arange(len(rec), dtype=np.float32)   # the payload: a record's row in its file
        rec.tofile(clouds / f"{stem}.bin")
        lab = rng.integers(0, 2 ** 32, len(rec), dtype=np.uint32)
        lab.astype("<u4").tofile(labels / f"{stem}.label")
        rows.append(rec)
        labs.append(lab)
    assert len({len(r) for r in rows}) == 3 and min(len(r) for r in rows) > 1000
    del G
    return {"tmp": tmp, "argv": argv, "clouds": clouds, "labels": labels, "rows": rows, "labs": labs}


def run(world, save, *extra, model="dusty2"):
    from dusty_gan_amd import transfer_raydrop
    argv = world["argv"][model] + ["--points", str(world["clouds"]), "--labels", str(world["labels"]), "--save-dir-path", str(save),
                                   "--realisations", str(K)] + STEPS + list(extra)
    out_dir = transfer_raydrop.main(argv)
    assert out_dir == os.path.join(str(save), "raydrop")
    return out_dir


@pytest.fixture(scope="module")
def whole_batch(world):
    """the command on the three clouds in one batch (the default batch size), run once"""
    return run(world, world["tmp"] / "whole")


@pytest.mark.parametrize("model", ["dusty1", "dusty2"])
def test_fixed_noise_ties_the_drop_rule_to_the_head_kernel(world, model):
    """keep under the inversion's own fixed noise = the mask the generator's head kernel (dg_head_post_fwd) stored for the same
    target, where a point fell - bit for bit: one mask rule, the channels in the head's order"""
    from dusty_gan_amd import raydrop, utils
    from dusty_gan_amd.datasets.raw import read_clouds
    from dusty_gan_amd.inversion import invert
    argv = world["argv"][model]
    cfg, G, lidar, device = utils.setup(argv[1], argv[3], ema=True, fix_noise=True)
    paths = [world["clouds"] / f"{s}.bin" for s in STEMS]
    rec, counts = read_clouds(paths, lidar.max_depth, device)
    res = raydrop.transfer(G, lidar, rec, counts, noise="fixed", num_step=20)
    depth, valid = lidar.points_to_depth(rec, drop_value=1, tau=2, counts=counts)
    mask = valid.float()
    assert torch.equal(res["target"], depth) and torch.equal(res["valid"], valid)
    ref = invert(G, mask * lidar.invert_depth(depth), mask, num_step=20)
    head = (ref["out"]["mask"] > 0).all(dim=1)                         # [B,H,W]: dusty2's two planes multiply
    assert ref["out"]["mask"].shape[1] == (2 if model == "dusty2" else 1)
    assert torch.equal(ref["out"]["confidence"], res["out"]["confidence"]) and torch.equal(ref["loss"], res["loss"])
    win = res["win"].view(-1, lidar.H, lidar.W)
    assert torch.equal(win >= 0, valid[:, 0])
    keep = res["keep"]
    assert tuple(keep.shape) == (3, 1, lidar.H, lidar.W) and keep.dtype == torch.uint8
    assert torch.equal(keep[:, 0] > 0, head & (win >= 0))
    frac = float(keep.float().mean())
    assert 0.02 < frac < 0.98, frac                                    # (the tie is not between two constant masks)
    assert torch.equal(res["counts"][:, 0].long(), keep.flatten(1).sum(dim=1))
    with pytest.raises(ValueError, match="one realisation"):
        raydrop.transfer(G, lidar, rec, counts, noise="fixed", realisations=2, num_step=20)
    with pytest.raises(ValueError, match="labels"):
        raydrop.transfer(G, lidar, rec, counts, labels=torch.zeros(3, rec.shape[1] - 1, dtype=torch.int64, device=device), num_step=20)


def test_invert_keys_a_scan_by_its_dataset_index(world):
    """invert(first_index=): scan 6 alone draws the initial latent and the perturbations it draws as row 2 of the batch that
    starts at scan 4 (the bound of tests/test_gpu_inversion.py's batch independence: 1e-5; another key moves the latent by
    about the perturbation's strength, 1e-2), and index 0 is the call without the argument, bit for bit"""
    from dusty_gan_amd import utils
    from dusty_gan_amd.datasets.raw import read_clouds
    from dusty_gan_amd.inversion import invert
    argv = world["argv"]["dusty1"]
    _, G, lidar, device = utils.setup(argv[1], argv[3], ema=True, fix_noise=True)
    rec, counts = read_clouds([world["clouds"] / f"{s}.bin" for s in STEMS], lidar.max_depth, device)
    depth, valid = lidar.points_to_depth(rec, drop_value=1, tau=2, counts=counts)
    mask = valid.float()
    ref = mask * lidar.invert_depth(depth)
    batch = invert(G, ref, mask, num_step=6, first_index=4)
    alone = invert(G, ref[2:3], mask[2:3], num_step=6, first_index=6)
    assert float((alone["latent"][0] - batch["latent"][2]).abs().max()) <= 1e-5
    other = invert(G, ref[2:3], mask[2:3], num_step=6)
    assert float((other["latent"][0] - batch["latent"][2]).abs().max()) > 1e-3
    zero = invert(G, ref[2:3], mask[2:3], num_step=6, first_index=0)
    assert torch.equal(zero["latent"], other["latent"]) and torch.equal(zero["loss"], other["loss"])
    with pytest.raises(ValueError, match="first_index"):
        invert(G, ref, mask, num_step=6, first_index=-1)


def read_outputs(out_dir):
    out = {}
    for stem in STEMS:
        for k in range(K):
            rec = np.fromfile(os.path.join(out_dir, "points", f"{stem}_{k}.bin"), np.float32).reshape(-1, 4)
            lab = np.fromfile(os.path.join(out_dir, "labels", f"{stem}_{k}.label"), "<u4")
            out[stem, k] = (rec, lab)
    return out


def test_command_outputs_are_input_records_in_pixel_order(world, whole_batch):
    from dusty_gan_amd import utils
    from dusty_gan_amd.datasets.raw import read_clouds
    out_dir = whole_batch
    assert sorted(os.listdir(out_dir)) == ["labels", "maps", "points", "stats.csv"]
    assert sorted(os.listdir(os.path.join(out_dir, "points"))) == sorted(f"{s}_{k}.bin" for s in STEMS for k in range(K))
    assert sorted(os.listdir(os.path.join(out_dir, "labels"))) == sorted(f"{s}_{k}.label" for s in STEMS for k in range(K))
    assert sorted(os.listdir(os.path.join(out_dir, "maps"))) == [s + ".npy" for s in STEMS]
    outs = read_outputs(out_dir)
    with open(os.path.join(out_dir, "stats.csv"), newline="") as f:
        table = list(csv.reader(f))
    assert table[0] == ["name", "points", "valid_pixels", "kept_0", "kept_1", "drop_rate", "loss"]
    assert [r[0] for r in table[1:]] == STEMS
    argv = world["argv"]["dusty2"]
    _, _, lidar, device = utils.setup(argv[1], argv[3], ema=True, fix_noise=True)
    for b, stem in enumerate(STEMS):
        src, src_lab, row = world["rows"][b], world["labs"][b], table[1 + b]
        maps = np.load(os.path.join(out_dir, "maps", f"{stem}.npy"))
        assert maps.shape == (2 + K, 64, 1024) and maps.dtype == np.float32
        assert int(row[1]) == len(src) and int(row[2]) == len(src)     # every record came from a pixel of its own
        assert (maps[0] == 1.0).sum() >= 64 * 1024 - len(src)          # (1 where no point fell)
        assert ((maps[1] >= 0) & (maps[1] <= 1)).all() and set(np.unique(maps[2:]).tolist()) <= {0.0, 1.0}
        assert (maps[2] != maps[3]).any()                              # two realisations, two masks
        for k in range(K):
            rec, lab = outs[stem, k]
            n = len(rec)
            assert 0 < n < len(src) and int(row[3 + k]) == n == len(lab) == int(maps[2 + k].sum())
            ids = rec[:, 3].astype(np.int64)
            assert len(np.unique(ids)) == n
            assert np.array_equal(R.bits(rec), R.bits(src[ids])), (stem, k)     # an output record IS an input record
            assert np.array_equal(lab, src_lab[ids]), (stem, k)
            # row-major pixel order: the survivors, projected on their own, fall into strictly ascending pixels - the pixels
            # the keep mask of the realisation marks
            path = os.path.join(out_dir, "points", f"{stem}_{k}.bin")
            r_u, cnt = read_clouds([path], lidar.max_depth, device)
            _, _, idx = lidar.points_to_depth(r_u, counts=cnt, return_index=True)
            px = idx[0].cpu().numpy()
            assert (np.diff(px) > 0).all() and np.array_equal(px, np.nonzero(maps[2 + k].reshape(-1))[0]), (stem, k)
        drop = 1.0 - np.mean([int(row[3]), int(row[4])]) / int(row[2])
        assert abs(float(row[5]) - drop) < 1e-12 and np.isfinite(float(row[6]))


def test_files_do_not_depend_on_the_batch(world, whole_batch):
    """the same seed with --batch-size 1 and in one batch of three: identical points/ and labels/ files; a second run of the
    batch reproduces them"""
    one = run(world, world["tmp"] / "one", "--batch-size", "1", "--no-maps")
    again = run(world, world["tmp"] / "again", "--batch-size", "3", "--no-maps")
    assert sorted(os.listdir(one)) == ["labels", "points", "stats.csv"]
    differ = []
    for sub in ("points", "labels"):
        for name in sorted(os.listdir(os.path.join(whole_batch, sub))):
            want = open(os.path.join(whole_batch, sub, name), "rb").read()
            for tag, other in (("batch 1", one), ("second run", again)):
                got = open(os.path.join(other, sub, name), "rb").read()
                if got != want:
                    differ.append((tag, sub, name, len(got), len(want)))
    print("files that differ:", differ)
    assert not differ


def test_another_seed_draws_other_drops(world, whole_batch):
    other = run(world, world["tmp"] / "seed", "--seed", "1", "--batch-size", "3", "--no-maps", "--corruption", "closing")
    a = np.fromfile(os.path.join(other, "points", "sim_a_0.bin"), np.float32)
    assert a.size > 0 and a.size % 4 == 0
    assert a.tobytes() != open(os.path.join(whole_batch, "points", "sim_a_0.bin"), "rb").read()


def test_baseline_checkpoint_is_refused_before_any_gpu_work(tmp_path, world, monkeypatch, capsys):
    from dusty_gan_amd import transfer_raydrop, utils
    argv = make_world(tmp_path, "dcgan_eqlr", "none")
    monkeypatch.setattr(utils, "setup", lambda *a, **k: pytest.fail("the generator was loaded"))
    with pytest.raises(SystemExit) as e:
        transfer_raydrop.main(argv + ["--points", str(world["clouds"]), "--save-dir-path", str(tmp_path)] + STEPS)
    assert e.value.code == 2 and "no measurability head: nothing to transfer" in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "raydrop")
