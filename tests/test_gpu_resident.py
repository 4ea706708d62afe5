"""The resident scan store (dataset.resident: true, datasets/resident.py) against the file loader it replaces: batches, the
fetch the step's first launch makes, whole training runs (graph replay, accumulation, resume) bit for bit."""
import numpy as np
import pytest
import torch

from tests.test_gpu_data import write_kitti_tree

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _pair(root, shape, flip, B, world=1, rank=0):
    from dusty_gan_amd.datasets import KITTIOdometry, ResidentScanLoader, ScanLoader
    ds = KITTIOdometry(root, "train", shape=shape, flip=flip)
    return (ScanLoader(ds, B, DEV, world=world, rank=rank, num_workers=2),
            ResidentScanLoader(ds, B, DEV, world=world, rank=rank, num_workers=2))


@pytest.mark.parametrize("Hs,Ws,shape", [(32, 512, (32, 256)), (8, 64, (8, 32))])
@pytest.mark.parametrize("flip", [False, True])
def test_resident_batches_equal_the_file_loaders(tmp_path, Hs, Ws, shape, flip):
    """world 1 and 2, every rank; B = 3 does not divide any shard; three epochs; the tree holds float64 files (the loader's
    generic path); a prologue-eligible and an ineligible shape"""
    write_kitti_tree(str(tmp_path), Hs, Ws, {0: 7, 1: 4})   # 11 train scans, file 1 of each sequence in float64
    for world in (1, 2):
        for rank in range(world):
            fl, rl = _pair(str(tmp_path), shape, flip, 3, world, rank)
            assert len(rl) == len(fl) and rl.store.shape[0] == (2 if flip else 1)
            assert rl.prologue_eligible() == (shape == (32, 256))
            flipped = 0
            for epoch in range(3):
                got, want = list(rl), list(fl)
                assert len(got) == len(want) == len(fl)
                for g, w in zip(got, want):
                    assert set(g) == {"depth", "mask"}
                    assert torch.equal(g["depth"], w["depth"]), (world, rank, epoch)
                    assert torch.equal(g["mask"], w["mask"]), (world, rank, epoch)
                flipped += sum(int(f) for f in rl.flips(epoch))
            assert (flipped > 0) == flip
            # resumed mid-epoch: both loaders skip the same batches and keep their flips aligned
            fl.epoch = rl.epoch = 4
            fl.skip = rl.skip = 1
            for g, w in zip(list(rl), list(fl)):
                assert torch.equal(g["depth"], w["depth"]) and torch.equal(g["mask"], w["mask"])


def test_resident_fetch_equals_the_file_paths_fetch(tmp_path):
    """the prologue job's x_real and partial sums (DgFetch, resident form) and the standalone summing fetch
    (dg_fetch_reals_resident_sum) equal the file path's on the same batch - counters in epochs 0..3, both parities"""
    from dusty_gan_amd import _lib as L
    from dusty_gan_amd.utils.lidar import LiDAR
    write_kitti_tree(str(tmp_path), 32, 512, {0: 7, 1: 4})
    fl, rl = _pair(str(tmp_path), (32, 256), True, 3)
    lidar = LiDAR(32, 256, 0.9, 120.0)
    epochs = [list(fl) for _ in range(4)]
    nb = len(rl)
    for n in (0, 2, nb, nb + 1, 2 * nb + 2, 3 * nb):
        e, k = n // nb, n % nb
        w = epochs[e][k]
        ctr = torch.full((1,), n, dtype=torch.int64, device=DEV)
        rl.ensure_tables(n, n)
        job = rl.fetch_job(lidar, ctr, -1.0)
        ref = lidar.fetch_job(w["depth"], w["mask"], None, -1.0)
        L.step_prologue([], [], fetch=job[0])
        L.step_prologue([], [], fetch=ref[0])
        assert torch.equal(job[1], ref[1]) and torch.equal(job[2], ref[2]), n
        L.AccArena.begin(DEV)
        x = rl.fetch_reals_pool(lidar, ctr, -1.0)
        sums = L.AccArena.take(3, DEV)
        out = torch.empty_like(w["depth"])
        L.check(L.lib().dg_fetch_reals_sum(L.ptr(w["depth"]), L.ptr(w["mask"]), 0.9, 120.0, -1.0, 3, 32 * 256, L.ptr(out),
                                           L.ptr(sums), L.stream_ptr()), "dg_fetch_reals_sum")
        assert torch.equal(x, out) and torch.equal(L.tagged_sums(x), sums), n
        L.AccArena.buf = None
    torch.cuda.synchronize()


def _cfg(root, n_acc, resident, resume=None, extra=()):
    from dusty_gan_amd.utils.config import load_config
    c = load_config(["model=dcgan_eqlr", "dataset=kitti_odometry", f"dataset.root={root}", "dataset.shape=[32,256]",
                     "dataset.flip=true", f"dataset.resident={str(resident).lower()}", "model.gen.in_ch=8",
                     "model.gen.ch_base=4", "model.gen.ch_max=16", "model.dis.ch_base=4", "model.dis.ch_max=16",
                     f"solver.batch_size={4 * n_acc}", f"solver.num_accumulation={n_acc}", "enable_amp=false", *extra])
    c.resume = resume
    return c


def _trainer(root, n_acc, resident, resume=None, seed=7):
    from dusty_gan_amd.trainers.dcgan_amp import Trainer
    torch.manual_seed(seed)
    return Trainer(_cfg(root, n_acc, resident, resume), {"gpu": 0, "ngpus": 1, "batch_size": 4, "num_workers": 2})


def _same(a, b):
    for net in ("G", "D", "G_ema"):
        fa, fb = getattr(a, net).store.flat, getattr(b, net).store.flat
        assert torch.equal(fa, fb), (net, float((fa - fb).abs().max()))


def _device_index(tr):
    from dusty_gan_amd import _lib as L
    with L.Counters.bind(tr.counters):
        L.Counters.flush_if(tr._pool_ctr)
    return int(tr._pool_ctr)


@pytest.mark.parametrize("n_acc", [1, 2])
def test_resident_run_is_bit_identical_to_the_file_run(tmp_path, monkeypatch, n_acc):
    """12 scans, B = 4: 3 batches per epoch, 8 steps through warm-up, capture and replay, over several epoch boundaries
    (with 2 micro-batches per step some steps straddle one).  The resident trainer replays with no static batch copy."""
    monkeypatch.setenv("DUSTY_GAN_GRAPH", "1")
    write_kitti_tree(str(tmp_path), 32, 512, {0: 7, 1: 5})
    f = _trainer(str(tmp_path), n_acc, False)
    r = _trainer(str(tmp_path), n_acc, True)
    assert r._pooled() and len(r._scan_loader) == 3
    for i in range(8):
        sf, sr = dict(f.step(i).items()), dict(r.step(i).items())
        assert sf == sr, (i, sf, sr)
    _same(f, r)
    assert r._graph is not None and not hasattr(r, "_g_pol") and not hasattr(r, "_g_mask")
    assert _device_index(r) == r.batches_drawn == f.batches_drawn == 8 * n_acc
    # another consumer draws a batch: the next replay fetches behind it, as the file path does
    f._next_batch()
    r._next_batch()
    for i in range(8, 10):
        assert dict(f.step(i).items()) == dict(r.step(i).items()), i
    _same(f, r)
    assert _device_index(r) == r.batches_drawn == 10 * n_acc + 1
    # the reference's `fetch_reals(next(loader))` on the resident loader is the file loader's
    xf, mf = f.fetch_reals(next(f.loader))
    xr, mr = r.fetch_reals(next(r.loader))
    assert torch.equal(xf, xr) and torch.equal(mf, mr)


def test_resident_resume_mid_epoch(tmp_path, monkeypatch):
    """a resident run checkpointed mid-epoch and resumed equals the uninterrupted one; so does a file-loader checkpoint
    resumed on the resident path"""
    monkeypatch.setenv("DUSTY_GAN_GRAPH", "1")
    root = str(tmp_path / "data")
    write_kitti_tree(root, 32, 512, {0: 7, 1: 5})
    a = _trainer(root, 1, True)
    sa = [dict(a.step(i).items()) for i in range(8)]
    for resident_writer in (True, False):
        b = _trainer(root, 1, resident_writer)
        for i in range(4):   # batch 4 of 3 per epoch: epoch 1, slab 1
            b.step(i)
        path = b.save_models(f"mid{int(resident_writer)}", 4 * 4, directory=str(tmp_path))
        c = _trainer(root, 1, True, resume=path, seed=999)
        assert c.batches_drawn == 4 and c._scan_loader.epoch == 1 and c._scan_loader.skip == 1
        sc = [dict(c.step(i).items()) for i in range(4, 8)]
        assert sc == sa[4:], resident_writer
        _same(a, c)


def test_resident_refuses_over_budget_before_allocating(tmp_path):
    from dusty_gan_amd.datasets import KITTIOdometry, ResidentScanLoader
    from dusty_gan_amd.datasets.resident import ResidentBudgetError, resident_bytes
    write_kitti_tree(str(tmp_path), 32, 512, {0: 7, 1: 5})
    ds = KITTIOdometry(str(tmp_path), "train", shape=(32, 256), flip=True)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    need = resident_bytes(12, 32, 256, True)
    with pytest.raises(ResidentBudgetError, match=f"needs {need} bytes"):
        ResidentScanLoader(ds, 4, DEV, max_gb=need / 2 / 1e9)
    assert torch.cuda.memory_allocated() == before
    ld = ResidentScanLoader(ds, 4, DEV, max_gb=need / 1e9)
    assert ld.nbytes == need and ld.store.numel() * 4 + ld.flip_dev.numel() == need
    assert ld.raw_bytes == 12 * 32 * 512 * 4 * 4 and ld.build_seconds > 0
    assert np.isfinite(float(ld.store.sum()))
