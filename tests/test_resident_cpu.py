"""Host-side pieces of the resident scan store (dataset.resident, datasets/resident.py) - no GPU needed: the flip schedule
against ScanLoader's own draws, the shard order, the position -> (epoch, slab, parity) map and the flip tables an accumulated
step reads across an epoch boundary, the size estimate and the refusal, and the config default."""
import types

import numpy as np
import pytest
import torch

from dusty_gan_amd.datasets import resident as R
from dusty_gan_amd.datasets.scans import ScanLoader, sampler_indices


class _Done:
    def synchronize(self):
        pass


def _loader_flips(seed, rank, epoch, nslab, B, skip=0):
    """the flips ScanLoader.__iter__ draws for batches skip.. of `epoch`: its own _submit on stand-in slots (no files, no GPU)"""
    me = types.SimpleNamespace(B=B, dataset=types.SimpleNamespace(flip=True), _read_into=None,
                               pool=types.SimpleNamespace(submit=lambda *a: None))
    rng = np.random.default_rng([seed, rank, epoch])   # (ScanLoader.__iter__'s generator and its skip loop)
    for _ in range(skip):
        rng.random(B)
    out = []
    for _ in range(skip, nslab):
        slot = types.SimpleNamespace(copied=_Done(), host=[None] * B)
        ScanLoader._submit(me, slot, list(range(B)), rng)
        out.append(slot.flip.numpy())
    return np.stack(out)


@pytest.mark.parametrize("seed,rank,epoch,skip", [(0, 0, 0, 0), (0, 1, 2, 0), (3, 0, 5, 2), (0, 3, 1, 4), (7, 2, 0, 1)])
def test_flip_schedule_is_the_loaders(seed, rank, epoch, skip):
    nslab, B = 6, 5
    want = _loader_flips(seed, rank, epoch, nslab, B, skip)
    got = R.flip_schedule(seed, rank, epoch, nslab, B)
    assert got.dtype == np.uint8 and got.shape == (nslab, B)
    assert np.array_equal(got[skip:], want)
    assert 0 < got.sum() < got.size
    assert not np.array_equal(R.flip_schedule(seed, rank, epoch + 1, nslab, B), got)   # flips change per epoch


@pytest.mark.parametrize("n,world,B", [(11, 1, 3), (11, 2, 3), (12, 2, 2), (7, 3, 2), (40, 2, 4)])
def test_shard_order_is_the_samplers(n, world, B):
    for rank in range(world):
        order, nslab = R.shard_order(n, world, rank, B)
        full = sampler_indices(n, world, rank, 0, 0, True)
        me = types.SimpleNamespace(dataset=[0] * n, world=world, rank=rank, B=B, drop_last=True)
        assert nslab == ScanLoader.__len__(me)
        assert order == full[:nslab * B]
        # slab k of any epoch is ScanLoader's batch k
        for k in range(nslab):
            assert order[k * B:(k + 1) * B] == full[k * B:(k + 1) * B]


def test_position_and_flip_tables_across_an_epoch_boundary():
    nslab, B = 3, 4
    assert [R.position(n, nslab) for n in range(7)] == [(0, 0, 0), (0, 1, 0), (0, 2, 0), (1, 0, 1), (1, 1, 1), (1, 2, 1),
                                                        (2, 0, 0)]
    ld = object.__new__(R.ResidentScanLoader)
    ld.seed, ld.rank, ld.nslab, ld.B, ld.flip = 0, 0, nslab, B, True
    ld._flips, ld._tab = {}, [None, None]
    ld.flip_dev = torch.full((2, nslab * B), 9, dtype=torch.uint8)   # (host stand-in for the device tables)

    def device_flips(ctr):   # what DgFetch's resident form reads for batch number ctr
        e, slab, par = R.position(ctr, nslab)
        return ld.flip_dev[par, slab * B:(slab + 1) * B].numpy()
    n_acc = 2
    for first in range(0, 12, n_acc):   # steps of two micro-batches: 2-3 and 8-9 straddle a boundary
        ld.ensure_tables(first, first + n_acc - 1)
        for ctr in range(first, first + n_acc):
            e, slab, _ = R.position(ctr, nslab)
            assert np.array_equal(device_flips(ctr), R.flip_schedule(0, 0, e, nslab, B)[slab]), (first, ctr)
    assert ld._tab == [2, 3]   # (batches 10-11: epoch 3; epoch 2 written for batches 6-7)
    with pytest.raises(ValueError):
        ld.ensure_tables(2, 2 + 4)   # five micro-batches over three epochs: two tables cannot hold them


def test_size_estimate_and_refusal(monkeypatch):
    assert R.resident_bytes(100, 64, 1024, False) == 100 * 64 * 1024 * 4
    assert R.resident_bytes(100, 64, 1024, True) == 2 * 100 * 64 * 1024 * 4 + 2 * 100
    # the KITTI train split at 64 x 1024 with both flip variants: ~10 GB at world 1
    assert 10.0e9 < R.resident_bytes(19130, 64, 1024, True) < 10.1e9
    assert R.resident_budget(1.5) == 1_500_000_000
    R.check_budget(10, 10)
    with pytest.raises(R.ResidentBudgetError, match="needs 11 bytes but 10 bytes are available"):
        R.check_budget(11, 10)

    # the loader refuses before it allocates or reads anything
    def boom(*a, **k):
        raise AssertionError("allocated or read before the budget check")
    monkeypatch.setattr(R.torch, "empty", boom)
    monkeypatch.setattr(R.torch, "zeros", boom)
    monkeypatch.setattr(R, "ScanLoader", boom)
    class DS:
        shape, flip, min_depth, max_depth, root, split = (32, 256), True, 0.9, 120.0, "r", "train"

        def __len__(self):
            return 10
    ds = DS()
    need = R.resident_bytes(9, 32, 256, True)   # 10 scans, B = 3 -> 3 batches of 3
    with pytest.raises(R.ResidentBudgetError) as ei:
        R.ResidentScanLoader(ds, 3, "cpu", max_gb=(need - 1) / 1e9)
    assert f"needs {need} bytes but {need - 1} bytes are available" in str(ei.value)


def test_mask_is_derivable_from_the_stored_depth():
    """valid -> d > min -> d - min >= ulp(min) -> stored depth >= ulp(min) / (max - min) > 0 (no underflow) for the shipped
    limits; limits where it could underflow are refused"""
    for lo, hi in ((0.9, 120.0), (0.5, 80.0), (1e-3, 1e4)):
        R._check_mask_derivable(lo, hi)
        lo32, rng32 = np.float32(lo), np.float32(hi - lo)
        d = np.nextafter(lo32, np.float32(np.inf))           # the smallest valid range
        assert d > lo32 and (d - lo32) / rng32 > 0
    for lo, hi in ((0.0, 120.0), (1e-38, 1e3), (5.0, 5.0)):
        with pytest.raises(ValueError):
            R._check_mask_derivable(lo, hi)


def test_resident_defaults_to_off():
    from dusty_gan_amd.utils.config import load_config
    for name in ("kitti_odometry", "sparse_mpo"):
        cfg = load_config([f"dataset={name}"])
        assert cfg.dataset.resident is False and cfg.dataset.get("resident_max_gb") is None
        assert load_config([f"dataset={name}", "dataset.resident=true"]).dataset.resident is True
    # configs saved before the key existed
    assert load_config(["dataset=synthetic"]).dataset.get("resident", False) is False
