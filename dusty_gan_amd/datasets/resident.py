"""A file dataset's training shard kept in HBM (`dataset.resident: true`): read once, then every batch is picked and converted
on the device by the training step's first launch.

Why the shard fits and stays fixed: the reference never calls `set_epoch` (ScanLoader.__iter__ always takes
`sampler_indices(..., epoch=0)`), so a rank sees one fixed shard of the split in one fixed order every epoch; only the
per-sample flips change.  The store keeps that order, cut to the loader's `len * B` samples (drop_last): batch k of any epoch
is the contiguous slab [k B, (k + 1) B) and no index table is needed.  (Reshuffling per epoch would break this layout.)

Layout: `store` [nvar, nslab B, H, W] fp32, the polar depth exactly as `dg_scan_to_polar` makes it for the file loader;
variant 1 (present when `dataset.flip`) is the horizontally flipped scan - the flip precedes the NEAREST resize
(datasets/kitti.py:73-75), so the two variants read different source columns and both are stored.  No mask is stored: the
loader's mask is `valid ? 1 : 0` and its depth `valid ? (d - min) / (max - min) : 0` with valid implying d > min, so
d - min >= ulp(min) > 0 and the quotient is at least ulp(min) / (max - min); `_check_mask_derivable` refuses depth limits
for which that could underflow to zero.  Then depth > 0 <=> valid, and `mask = depth > 0` is the loader's mask bit for bit
(the build checks it on every stored sample as well).

Flips: epoch e's flips are the loader's draws, `np.random.default_rng([seed, rank, e])`, B per batch in order.  The device
keeps two per-sample flip tables, chosen by epoch parity; the host writes an epoch's table with a stream-ordered copy before
the first step that reads it (`ensure_tables`), never during a capture.
"""
import time
from collections import deque
from collections.abc import Mapping

import numpy as np
import torch

from .. import _lib as L
from .scans import ScanLoader, sampler_indices

BUDGET_FRACTION = 0.8   # default budget: this fraction of the device's free memory (torch.cuda.mem_get_info)


class ResidentBudgetError(MemoryError):
    pass


def shard_order(n, world, rank, B, seed=0, shuffle=True):
    """the rank's samples in sampler order, cut to whole batches: (indices, batches per epoch)"""
    idx = sampler_indices(n, world, rank, seed, 0, shuffle)
    nslab = len(idx) // B
    return idx[:nslab * B], nslab


def flip_schedule(seed, rank, epoch, nslab, B):
    """[nslab, B] uint8: the flips ScanLoader draws in `epoch` (its `skip` discards the leading batches' draws, so the rows
    from `skip` on are what a resumed loader draws)"""
    rng = np.random.default_rng([seed, rank, epoch])
    return np.stack([(rng.random(B) > 0.5).astype(np.uint8) for _ in range(nslab)]) if nslab else np.zeros((0, B), np.uint8)


def position(n, nslab):
    """batch number n of the run (batches drawn before it) -> (epoch, slab, flip-table parity)"""
    e = n // nslab
    return e, n % nslab, e & 1


def resident_bytes(nsamples, H, W, flip):
    """device bytes of a store of `nsamples` samples at H x W: the depth images of every variant and the two flip tables"""
    nvar = 2 if flip else 1
    return nvar * nsamples * H * W * 4 + (2 * nsamples if flip else 0)


def resident_budget(max_gb=None, device=None):
    """bytes a store may take: `dataset.resident_max_gb` (1 GB = 1e9 bytes), else BUDGET_FRACTION of the free memory"""
    if max_gb is not None:
        return int(float(max_gb) * 1e9)
    free, _total = torch.cuda.mem_get_info(device)
    return int(free * BUDGET_FRACTION)


def check_budget(need, avail):
    if need > avail:
        raise ResidentBudgetError(f"resident scan store needs {need} bytes but {avail} bytes are available "
                                  "(dataset.resident_max_gb, or a fraction of the free device memory); "
                                  "set dataset.resident=false to read the scans from files")


def _check_mask_derivable(min_depth, max_depth):
    """the smallest stored depth of a valid cell, ulp(min) / (max - min) in fp32, must be a normal float (see above)"""
    lo, hi = np.float32(min_depth), np.float32(max_depth)
    rng = np.float32(max_depth - min_depth)
    if not (lo > 0 and hi > lo) or np.spacing(lo) / rng < np.finfo(np.float32).tiny:
        raise ValueError(f"dataset.resident needs 0 < min_depth < max_depth, far enough apart in scale that the stored depth "
                         f"of every valid cell is a normal float > 0; got {min_depth}, {max_depth}")


class ResidentBatch(Mapping):
    """{"depth", "mask"} [B,1,H,W] of batch `slab` in `epoch`, gathered from the store by one launch on first access.  The
    training step never touches it (it reads the store by the device counter), so drawing a batch costs no launch."""

    def __init__(self, loader, epoch, slab):
        self.loader, self.epoch, self.slab, self._out = loader, epoch, slab, None

    def _get(self):
        if self._out is None:
            self._out = self.loader.gather(self.epoch, self.slab)
        return self._out

    def __getitem__(self, k):
        return self._get()[k]

    def __iter__(self):
        return iter(("depth", "mask"))

    def __len__(self):
        return 2


class ResidentScanLoader:
    """ScanLoader's surface (`len`, one epoch per `iter`, `epoch` / `skip`, `graph_safe`) over a store built once in HBM.
    `iter` yields ResidentBatch objects; a batch materialised by `batch["depth"]` equals ScanLoader's (torch.equal)."""
    graph_safe = True

    def __init__(self, dataset, batch_size, device, world=1, rank=0, num_workers=4, seed=0, shuffle=True, max_gb=None):
        if len(dataset) == 0:
            raise FileNotFoundError(f"no scans under {dataset.root} for split '{dataset.split}'")
        self.dataset, self.B, self.device = dataset, int(batch_size), torch.device(device)
        self.world, self.rank, self.seed, self.shuffle = world, rank, seed, shuffle
        self.order, self.nslab = shard_order(len(dataset), world, rank, self.B, seed, shuffle)
        if self.nslab == 0:
            raise ValueError(f"the shard of rank {rank} holds fewer than one batch of {self.B} scans")
        self.H, self.W = (int(v) for v in dataset.shape)
        self.flip = bool(dataset.flip)
        self.nvar = 2 if self.flip else 1
        # everything is checked before anything is allocated
        self.nbytes = resident_bytes(len(self.order), self.H, self.W, self.flip)
        check_budget(self.nbytes, resident_budget(max_gb, self.device))
        _check_mask_derivable(dataset.min_depth, dataset.max_depth)
        self.epoch = 0
        self.skip = 0
        self._flips = {}            # epoch -> host flip schedule (the few most recent)
        self._tab = [None, None]    # epoch whose flips each device table holds
        self.store = torch.empty(self.nvar, len(self.order), self.H, self.W, dtype=torch.float32, device=self.device)
        self.flip_dev = (torch.zeros(2, len(self.order), dtype=torch.uint8, device=self.device) if self.flip else None)
        self._build(num_workers)

    # ---------------------------------------------------------------- build
    def _build(self, num_workers):
        """read the shard once with ScanLoader's machinery (thread pool, pinned slots, the .npy fast path, the float64
        fallback, the shape checks) and convert each batch with dg_scan_to_polar into both variants"""
        t0 = time.perf_counter()
        reader = ScanLoader(self.dataset, self.B, self.device, world=self.world, rank=self.rank, num_workers=num_workers,
                            prefetch=2, seed=self.seed, shuffle=self.shuffle)
        ds, B, HW = self.dataset, self.B, self.H * self.W
        flat = self.store.view(self.nvar, -1, HW)
        mask = torch.empty(B, HW, dtype=torch.float32, device=self.device)
        ones = torch.ones(B, dtype=torch.uint8, device=self.device)
        bad = torch.zeros((), dtype=torch.int64, device=self.device)
        batches = [self.order[i:i + B] for i in range(0, len(self.order), B)]

        def submit(s, idxs):
            s.copied.synchronize()
            s.futs = [reader.pool.submit(reader._read_into, s.host[j], i) for j, i in enumerate(idxs)]
        pending, free, nxt = deque(), deque(reader.slots), 0
        while nxt < len(batches) and free:
            s = free.popleft()
            submit(s, batches[nxt])
            s.k = nxt
            pending.append(s)
            nxt += 1
        try:
            while pending:
                s = pending.popleft()
                for f in s.futs:
                    f.result()  # re-raises reader errors here
                cur = torch.cuda.current_stream(self.device)
                with torch.cuda.stream(reader.copy_stream):
                    if s.consumed is not None:
                        reader.copy_stream.wait_event(s.consumed)
                    s.dev.copy_(s.pinned, non_blocking=True)
                    s.copied.record(reader.copy_stream)
                cur.wait_event(s.copied)
                Hs, Ws, C = reader.scan_shape
                for v in range(self.nvar):
                    pol = flat[v, s.k * B:(s.k + 1) * B]
                    L.check(L.lib().dg_scan_to_polar(L.ptr(s.dev), B, Hs, Ws, C, self.H, self.W,
                                                     L.ptr(ones) if v else None, float(ds.min_depth), float(ds.max_depth),
                                                     0.0, L.ptr(pol), L.ptr(mask), None, None, L.stream_ptr()),
                            "dg_scan_to_polar")
                    bad += (mask != (pol > 0).float()).sum()
                s.consumed = torch.cuda.Event()
                s.consumed.record(cur)
                if nxt < len(batches):
                    submit(s, batches[nxt])
                    s.k = nxt
                    pending.append(s)
                    nxt += 1
            nbad = int(bad)   # (synchronises: the build is complete)
        finally:
            reader.pool.shutdown(wait=True)
            reader.slots = []
        if nbad:
            raise RuntimeError(f"resident store: {nbad} cells where the mask is not depth > 0")
        Hs, Ws, C = reader.scan_shape
        self.build_seconds = time.perf_counter() - t0
        self.raw_bytes = len(self.order) * Hs * Ws * C * 4

    # ---------------------------------------------------------------- epochs and flips
    def __len__(self):
        return self.nslab

    def __iter__(self):
        e = self.epoch
        self.epoch += 1
        first, self.skip = min(self.skip, self.nslab), 0
        for k in range(first, self.nslab):
            yield ResidentBatch(self, e, k)

    def flips(self, epoch):
        """epoch's flips [nslab B] uint8 (host), as ScanLoader draws them (none without dataset.flip)"""
        if not self.flip:
            return np.zeros(self.nslab * self.B, np.uint8)
        f = self._flips.get(epoch)
        if f is None:
            f = flip_schedule(self.seed, self.rank, epoch, self.nslab, self.B).reshape(-1)
            if len(self._flips) >= 4:
                self._flips.pop(min(self._flips))
            self._flips[epoch] = f
        return f

    def _load(self, epoch):
        if self.flip_dev is None or self._tab[epoch & 1] == epoch:
            return
        if self.flip_dev.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("resident flip table written during a capture")
        # (a copy from pageable memory: ordered on the current stream behind every launch that read the old table)
        self.flip_dev[epoch & 1].copy_(torch.from_numpy(self.flips(epoch)))
        self._tab[epoch & 1] = epoch

    def ensure_tables(self, first, last):
        """the flip tables for batch numbers first..last (one step's micro-batches), written before the step is launched"""
        e0, e1 = first // self.nslab, last // self.nslab
        if e1 - e0 > 1:
            raise ValueError(f"a step of {last - first + 1} micro-batches spans more than two epochs of {self.nslab} batches")
        for e in range(e0, e1 + 1):
            self._load(e)

    # ---------------------------------------------------------------- device reads
    def gather(self, epoch, slab):
        """batch `slab` of `epoch` as ScanLoader yields it (one launch, dg_resident_gather)"""
        self._load(epoch)
        f32 = dict(dtype=torch.float32, device=self.device)
        out = {"depth": torch.empty(self.B, 1, self.H, self.W, **f32), "mask": torch.empty(self.B, 1, self.H, self.W, **f32)}
        flip = None if self.flip_dev is None else self.flip_dev[epoch & 1, slab * self.B:]
        L.check(L.lib().dg_resident_gather(L.ptr(self.store), self.nslab, self.B, self.H * self.W, slab, L.ptr(flip),
                                           L.ptr(out["depth"]), L.ptr(out["mask"]), L.stream_ptr()), "dg_resident_gather")
        return out

    def prologue_eligible(self):
        return (self.H * self.W) % (1024 * L.XSUM_PARTS) == 0

    def fetch_job(self, lidar, ctr, drop_const):
        """fetch_reals of batch number *ctr as a job of the step's first launch (DgFetch's resident form): (DgFetch, out,
        parts), or None where the prologue form does not apply"""
        if not self.prologue_eligible():
            return None
        out = torch.empty(self.B, 1, self.H, self.W, dtype=torch.float32, device=self.device)
        parts = torch.empty(self.B, L.XSUM_PARTS, dtype=torch.float32, device=self.device)
        f = L.DgFetch()
        f.pol, f.mask, f.pool_ctr, f.npool = L.ptr(self.store), None, L.ptr(ctr), 0
        f.min_depth, f.max_depth, f.drop_const = lidar.min_depth, lidar.max_depth, float(drop_const)
        f.B, f.HW, f.out, f.parts = self.B, self.H * self.W, L.ptr(out), L.ptr(parts)
        f.nslab, f.flip_tab = self.nslab, L.ptr(self.flip_dev)
        return f, out, parts

    def fetch_reals_pool(self, lidar, ctr, drop_const):
        """fetch_reals of batch number *ctr as a launch of its own (dg_fetch_reals_resident_sum), sums into the open arena;
        None unless the arena is open and H W % 256 == 0"""
        HW = self.H * self.W
        sums = L.AccArena.take(self.B, self.device) if HW % 256 == 0 else None
        if sums is None:
            return None
        out = torch.empty(self.B, 1, self.H, self.W, dtype=torch.float32, device=self.device)
        L.check(L.lib().dg_fetch_reals_resident_sum(L.ptr(self.store), L.ptr(ctr), self.nslab, L.ptr(self.flip_dev),
                                                    lidar.min_depth, lidar.max_depth, float(drop_const), self.B, HW,
                                                    L.ptr(out), L.ptr(sums), L.stream_ptr()), "dg_fetch_reals_resident_sum")
        return L.tag_sums(out, sums)
