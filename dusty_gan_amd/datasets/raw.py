"""Raw Velodyne scans -> the files `dataset=kitti_odometry` trains from: the spherical projections read by ScanLoader /
ResidentScans and the angle grid `LiDAR(angle_file=...)` needs.

Reference: process_kitti.py:76-118 (process_point_clouds: one `.bin` -> one 64 x 2048 x 4 `.npy`) and :143-183
(compute_avg_angles -> angles.pt).  There, joblib workers argsort and scatter every scan in Python; here the host threads
only move bytes - ScanLoader's pipeline in reverse - and the arithmetic is three launches per chunk of scans
(`dg_scan_project`, csrc/scan_project.hip) plus one per chunk for the angle sums (`dg_angle_accum`).

The second half of the file does the same for clouds of ANY spinning sensor, whose records come in no order:
`cloud_chunks` reads `.bin` / `.npy` clouds into pinned slots, `project_clouds_beams` / `project_files_beams` give every
point the row of its nearest beam (`dg_beam_project`, csrc/beam_project.hip; the table comes from datasets/beams.py).
"""
import os
import os.path as osp
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import _lib as L

H_RINGS = 64  # the reference hard-codes the last ring's row (process_kitti.py:102)


class RawScanError(L.DgError):
    """a raw scan the reference's script would have raised on; `.names` lists the scans (files)"""

    def __init__(self, names, why="more than 128 ring starts (a ring row below -64, where numpy's index raises)"):
        self.names = list(names)
        super().__init__(why + ": " + ", ".join(str(n) for n in self.names))


def _device(device):
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def _check_offsets(offsets, n_points):
    o = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if o.size < 2 or o[0] != 0 or o[-1] != n_points or np.any(np.diff(o) < 0):
        raise ValueError(f"offsets must ascend from 0 to the number of points ({n_points}); got {o.tolist()[:8]}...")
    return o


def _launch_project(points, offsets, S, W, keys, status, cells, out):
    L.check(L.lib().dg_scan_project(L.ptr(points), L.ptr(offsets), S, H_RINGS, W, L.ptr(keys), L.ptr(status),
                                    L.ptr(cells), L.ptr(out), L.stream_ptr()), "dg_scan_project")


def _results(out, cells, keys):
    """out alone, or the tuple (out[, cells][, keys])"""
    extra = tuple(t for t in (cells, keys) if t is not None)
    return (out,) + extra if extra else out


def project_scans(points, offsets, W=2048, return_cells=False, names=None, device=None, return_keys=False):
    """process_point_clouds (process_kitti.py:76-118) for a batch of raw scans, on the GPU.
    points [N,4] fp32 (tensor or array: the scans' records back to back), offsets [S+1] ints on the host (scan s =
    points[offsets[s]:offsets[s+1]]) -> device tensor [S,64,W,4]: every cell holds its nearest point (float32 depth; on a
    tie the lower point index), zeros where none fell.  return_cells: also every point's row * W + column [N] int32.
    return_keys: also (last) the z-buffer words [S*64*W] int64 as the call left them - every cell's (range bits << 32 | the
    winner's index within its scan) or -1 for an empty cell: what datasets.labels.project_labels reads.
    Raises RawScanError (naming names[s], or the index s) for a scan with a ring row below -64."""
    points = torch.as_tensor(points)
    if not points.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("project_scans runs on the GPU only (no CPU fallback)")
        points = points.to(_device(device))
    assert points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] == 4, (points.dtype, points.shape)
    points = points.contiguous()
    o = _check_offsets(offsets, points.shape[0])
    S, W, dev = o.size - 1, int(W), points.device
    with torch.cuda.device(dev):
        offs = torch.from_numpy(o).to(dev)
        keys = torch.empty(S * H_RINGS * W, dtype=torch.int64, device=dev)
        status = torch.empty(S, dtype=torch.int32, device=dev)
        cells = torch.empty(max(points.shape[0], 1), dtype=torch.int32, device=dev) if return_cells else None
        out = torch.empty(S, H_RINGS, W, 4, dtype=torch.float32, device=dev)
        if points.shape[0] == 0:   # nothing to scatter (and no pointer to hand over)
            out.zero_()
            return _results(out, cells[:0] if return_cells else None, keys.fill_(-1) if return_keys else None)
        _launch_project(points, offs, S, W, keys, status, cells, out)
        bad = torch.nonzero(status).flatten().tolist()
    if bad:
        raise RawScanError([names[s] if names is not None else f"scan {s}" for s in bad])
    return _results(out, cells[:points.shape[0]] if return_cells else None, keys if return_keys else None)


# ------------------------------------------------------------------------------------------------ angle grid
class AngleAccumulator:
    """compute_avg_angles (process_kitti.py:143-183) in chunks: `add` a device batch [S,H,W,C] of projected scans, `finish`
    -> [2,H,W] fp32 (pitch, yaw).  The sums are integers (32.32 fixed point), so the grid does not depend on the chunking."""

    def __init__(self, H, W, device, min_depth=0.9, max_depth=120.0):
        self.H, self.W, self.device = int(H), int(W), torch.device(device)
        self.min_depth, self.max_depth = float(min_depth), float(max_depth)
        self.sums = torch.zeros(2, self.H, self.W, dtype=torch.int64, device=self.device)
        self.count = torch.zeros(self.H, self.W, dtype=torch.int32, device=self.device)
        self.total = 0

    def add(self, scans):
        assert scans.is_cuda and scans.dtype == torch.float32 and scans.dim() == 4 and scans.is_contiguous()
        S, H, W, C = scans.shape
        assert (H, W) == (self.H, self.W), (scans.shape, self.H, self.W)
        if S == 0:
            return
        with torch.cuda.device(self.device):
            L.check(L.lib().dg_angle_accum(L.ptr(scans), S, H, W, C, self.min_depth, self.max_depth, L.ptr(self.sums),
                                           L.ptr(self.count), L.stream_ptr()), "dg_angle_accum")
        self.total += S

    def finish(self):
        if self.total == 0:
            raise ValueError("no scans were added")
        out = torch.empty(2, self.H, self.W, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().dg_angle_finish(L.ptr(self.sums), L.ptr(self.count), self.H, self.W, L.ptr(out),
                                            L.stream_ptr()), "dg_angle_finish")
        if bool(torch.isnan(out).any()):   # `assert angles.isnan().sum() == 0` (process_kitti.py:181)
            raise ValueError("a whole ring or a whole column of the angle grid has no valid pixel in any scan")
        return out


def _npy_header(f):
    """(shape, fortran_order, dtype) of an open .npy file positioned at its payload, or None"""
    try:
        version = np.lib.format.read_magic(f)
        return (np.lib.format.read_array_header_1_0 if version == (1, 0) else np.lib.format.read_array_header_2_0)(f)
    except ValueError:
        return None


def _read_npy_into(path, dst):
    """one projected scan into a pinned slot (ScanLoader._read_into's fast path, with np.load behind it)"""
    with open(path, "rb") as f:
        header = _npy_header(f)
        if header is not None and tuple(header[0]) == dst.shape and header[2] == np.float32 and not header[1]:
            if f.readinto(memoryview(dst).cast("B")) != dst.nbytes:
                raise ValueError(f"{path}: truncated file")
            return
    arr = np.load(path)
    if arr.shape != dst.shape:
        raise ValueError(f"{path}: shape {arr.shape} != {dst.shape}")
    np.copyto(dst, arr, casting="same_kind")


def average_angles(source, min_depth=None, max_depth=None, chunk=16, num_workers=4, device=None):
    """compute_avg_angles (process_kitti.py:143-183) -> [2,H,W] fp32 device tensor (pitch, yaw), over projected scans at
    their own size.  source: a ScanDataset (its datalist and depth range), a list of `.npy` paths, or a tensor [S,H,W,C].
    Host threads read `chunk` files into a pinned slot, one H2D copy per chunk on a side stream, one launch per chunk."""
    chunk = max(1, int(chunk))
    if hasattr(source, "datalist"):
        paths = list(source.datalist)
        min_depth = source.min_depth if min_depth is None else min_depth
        max_depth = source.max_depth if max_depth is None else max_depth
    else:
        paths = source
    min_depth = 0.9 if min_depth is None else min_depth      # KITTIOdometry's defaults, as process_kitti.py:208-212
    max_depth = 120.0 if max_depth is None else max_depth
    if torch.is_tensor(paths) or isinstance(paths, np.ndarray):
        scans = torch.as_tensor(paths)
        dev = scans.device if scans.is_cuda else _device(device)
        assert scans.dim() == 4 and scans.dtype == torch.float32, (scans.shape, scans.dtype)
        acc = AngleAccumulator(scans.shape[1], scans.shape[2], dev, min_depth, max_depth)
        for i in range(0, scans.shape[0], chunk):
            acc.add(scans[i:i + chunk].to(dev).contiguous())
        return acc.finish()
    paths = [os.fspath(p) for p in paths]
    if not paths:
        raise FileNotFoundError("average_angles: no projected scans")
    dev = _device(device)
    shape = tuple(np.load(paths[0], mmap_mode="r").shape)
    if len(shape) != 3 or shape[-1] < 3:
        raise ValueError(f"{paths[0]}: expected a [rings, points, >=3] array, got {shape}")
    acc = AngleAccumulator(shape[0], shape[1], dev, min_depth, max_depth)
    pool = ThreadPoolExecutor(max(1, int(num_workers)))
    copy_stream = torch.cuda.Stream(dev)
    slots = []
    for _ in range(2):
        pinned = torch.empty(chunk, *shape, dtype=torch.float32).pin_memory()
        slots.append({"pinned": pinned, "host": pinned.numpy(), "dev": torch.empty(chunk, *shape, dtype=torch.float32, device=dev),
                      "copied": torch.cuda.Event(), "consumed": None, "futs": [], "n": 0})
    batches = [paths[i:i + chunk] for i in range(0, len(paths), chunk)]

    def submit(s, names):
        s["copied"].synchronize()
        s["futs"] = [pool.submit(_read_npy_into, p, s["host"][j]) for j, p in enumerate(names)]
        s["n"] = len(names)

    try:
        pending, free, nxt = deque(), deque(slots), 0
        while nxt < len(batches) and free:
            s = free.popleft()
            submit(s, batches[nxt])
            pending.append(s)
            nxt += 1
        while pending:
            s = pending.popleft()
            for f in s["futs"]:
                f.result()
            cur = torch.cuda.current_stream(dev)
            with torch.cuda.stream(copy_stream):
                if s["consumed"] is not None:
                    copy_stream.wait_event(s["consumed"])
                s["dev"].copy_(s["pinned"], non_blocking=True)
                s["copied"].record(copy_stream)
            cur.wait_event(s["copied"])
            acc.add(s["dev"][:s["n"]])
            s["consumed"] = torch.cuda.Event()
            s["consumed"].record(cur)
            if nxt < len(batches):
                submit(s, batches[nxt])
                pending.append(s)
                nxt += 1
        return acc.finish()
    finally:
        pool.shutdown(wait=True)


# ------------------------------------------------------------------------------------------------ .bin -> .npy
def write_npy(path, arr):
    """np.save's v1.0 file for a C-ordered float32 array, header then payload straight from the (pinned) buffer; the file
    appears under its name only when complete"""
    tmp = path + ".part"
    with open(tmp, "wb") as f:
        np.lib.format.write_array_header_1_0(f, {"descr": "<f4", "fortran_order": False, "shape": tuple(arr.shape)})
        f.write(memoryview(arr).cast("B"))
    os.replace(tmp, path)


def _read_bin_into(path, dst):
    with open(path, "rb") as f:
        if f.readinto(memoryview(dst).cast("B")) != dst.nbytes:
            raise ValueError(f"{path}: changed size while being read")


def _cloud_rows(path):
    """(rows, columns) of a cloud file: a KITTI `.bin` (N x 4 float32) or a `.npy` of shape N x 3 or N x 4"""
    if path.endswith(".npy"):
        with open(path, "rb") as f:
            header = _npy_header(f)
        if header is None or len(header[0]) != 2 or header[0][1] not in (3, 4):
            raise RawScanError([path], "not an N x 3 or N x 4 .npy array")
        n, cols = int(header[0][0]), int(header[0][1])
    else:
        size = osp.getsize(path)
        if size % 16:
            raise RawScanError([path], f"{size} bytes is not a whole number of (x, y, z, reflectance) float32 records")
        n, cols = size // 16, 4
    if n == 0:
        raise RawScanError([path], "an empty cloud")
    return n, cols


def read_clouds(paths, max_depth, device=None, *, return_raw=False):
    """cloud files -> (records [B,Nmax,4] float32 in UNIT space (metres / max_depth; column 3 as stored, 0 for N x 3 files),
    counts [B] int32) on `device`: what LiDAR.points_to_depth takes with counts=.  A file is a KITTI `.bin` (N x 4
    little-endian float32, metres) or a `.npy` of shape N x 3 or N x 4 (metres).  Clouds shorter than the longest are padded
    with zero records, which points_to_depth does not read.  An empty file, a `.bin` whose size is not a multiple of 16 bytes
    or a `.npy` of another shape raises RawScanError naming the file.  return_raw: a third result, the same records in METRES
    as the files hold them, bit for bit (raydrop.gather copies its output from them: dividing and multiplying back would not
    be exact)."""
    paths = [os.fspath(p) for p in paths]
    if not paths:
        raise FileNotFoundError("read_clouds: no cloud files")
    shapes = [_cloud_rows(p) for p in paths]
    counts = np.array([n for n, _ in shapes], dtype=np.int32)
    records = np.zeros((len(paths), int(counts.max()), 4), dtype=np.float32)
    raw = np.zeros_like(records) if return_raw else None
    for b, (path, (n, cols)) in enumerate(zip(paths, shapes)):
        if not path.endswith(".npy"):
            _read_bin_into(path, records[b, :n])
        elif cols == 4:
            _read_npy_into(path, records[b, :n])
        else:
            xyz = np.empty((n, 3), dtype=np.float32)
            _read_npy_into(path, xyz)
            records[b, :n, :3] = xyz
        if raw is not None:
            raw[b, :n] = records[b, :n]
        records[b, :n, :3] /= np.float32(max_depth)
    dev = _device(device)
    res = (torch.from_numpy(records).to(dev), torch.from_numpy(counts).to(dev))
    return res + (torch.from_numpy(raw).to(dev),) if return_raw else res


class _ProjSlot:
    """one chunk in flight: pinned points / offsets / output, their device twins and the kernels' workspaces"""

    def __init__(self, chunk, W, device):
        self.chunk, self.W, self.device = chunk, W, device
        self.cap = 0
        self.pts_pin = self.pts_dev = None
        self.off_pin = torch.empty(chunk + 1, dtype=torch.int64).pin_memory()
        self.off_dev = torch.empty(chunk + 1, dtype=torch.int64, device=device)
        self.keys = torch.empty(chunk * H_RINGS * W, dtype=torch.int64, device=device)
        self.st_dev = torch.empty(chunk, dtype=torch.int32, device=device)
        self.st_pin = torch.empty(chunk, dtype=torch.int32).pin_memory()
        self.out_dev = torch.empty(chunk, H_RINGS, W, 4, dtype=torch.float32, device=device)
        self.out_pin = torch.empty(chunk, H_RINGS, W, 4, dtype=torch.float32).pin_memory()
        self.out_host = self.out_pin.numpy()
        self.done = torch.cuda.Event()
        self.rfuts, self.wfuts, self.pairs, self.n = [], [], [], 0
        # the label images (project_files(label_pairs=...)): allocated with the first chunk that carries labels
        self.lab_cap, self.lab_pin, self.lab_host, self.lab_dev = 0, None, None, None
        self.sem_dev = self.sem_pin = self.sem_host = self.lst_dev = self.lst_pin = None
        self.label_pairs, self.has_labels = [], False

    def reserve(self, n_points):
        if n_points > self.cap:
            self.cap = int(n_points * 1.25) + 1024
            self.pts_pin = torch.empty(self.cap, 4, dtype=torch.float32).pin_memory()
            self.pts_host = self.pts_pin.numpy()
            self.pts_dev = torch.empty(self.cap, 4, dtype=torch.float32, device=self.device)

    def reserve_labels(self, n_points):
        if self.sem_dev is None:
            self.sem_dev = torch.empty(self.chunk, H_RINGS, self.W, dtype=torch.uint8, device=self.device)
            self.sem_pin = torch.empty(self.chunk, H_RINGS, self.W, dtype=torch.uint8).pin_memory()
            self.sem_host = self.sem_pin.numpy()
            self.lst_dev = torch.empty(self.chunk, dtype=torch.int32, device=self.device)
            self.lst_pin = torch.empty(self.chunk, dtype=torch.int32).pin_memory()
        if n_points > self.lab_cap:
            self.lab_cap = int(n_points * 1.25) + 1024
            self.lab_pin = torch.empty(self.lab_cap, dtype=torch.int32).pin_memory()
            self.lab_host = self.lab_pin.numpy()
            self.lab_dev = torch.empty(self.lab_cap, dtype=torch.int32, device=self.device)


def project_files(pairs, W=2048, chunk=16, num_workers=4, device=None, progress=None, label_pairs=None):
    """[(raw `.bin`, destination `.npy`)] -> the files, `chunk` scans per launch.  ScanLoader's pipeline in reverse: host
    threads read the `.bin` records into a pinned slot, one H2D copy per chunk on a side stream, dg_scan_project, one D2H copy
    into a pinned slot, host threads write v1.0 / C-order / float32 `.npy` files of shape (64, W, 4).  A scan the reference
    would have raised on (RawScanError) is not written; the rest of its chunk is.  Returns the number of files written.
    A destination of None is not written (its label image may still be).
    label_pairs: one entry per pair, None or (SemanticKITTI `.label` of the scan, destination `.png`): the scan's label image
    (datasets.labels; process_kitti.py:120-131) out of the same chunk and the same z-buffer words as its `.npy`, the label
    reads and PNG writes on the same host threads.  A label file of another length than its scan, or an id outside the
    table among the winners, raises RawScanError after the rest is written.  The PNGs are not counted in the result."""
    pairs = [(os.fspath(a), None if b is None else os.fspath(b)) for a, b in pairs]
    if not pairs:
        return 0
    if label_pairs is None:
        label_pairs = [None] * len(pairs)
    label_pairs = [None if lp is None else (os.fspath(lp[0]), os.fspath(lp[1])) for lp in label_pairs]
    if len(label_pairs) != len(pairs):
        raise ValueError(f"{len(label_pairs)} label pairs for {len(pairs)} scans")
    if any(lp is not None for lp in label_pairs):
        from . import labels as LB
    chunk, W, dev = max(1, int(chunk)), int(W), _device(device)
    pool = ThreadPoolExecutor(max(1, int(num_workers)))
    copy_stream = torch.cuda.Stream(dev)
    batches = [(pairs[i:i + chunk], label_pairs[i:i + chunk]) for i in range(0, len(pairs), chunk)]
    free = deque(_ProjSlot(chunk, W, dev) for _ in range(min(3, len(batches))))
    reading, on_gpu, slots = deque(), deque(), list(free)
    made_dirs, written, bad, bad_labels = set(), 0, [], []

    def read_labels_into(path, dst):
        if osp.getsize(path) != dst.nbytes:
            raise RawScanError([path], f"not one uint32 label for each of the scan's {dst.size} points")
        _read_bin_into(path, dst)

    def start_read(s, batch_and_labels):
        batch, lpairs = batch_and_labels
        for f in s.wfuts:   # the slot's previous files are on disk (re-raises a writer's error)
            f.result()
        s.wfuts = []
        sizes = [osp.getsize(src) for src, _ in batch]
        for (src, _), sz in zip(batch, sizes):
            if sz % 16:
                raise ValueError(f"{src}: {sz} bytes is not a whole number of (x, y, z, reflectance) float32 records")
        o = np.concatenate([[0], np.cumsum([sz // 16 for sz in sizes])]).astype(np.int64)
        s.reserve(int(o[-1]))
        s.off_pin[:len(o)] = torch.from_numpy(o)
        s.pairs, s.n, s.npts = batch, len(batch), int(o[-1])
        s.rfuts = [pool.submit(_read_bin_into, src, s.pts_host[o[j]:o[j + 1]]) for j, (src, _) in enumerate(batch)
                   if o[j + 1] > o[j]]
        s.label_pairs, s.has_labels = lpairs, any(lp is not None for lp in lpairs)
        if s.has_labels:
            s.reserve_labels(int(o[-1]))
            for j, lp in enumerate(lpairs):
                if lp is None:
                    s.lab_host[o[j]:o[j + 1]] = 0   # ("unlabeled": in the table; the image is not written)
                elif o[j + 1] > o[j] or osp.getsize(lp[0]):
                    s.rfuts.append(pool.submit(read_labels_into, lp[0], s.lab_host[o[j]:o[j + 1]]))

    def launch(s):
        for f in s.rfuts:
            f.result()
        cur = torch.cuda.current_stream(dev)
        n = s.n
        if s.npts == 0:
            s.out_pin[:n].zero_()
            s.st_pin[:n].zero_()
            if s.has_labels:
                s.sem_pin[:n].zero_()
                s.lst_pin[:n].zero_()
            s.done.record(cur)
            return
        with torch.cuda.stream(copy_stream):
            s.pts_dev[:s.npts].copy_(s.pts_pin[:s.npts], non_blocking=True)
            s.off_dev[:n + 1].copy_(s.off_pin[:n + 1], non_blocking=True)
            if s.has_labels:
                s.lab_dev[:s.npts].copy_(s.lab_pin[:s.npts], non_blocking=True)
            up = torch.cuda.Event()
            up.record(copy_stream)
        cur.wait_event(up)
        with torch.cuda.device(dev):
            _launch_project(s.pts_dev, s.off_dev, n, W, s.keys, s.st_dev, None, s.out_dev)
            if s.has_labels:   # the same chunk, the same keys
                LB.launch_scan_labels(s.keys, s.off_dev, s.lab_dev, LB.device_lut(dev), n, H_RINGS, W, s.sem_dev, None, s.lst_dev[:n])
        ran = torch.cuda.Event()
        ran.record(cur)
        with torch.cuda.stream(copy_stream):
            copy_stream.wait_event(ran)
            s.out_pin[:n].copy_(s.out_dev[:n], non_blocking=True)
            s.st_pin[:n].copy_(s.st_dev[:n], non_blocking=True)
            if s.has_labels:
                s.sem_pin[:n].copy_(s.sem_dev[:n], non_blocking=True)
                s.lst_pin[:n].copy_(s.lst_dev[:n], non_blocking=True)
            s.done.record(copy_stream)

    def submit_write(s, fn, path, arr):
        d = osp.dirname(path)
        if d not in made_dirs:
            os.makedirs(d, exist_ok=True)
            made_dirs.add(d)
        s.wfuts.append(pool.submit(fn, path, arr))

    def start_write(s):
        nonlocal written
        s.done.synchronize()
        status = s.st_pin[:s.n].tolist()
        lstatus = s.lst_pin[:s.n].tolist() if s.has_labels else [0] * s.n
        for j, (src, dst) in enumerate(s.pairs):
            if status[j]:
                bad.append(src)
                continue
            lp = s.label_pairs[j]
            if lp is not None and lstatus[j]:
                ids = LB.read_label_file(lp[0]) & 0xFFFF
                bad_labels.append(f"{lp[0]} (ids {sorted(int(i) for i in np.unique(ids[LB.SEMANTIC_KITTI_LUT[ids] == LB.UNKNOWN]))})")
                lp = None
            if dst is not None:
                submit_write(s, write_npy, dst, s.out_host[j])
                written += 1
            if lp is not None:
                submit_write(s, LB.write_label_png, lp[1], s.sem_host[j])
        if progress is not None:
            progress(s.n)

    try:
        nxt = 0
        while nxt < len(batches) and len(reading) < 2 and free:
            s = free.popleft()
            start_read(s, batches[nxt])
            reading.append(s)
            nxt += 1
        while reading or on_gpu:
            if reading:
                s = reading.popleft()
                launch(s)
                on_gpu.append(s)
            if len(on_gpu) > 1 or not reading:
                s = on_gpu.popleft()
                start_write(s)
                free.append(s)
            if nxt < len(batches) and free:
                s = free.popleft()
                start_read(s, batches[nxt])   # (waits for the slot's writers first)
                reading.append(s)
                nxt += 1
        for s in slots:
            for f in s.wfuts:
                f.result()
    finally:
        pool.shutdown(wait=True)
    if bad:
        raise RawScanError(bad)
    if bad_labels:
        raise RawScanError(bad_labels, "a label id outside the SemanticKITTI table")
    return written


# ------------------------------------------------------------------------------------------------ any sensor: clouds -> .npy
def _read_cloud_into(path, dst, cols):
    """one cloud file (see _cloud_rows) into its [n,4] slice of a pinned slot, metres as stored; column 3 of an N x 3 file is 0"""
    if not path.endswith(".npy"):
        _read_bin_into(path, dst)
    elif cols == 4:
        _read_npy_into(path, dst)
    else:
        xyz = np.empty((dst.shape[0], 3), dtype=np.float32)
        _read_npy_into(path, xyz)
        dst[:, :3] = xyz
        dst[:, 3] = 0.0


class _CloudSlot:
    """one chunk of clouds on its way to the device: pinned records / offsets and their device twins"""

    def __init__(self, chunk, device):
        self.device, self.cap = device, 0
        self.pts_pin = self.pts_host = self.pts_dev = None
        self.off_pin = torch.empty(chunk + 1, dtype=torch.int64).pin_memory()
        self.off_dev = torch.empty(chunk + 1, dtype=torch.int64, device=device)
        self.copied = torch.cuda.Event()   # H2D of this slot finished -> the pinned buffers may be refilled
        self.futs, self.batch, self.npts = [], [], 0

    def reserve(self, n_points):
        if n_points > self.cap or self.pts_dev is None:   # (the first chunk allocates even when it holds no point)
            self.cap = int(n_points * 1.25) + 1024
            self.pts_pin = torch.empty(self.cap, 4, dtype=torch.float32).pin_memory()
            self.pts_host = self.pts_pin.numpy()
            self.pts_dev = torch.empty(self.cap, 4, dtype=torch.float32, device=self.device)


def cloud_chunks(items, chunk=16, num_workers=4, device=None, path_of=None):
    """generator over `items` (cloud files: `.bin` N x 4 or `.npy` N x 3 / N x 4, or anything path_of maps to one), `chunk`
    at a time: yields (points [N,4] fp32, offsets [S+1] int64, the items of the chunk) - device tensors as dg_scan_project
    takes them, valid until the generator is advanced.  Host threads read the next chunk into a pinned slot while the caller
    works on this one; the H2D copies ride the caller's stream.  A file read_clouds would refuse raises RawScanError."""
    items = list(items)
    path_of = os.fspath if path_of is None else path_of
    chunk, dev = max(1, int(chunk)), _device(device)
    batches = [items[i:i + chunk] for i in range(0, len(items), chunk)]
    slots = [_CloudSlot(chunk, dev) for _ in range(min(2, len(batches)))]
    pool = ThreadPoolExecutor(max(1, int(num_workers)))

    def start(s, batch):
        s.copied.synchronize()   # (no-op for a never-recorded event)
        paths = [path_of(it) for it in batch]
        shapes = [_cloud_rows(p) for p in paths]
        o = np.concatenate([[0], np.cumsum([n for n, _ in shapes])]).astype(np.int64)
        s.reserve(int(o[-1]))
        s.off_pin[:len(o)] = torch.from_numpy(o)
        s.batch, s.npts = batch, int(o[-1])
        s.futs = [pool.submit(_read_cloud_into, p, s.pts_host[o[j]:o[j + 1]], cols)
                  for j, (p, (_, cols)) in enumerate(zip(paths, shapes))]

    try:
        if batches:
            start(slots[0], batches[0])
        for k in range(len(batches)):
            s = slots[k % 2]
            if k + 1 < len(batches):
                start(slots[(k + 1) % 2], batches[k + 1])
            for f in s.futs:
                f.result()
            n = len(s.batch)
            s.pts_dev[:s.npts].copy_(s.pts_pin[:s.npts], non_blocking=True)
            s.off_dev[:n + 1].copy_(s.off_pin[:n + 1], non_blocking=True)
            s.copied.record(torch.cuda.current_stream(dev))
            yield s.pts_dev[:s.npts], s.off_dev[:n + 1], s.batch
    finally:
        pool.shutdown(wait=True)


def _beam_table(beams):
    """the table as dg_beam_project reads it: float64 on the host, radians, strictly descending"""
    b = np.ascontiguousarray(np.asarray(beams, dtype=np.float64).reshape(-1))
    if b.size < 1 or not np.all(np.isfinite(b)) or np.any(np.diff(b) >= 0):
        raise ValueError(f"the beam table must hold strictly descending elevations (radians); got {b.tolist()[:8]}...")
    return b


def _launch_beam_project(points, offsets, S, table, W, keys, cells, out):
    L.check(L.lib().dg_beam_project(L.ptr(points), L.ptr(offsets), S, table.ctypes.data, table.size, W, L.ptr(keys),
                                    L.ptr(cells), L.ptr(out), L.stream_ptr()), "dg_beam_project")


def project_clouds_beams(points, offsets, beams, W=2048, return_cells=False, device=None, return_keys=False):
    """project_scans for clouds whose records come in ANY order, from a sensor with the beam table `beams` ([H] elevations in
    radians, strictly descending: estimate_beams' result).  -> device tensor [S,H,W,4]: a point's row is its nearest beam
    (in double; a tie goes to the lower row), its column project_scans' own; every cell holds its nearest point (float32
    range; on a tie the lower point index), zeros where none fell.  A point with a non-finite coordinate takes no part, nor
    does the origin.  return_cells: also every point's row * W + column [N] int32, -1 where it took no part.  return_keys:
    also (last) the z-buffer words [S*H*W] int64 as the call left them, as project_scans returns them."""
    points = torch.as_tensor(points)
    if not points.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("project_clouds_beams runs on the GPU only (no CPU fallback)")
        points = points.to(_device(device))
    assert points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] == 4, (points.dtype, points.shape)
    points = points.contiguous()
    o = _check_offsets(offsets, points.shape[0])
    table = _beam_table(beams)
    S, H, W, dev = o.size - 1, table.size, int(W), points.device
    with torch.cuda.device(dev):
        offs = torch.from_numpy(o).to(dev)
        keys = torch.empty(S * H * W, dtype=torch.int64, device=dev)
        cells = torch.empty(max(points.shape[0], 1), dtype=torch.int32, device=dev) if return_cells else None
        out = torch.empty(S, H, W, 4, dtype=torch.float32, device=dev)
        if points.shape[0] == 0:   # nothing to scatter (and no pointer to hand over)
            out.zero_()
            return _results(out, cells[:0] if return_cells else None, keys.fill_(-1) if return_keys else None)
        _launch_beam_project(points, offs, S, table, W, keys, cells, out)
    return _results(out, cells[:points.shape[0]] if return_cells else None, keys if return_keys else None)


def project_files_beams(pairs, beams, W=2048, chunk=16, num_workers=4, device=None, progress=None, on_chunk=None):
    """project_files for any sensor: [(cloud file, destination `.npy`)] -> the files, (H, W, 4) float32 each, `chunk` clouds
    per dg_beam_project.  Host threads read the clouds (cloud_chunks) and write the `.npy` files; on_chunk(pairs of the
    chunk, their projections [S,H,W,4] on the device) runs before the projections leave the device (the angle grid's
    sums).  Returns the number of files written."""
    pairs = [(os.fspath(a), os.fspath(b)) for a, b in pairs]
    if not pairs:
        return 0
    table = _beam_table(beams)
    chunk, H, W, dev = max(1, int(chunk)), table.size, int(W), _device(device)
    pool = ThreadPoolExecutor(max(1, int(num_workers)))
    copy_stream = torch.cuda.Stream(dev)
    keys = torch.empty(chunk * H * W, dtype=torch.int64, device=dev)
    outs = [{"dev": torch.empty(chunk, H, W, 4, dtype=torch.float32, device=dev),
             "pin": torch.empty(chunk, H, W, 4, dtype=torch.float32).pin_memory(), "done": torch.cuda.Event(),
             "read": None, "wfuts": [], "batch": []} for _ in range(2)]
    made_dirs, written = set(), 0

    def start_write(o):
        nonlocal written
        o["done"].synchronize()
        host = o["pin"].numpy()
        for j, (_, dst) in enumerate(o["batch"]):
            d = osp.dirname(dst)
            if d not in made_dirs:
                os.makedirs(d, exist_ok=True)
                made_dirs.add(d)
            o["wfuts"].append(pool.submit(write_npy, dst, host[j]))
            written += 1
        if progress is not None:
            progress(len(o["batch"]))

    try:
        prev = None
        with torch.cuda.device(dev):
            for k, (pts, offs, batch) in enumerate(cloud_chunks(pairs, chunk, num_workers, dev, path_of=lambda p: p[0])):
                o, n = outs[k % 2], len(batch)
                for f in o["wfuts"]:   # the slot's previous files are on disk (re-raises a writer's error)
                    f.result()
                o["wfuts"], o["batch"] = [], batch
                cur = torch.cuda.current_stream(dev)
                if o["read"] is not None:
                    cur.wait_event(o["read"])   # the slot's previous D2H copy has read `dev`
                _launch_beam_project(pts, offs, n, table, W, keys, None, o["dev"])
                if on_chunk is not None:
                    on_chunk(batch, o["dev"][:n])
                ran = torch.cuda.Event()
                ran.record(cur)
                with torch.cuda.stream(copy_stream):
                    copy_stream.wait_event(ran)
                    o["pin"][:n].copy_(o["dev"][:n], non_blocking=True)
                    o["done"].record(copy_stream)
                o["read"] = o["done"]
                if prev is not None:
                    start_write(prev)
                prev = o
            if prev is not None:
                start_write(prev)
        for o in outs:
            for f in o["wfuts"]:
                f.result()
    finally:
        pool.shutdown(wait=True)
    return written
