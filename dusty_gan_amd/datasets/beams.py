"""The beam table of a spinning LiDAR, estimated from its own clouds: what `process_clouds` needs before it
can give every point a row.  The reference holds no code for it - its rows come from KITTI's file order.

`elevation_histogram` counts the elevations of a dataset's points on the GPU (`dg_elev_hist`, csrc/beam_project.hip: integer
counts, added chunk by chunk); `estimate_beams` turns the few thousand counts into H elevations in float64 numpy on the host.
"""
import os

import numpy as np
import torch

from .. import _lib as L
from .raw import _check_offsets, _device, cloud_chunks

NB_DEFAULT = 8192   # over +-pi/2: 0.022 degrees per bin, an order below any sensor's beam spacing


def _add_hist(points, offsets, S, min_depth, max_depth, lo, hi, hist):
    L.check(L.lib().dg_elev_hist(L.ptr(points), L.ptr(offsets), S, float(min_depth), float(max_depth), float(lo), float(hi),
                                 hist.numel(), L.ptr(hist), L.stream_ptr()), "dg_elev_hist")


def elevation_histogram(source, min_depth=0.9, max_depth=120.0, lo=-np.pi / 2, hi=np.pi / 2, NB=NB_DEFAULT, chunk=16,
                        num_workers=4, device=None):
    """-> int64 numpy array [NB]: the number of points with min_depth < |xyz| < max_depth (metres, both strict) whose elevation
    atan2(z, |xy|) lies in bin k of [lo, hi), over all the clouds of `source`: a list of cloud files (`.bin` N x 4, `.npy` N x 3
    / N x 4; read `chunk` at a time by host threads that only move bytes), a tensor / array [N,4], or (points [N,4], offsets
    [S+1]).  Non-finite points and the origin are not counted.  The counts do not depend on the chunking."""
    NB = int(NB)
    if not (float(lo) < float(hi)) or not 64 <= NB <= 16384:
        raise ValueError(f"elevation_histogram: lo < hi and 64 <= NB <= 16384 are required (lo={lo}, hi={hi}, NB={NB})")
    files = isinstance(source, (list, tuple)) and (len(source) == 0 or isinstance(source[0], (str, os.PathLike)))
    if files:
        if not source:
            raise FileNotFoundError("elevation_histogram: no cloud files")
        dev = _device(device)
    else:
        points, offsets = source if isinstance(source, (list, tuple)) else (source, None)
        points = torch.as_tensor(points)
        if not points.is_cuda:
            if not torch.cuda.is_available():
                raise RuntimeError("elevation_histogram runs on the GPU only (no CPU fallback)")
            points = points.to(_device(device))
        assert points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] == 4, (points.dtype, points.shape)
        points, dev = points.contiguous(), points.device
        o = _check_offsets([0, points.shape[0]] if offsets is None else offsets, points.shape[0])
    with torch.cuda.device(dev):
        hist = torch.zeros(NB, dtype=torch.int64, device=dev)   # (the kernel's u64 words: counts stay far below 2^63)
        if files:
            for pts, offs, batch in cloud_chunks(source, chunk, num_workers, dev):
                _add_hist(pts, offs, len(batch), min_depth, max_depth, lo, hi, hist)
        elif points.shape[0] > 0:
            _add_hist(points, torch.from_numpy(o).to(dev), o.size - 1, min_depth, max_depth, lo, hi, hist)
        return hist.cpu().numpy()


def bin_centres(NB, lo=-np.pi / 2, hi=np.pi / 2):
    return lo + (np.arange(int(NB), dtype=np.float64) + 0.5) * ((hi - lo) / int(NB))


def _mass_quantile(hist, centres, q):
    """the centre of the bin in which the cumulative mass reaches q of the total"""
    c = np.cumsum(hist)
    return centres[min(int(np.searchsorted(c, q * c[-1], side="left")), len(hist) - 1)]


def _assign(centres_sorted, x):
    """the nearest of the ascending centres for every x; an x on a midpoint goes to the lower one"""
    return np.searchsorted((centres_sorted[:-1] + centres_sorted[1:]) / 2, x, side="left")


def _kmeans(w, x, H):
    """1-D Lloyd on the populated bin centres x (ascending) with weights w: centres start at the equal-mass quantiles
    (i + 0.5) / H and move to their cluster's weighted mean until no bin changes cluster (at most 200 sweeps)"""
    c = np.cumsum(w)
    centres = x[np.minimum(np.searchsorted(c, (np.arange(H) + 0.5) / H * c[-1], side="left"), len(x) - 1)].astype(np.float64)
    label = None
    for _ in range(200):
        if np.any(np.diff(centres) <= 0):
            raise ValueError(f"estimate_beams: a cluster ended empty (two of the {H} centres coincide) - the clouds show fewer "
                             f"than {H} beams")
        new = _assign(centres, x)
        mass = np.bincount(new, weights=w, minlength=H)
        if np.any(mass == 0):
            raise ValueError(f"estimate_beams: a cluster ended empty - the clouds show fewer than {H} beams")
        if label is not None and np.array_equal(new, label):
            break
        label = new
        centres = np.bincount(new, weights=w * x, minlength=H) / mass
    return centres


def estimate_beams(hist, H, lo=-np.pi / 2, hi=np.pi / 2, method="kmeans", fov_up=None, fov_down=None):
    """an elevation histogram (elevation_histogram's; bin k covers lo + [k, k + 1) (hi - lo) / NB) -> the sensor's beam table:
    H elevations in RADIANS, strictly descending (row 0 = the highest beam, as in the KITTI files), float64.
      "kmeans"   1-D Lloyd on the weighted bin centres from equal-mass quantile starts: the table the clouds themselves show
      "uniform"  H equally spaced elevations from fov_up down to fov_down (DEGREES; not given: the 99.9 % and 0.1 % mass
                 quantiles) - the RangeNet++ convention
      a path     a text file of H elevations in degrees, one per line: the datasheet's table
    ValueError: a cluster ends empty, the histogram has fewer than H populated bins, or the table is not strictly monotonic
    once sorted."""
    hist = np.asarray(hist, dtype=np.float64).reshape(-1)
    H = int(H)
    if H < 1 or not (float(lo) < float(hi)) or hist.size < 1 or np.any(hist < 0):
        raise ValueError(f"estimate_beams: H >= 1, lo < hi and a non-negative histogram are required (H={H}, lo={lo}, hi={hi})")
    centres = bin_centres(hist.size, lo, hi)
    full = hist > 0
    if method == "kmeans":
        if int(full.sum()) < H:
            raise ValueError(f"estimate_beams: the histogram has {int(full.sum())} populated bins, fewer than {H} beams")
        table = _kmeans(hist[full], centres[full], H)
    elif method == "uniform":
        if (fov_up is None or fov_down is None) and not full.any():
            raise ValueError("estimate_beams: an empty histogram has no field of view")
        up = np.deg2rad(fov_up) if fov_up is not None else _mass_quantile(hist, centres, 0.999)
        down = np.deg2rad(fov_down) if fov_down is not None else _mass_quantile(hist, centres, 0.001)
        table = np.linspace(float(up), float(down), H) if H > 1 else np.array([(float(up) + float(down)) / 2])
    else:
        path = os.fspath(method)
        if not os.path.isfile(path):
            raise ValueError(f"estimate_beams: method must be 'kmeans', 'uniform' or a table file; {path!r} is none of them")
        table = np.deg2rad(np.loadtxt(path, dtype=np.float64, ndmin=1).reshape(-1))
        if table.size != H:
            raise ValueError(f"{path}: {table.size} elevations, expected {H}")
    table = np.sort(np.asarray(table, dtype=np.float64))[::-1].copy()
    if not np.all(np.isfinite(table)) or np.any(np.diff(table) >= 0):
        raise ValueError(f"estimate_beams: the table is not strictly monotonic: {np.rad2deg(table).tolist()}")
    return table


def beam_shares(hist, beams, lo=-np.pi / 2, hi=np.pi / 2):
    """each beam's share of the histogram's points (every bin goes to the beam nearest to its centre), in the table's order:
    a share far from 1 / H is how a wrong H shows"""
    hist = np.asarray(hist, dtype=np.float64).reshape(-1)
    asc = np.asarray(beams, dtype=np.float64)[::-1]
    mass = np.bincount(_assign(asc, bin_centres(hist.size, lo, hi)), weights=hist, minlength=asc.size)
    return (mass / max(hist.sum(), 1.0))[::-1].copy()
