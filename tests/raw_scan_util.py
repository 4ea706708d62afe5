"""Helpers shared by the raw-scan tests and tests/golden/make_raw_scan_golden.py: reading tests/golden/raw_scan.npz and
the EXCLUDED SET of a fixture scan - the cells where the GPU projection may legitimately differ from the reference's.

Everything here is computed from the fixture's inputs and recorded reference results alone, never from the code under test.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raw_scan.npz")
H = 64
BAND_SPACINGS = 4      # float32 spacings of W around an integer column coordinate
EXCLUDED_CAP = 0.01    # of a scan's non-empty cells


def load():
    return np.load(GOLDEN)


def scan_names(g):
    return [str(n) for n in g["meta/scans"]]


def scan(g, name):
    """(points [N,4] f32, W, reference winner index per cell [64,W] (-1 = empty), reference row [N] (as the reference
    computed it: negative for the wrapped rings), reference column [N])"""
    p = f"scan/{name}/"
    return (g[p + "points"], int(g[p + "W"]), g[p + "winner"].astype(np.int64), g[p + "row"].astype(np.int64),
            g[p + "col"].astype(np.int64))


def expected_image(points, winner):
    """the reference's projection [64,W,4] rebuilt from the winner indices"""
    out = np.zeros(winner.shape + (4,), dtype=np.float32)
    out[winner >= 0] = points[winner[winner >= 0]]
    return out


def depth32(points):
    """np.linalg.norm(xyz, ord=2, axis=1) in float32, as process_kitti.py:85"""
    return np.linalg.norm(points[:, :3], ord=2, axis=1)


def excluded_cells(points, W, winner, row, col):
    """bool [64,W]: the cells of
      (a) points whose column coordinate, in float64, lies within BAND_SPACINGS float32 spacings of W of an integer - a 1-ulp
          difference between two float32 atan2 moves such a point to the neighbouring column: its reference cell and both
          columns either side of that integer are excluded;
      (b) points whose float32 depth ties with the winner of their cell (the reference's argsort leaves the order open).
    Also returns the number of points in (a) and in (b)."""
    x, y = points[:, 0].astype(np.float64), points[:, 1].astype(np.float64)
    g = ((-np.arctan2(y, x) / np.pi + 1.0) / 2.0 % 1.0) * W
    k = np.rint(g)
    band = np.abs(g - k) <= BAND_SPACINGS * float(np.spacing(np.float32(W)))
    r = row % H
    ex = np.zeros((H, W), dtype=bool)
    kb = k[band].astype(np.int64)
    ex[r[band], col[band]] = True
    ex[r[band], kb % W] = True
    ex[r[band], (kb - 1) % W] = True
    d = depth32(points)
    win_at = winner[r, col]                       # the winner of each point's cell
    tie = (win_at != np.arange(len(points))) & (d == d[win_at])
    ex[r[tie], col[tie]] = True
    return ex, int(band.sum()), int(tie.sum())


def check_cap(points, W, winner, row, col):
    """the condition the parity test rests on: the excluded set is at most EXCLUDED_CAP of the scan's non-empty cells and no
    point ties with a winner.  Returns (excluded cells, non-empty cells)."""
    ex, _, n_tie = excluded_cells(points, W, winner, row, col)
    filled = int((winner >= 0).sum())
    assert n_tie == 0, f"{n_tie} points tie in depth with the winner of their cell"
    assert ex.sum() <= EXCLUDED_CAP * filled, (int(ex.sum()), filled)
    return int(ex.sum()), filled
