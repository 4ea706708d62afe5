"""A float64 / numpy restatement of the beam-table projection (csrc/beam_project.hip) and a synthetic spinning sensor to feed
it: the per-point elevation and range, the histogram bin, the nearest-beam row, the cell winner.  The column is the float64
expression of tests/raw_scan_util.py with its band (a point inside the band may land one column over in float32).

Everything here is computed from the inputs alone, never from the code under test.  `near_*` report the points a last-bit
difference between two evaluations of atan2 could move across a discontinuity; the tests use seeds for which those lists are
empty (tests/test_beams_cpu.py asserts it), so no case is ever excluded on the GPU.

DEFECT SWITCHES (`defect=`): "tie_upper" lets the UPPER index win ties (cell and row), "ascending" numbers the rows from the
lowest beam.  `self_check` must fail under either - that is what tests/test_beams_cpu.py holds this file to.
"""
import numpy as np

from tests import raw_scan_util as U

EDGE = 1e-9   # radians


def xyz64(points):
    p = np.asarray(points, dtype=np.float32)
    return p[:, 0].astype(np.float64), p[:, 1].astype(np.float64), p[:, 2].astype(np.float64)


def elevation(points):
    """u = atan2(z, sqrt(x^2 + y^2)) in double on the float32 coordinates (csrc/points_body.h)"""
    x, y, z = xyz64(points)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.arctan2(z, np.sqrt(x * x + y * y))


def range64(points):
    x, y, z = xyz64(points)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt((x * x + y * y) + z * z)


def takes_part(points):
    """finite coordinates and not the origin"""
    d = range64(points)
    with np.errstate(invalid="ignore"):
        return np.isfinite(np.asarray(points, dtype=np.float32)[:, :3]).all(1) & (d > 0)


def histogram(points, min_depth, max_depth, lo, hi, NB):
    """int64 [NB]: the points with min_depth < d < max_depth and lo <= u < hi, by floor((u - lo) * (NB / (hi - lo)))"""
    u, d = elevation(points), range64(points)
    with np.errstate(invalid="ignore"):
        ok = takes_part(points) & (d > min_depth) & (d < max_depth) & (u >= lo) & (u < hi)
    b = np.minimum(np.floor((u[ok] - lo) * (NB / (hi - lo))).astype(np.int64), NB - 1)
    return np.bincount(b, minlength=NB).astype(np.int64)


def near_bin_edge(points, min_depth, max_depth, lo, hi, NB):
    """indices of the counted points within EDGE of a bin edge (lo and hi included)"""
    u, d = elevation(points), range64(points)
    with np.errstate(invalid="ignore"):
        ok = takes_part(points) & (d > min_depth) & (d < max_depth) & (u >= lo - EDGE) & (u < hi + EDGE)
    f = (u - lo) * (NB / (hi - lo))
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(ok & (np.abs(f - np.rint(f)) * ((hi - lo) / NB) <= EDGE))


def nearest_beam(u, beams, defect=None):
    """the row of the beam nearest to u (beams descending: row 0 is the highest); an exact tie goes to the LOWER row"""
    b = np.asarray(beams, dtype=np.float64)
    if defect == "ascending":
        b = b[::-1]
    dist = np.abs(b[None, :] - np.asarray(u, dtype=np.float64)[:, None])
    if defect == "tie_upper":
        return (len(b) - 1 - np.argmin(dist[:, ::-1], axis=1)).astype(np.int64)
    return np.argmin(dist, axis=1).astype(np.int64)


def near_midpoint(points, beams):
    """indices of the points within EDGE of the midpoint between two neighbouring beams"""
    b = np.asarray(beams, dtype=np.float64)
    if len(b) < 2:
        return np.zeros(0, dtype=np.int64)
    u = elevation(points)
    mids = (b[:-1] + b[1:]) / 2
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(takes_part(points) & (np.abs(u[:, None] - mids[None, :]).min(1) <= EDGE))


def column_coordinate(points, W):
    x, y, _ = xyz64(points)
    with np.errstate(invalid="ignore"):
        return ((-np.arctan2(y, x) / np.pi + 1.0) / 2.0 % 1.0) * W   # raw_scan_util.excluded_cells' expression


def near_column_edge(points, W):
    """indices of the points inside raw_scan_util's band around an integer column coordinate"""
    g = column_coordinate(points, W)
    with np.errstate(invalid="ignore"):
        band = np.abs(g - np.rint(g)) <= U.BAND_SPACINGS * float(np.spacing(np.float32(W)))
    return np.flatnonzero(takes_part(points) & band)


def project(points, beams, W, defect=None):
    """-> (image [H,W,4] float32, cell [N] int64): every cell holds the nearest of its points by the float32-rounded range,
    the LOWER index on a tie, zeros where none fell; cell = row * W + column, -1 for a point that takes no part"""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 4)
    H = len(beams)
    image = np.zeros((H, W, 4), dtype=np.float32)
    cell = np.full(len(points), -1, dtype=np.int64)
    idx = np.flatnonzero(takes_part(points))
    if idx.size == 0:
        return image, cell
    row = nearest_beam(elevation(points[idx]), beams, defect)
    col = np.floor(column_coordinate(points[idx], W)).astype(np.int64) % W
    cell[idx] = row * W + col
    d32 = range64(points[idx]).astype(np.float32)
    order = np.lexsort((-idx if defect == "tie_upper" else idx, d32))[::-1]   # far to near; of equals the loser first
    winner = np.full(H * W, -1, dtype=np.int64)
    for i, c in zip(idx[order], cell[idx][order]):   # later writes win
        winner[c] = i
    flat = image.reshape(-1, 4)
    flat[winner >= 0] = points[winner[winner >= 0]]
    return image, cell


def synthetic_sensor(beams, W0, seed, jitter=0.0, drop=0.0, r_lo=2.0, r_hi=80.0, shuffle=True, yaw_jitter=0.2):
    """a spinning sensor's cloud [N,4] float32: one return per (beam, azimuth step) but for a `drop` share of them, at the
    step's centre (+- yaw_jitter steps), the beam's elevation (+- 0.98 jitter rad, so float32 rounding stays inside jitter)
    and a random range; records in beam-major order, or shuffled"""
    rng = np.random.default_rng(seed)
    b = np.asarray(beams, dtype=np.float64)
    H = len(b)
    el = b[:, None] + rng.uniform(-0.98, 0.98, (H, W0)) * jitter
    az = -np.pi + (np.arange(W0)[None, :] + 0.5 + rng.uniform(-yaw_jitter, yaw_jitter, (H, W0))) * (2 * np.pi / W0)
    r = rng.uniform(r_lo, r_hi, (H, W0))
    pts = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), rng.random((H, W0))], -1)
    pts = pts.reshape(-1, 4)[rng.random(H * W0) >= drop].astype(np.float32)
    return pts[rng.permutation(len(pts))] if shuffle else pts


def uniform_beams(H, up_deg=3.0, down_deg=-25.0):
    return np.deg2rad(np.linspace(up_deg, down_deg, H))


GPU_CASES = {   # name -> (H, W, W0, [seed per cloud], drop): the clouds tests/test_gpu_beam_project.py projects
    "5x16": (5, 16, 32, [101, 102, 103], 0.1),
    "32x64": (32, 64, 128, [201, 202, 203], 0.1),
    "64x2048": (64, 2048, 2048, [301], 0.08),
}
HIST_CLOUDS = [(0, 401), (700, 402), (5000, 403)]   # (points, seed) of the histogram test's clouds


def gpu_case(name):
    """(beams, W, clouds): 28 degrees of equally spaced beams, elevation jitter 0.15 of their spacing"""
    H, W, W0, seeds, drop = GPU_CASES[name]
    beams = uniform_beams(H)
    jitter = 0.15 * np.deg2rad(28.0) / max(H - 1, 1)
    return beams, W, [synthetic_sensor(beams, W0, seed, jitter=jitter, drop=drop) for seed in seeds]


def hist_clouds():
    """clouds of 0, 700 and 5000 points with elevations all over [-pi/2, pi/2] and ranges either side of the depth limits;
    the non-empty ones also hold a point exactly at each depth limit (0.9 is no float32: the limits used are 1 and 120), a NaN,
    an infinite coordinate and the origin"""
    out = []
    for n, seed in HIST_CLOUDS:
        rng = np.random.default_rng(seed)
        el, az = rng.uniform(-1.55, 1.55, n), rng.uniform(-np.pi, np.pi, n)
        r = np.exp(rng.uniform(np.log(0.3), np.log(200.0), n))
        pts = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), rng.random(n)],
                       -1).astype(np.float32).reshape(-1, 4)
        if n:
            pts[:6] = [[1, 0, 0, 1], [0, 120, 0, 1], [np.nan, 1, 1, 1], [1, np.inf, 1, 1], [1, 1, -np.inf, 1], [0, 0, 0, 1]]
        out.append(pts)
    return out


def self_check(defect=None):
    """hand-made cases with known answers; AssertionError under either defect switch"""
    a = 0.1
    beams = np.array([a, -a])
    W = 8
    yaw = -np.pi + 2.5 * (2 * np.pi / W)          # the middle of column 5: (-yaw / pi + 1) / 2 * 8 = 5.5
    ray = np.array([np.cos(yaw), np.sin(yaw)])

    def pt(r, z, refl):
        return [r * ray[0], r * ray[1], z, refl]
    # row 0 is the highest beam
    pts = np.array([pt(10.0, 10.0 * np.tan(a), 1.0), pt(10.0, -10.0 * np.tan(a), 2.0)], dtype=np.float32)
    _, cell = project(pts, beams, W, defect)
    assert cell.tolist() == [0 * W + 5, 1 * W + 5], cell
    # z = 0 lies exactly between the beams at +-a: the lower row
    pts = np.array([pt(10.0, 0.0, 1.0)], dtype=np.float32)
    _, cell = project(pts, beams, W, defect)
    assert cell.tolist() == [5], cell
    # two points of one cell with the same float32 range: the lower index
    pts = np.array([pt(10.0, 10.0 * np.tan(a), 1.0), pt(10.0, 10.0 * np.tan(a), 2.0)], dtype=np.float32)
    image, _ = project(pts, beams, W, defect)
    assert image[0, 5, 3] == 1.0, image[0, 5]
