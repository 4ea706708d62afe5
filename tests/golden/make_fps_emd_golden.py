"""Generate tests/golden/fps_emd.npz from the REFERENCE's own device kernels, run on an MI355X.

Needs only oracle/_ref/libref_fps_emd.so (oracle/Makefile.ref: the reference's furthest_point_sampling.cu and
earth_mover_distance.cu, hipified and compiled for gfx950 with the compiler's defaults) and a GPU; one process:
    python tests/golden/make_fps_emd_golden.py [out.npz]
Every reference call is made TWICE on fresh buffers and the file is written only if all pairs of results are
bit-identical (the FPS kernel reads dists_i[0] with no barrier before the next iteration overwrites it, so its
determinism on 64-lane waves is observed here, not assumed).

FPS cases: B = 3 clouds each, m = min(n, 48), n in RUNGS (every block size 1..512 of the reference's launcher, n no
multiple of the block, n > 2 * 512).  Three families:
    lattice_n<n>  integer coordinates * 2^-k, no point at the origin, every squared norm > 1e-3: every product and sum is
                  exact in float32, fused or not, and exact distance ties are everywhere -> isolates the TIE ORDER.
                  cloud 0: draws with replacement from a 5^3 lattice (ties between threads); cloud 1: the first T points
                  repeated with period T = block size (tied duplicates in the SAME thread, where n > T); cloud 2: a 13^3
                  grid in raster order (symmetric ties).
    thresh_n<n>   a tight cluster far from the origin plus, at seeded positions, points whose squared norm is EXACTLY
                  float32(1e-3), its lower / upper float32 neighbour, or 0 - the origin-skip threshold `mag <= 1e-3`
                  (double literal).  The neighbours come from one non-zero coordinate c with fl(c*c) = target (mag is one
                  exact product, fused or not).  float32(1e-3) itself is NOT the rounded square of any float32 (c*c steps
                  by two ulps there and misses it), so it is built from coordinates (a, b, c) * 2^-17 with a, b, c < 4096
                  and a^2 + b^2 < 2^24: the three squares and the first sum are exact and the last sum is rounded once,
                  fused or not; the neighbours get such points too.
                  Near the origin these points are the far ones, so the first picks are decided by the threshold.
    scan_n<n>     tests.test_gpu_metrics.lidar_like_clouds: dropped returns at the origin, one exact duplicate.
thresh and scan clouds are kept only for seeds whose selection is CONTRACTION-INDEPENDENT: furthest point sampling is
replayed in float64 and at every step the winner must lead the best strictly smaller candidate by > 1e-5 relative
(float32 rounding, fused or not, moves a distance by < 1e-6 relative); candidates at exactly the winner's distance must be
coordinate-identical points (a tie, decided by the tie order), and no other squared norm may lie within 1e-5 relative of
the threshold.  Seeds are searched until every n has one; the reference's picks must then be the float64 replay's.

EMD cases (paired clouds [b,n,3] / [b,m,3], scan-like unless stated):
    p<n>_<m>      (1,1) (2,3) (4,4) (64,64) (96,32) (50,150) (100,30) (520,1030) (1030,520), b = 2: integer and truncated
                  n/m factors both ways, the 512-thread and 1024-point chunk edges
    b35_8_8       b = 35: the 32-block grid stride
    far_96_32     two clouds 100 apart: every exponential underflows, the 1e-9 guards decide all levels but the last
    self_64       a cloud paired with itself
    mat64         3 x 4 clouds of 64 points: all twelve pairs, run paired (a[i] against b[j])
Per case: ref = the reference's cost (float32), f64 = oracle.metrics_oracle.emd_cost(dtype=float64), e_ref = |ref - f64|.

Contents:  meta/made_by, meta/device, meta/torch, meta/hip, meta/fps_cases, meta/emd_cases (names)
           fps/<name>/xyz [3,n,3] f32, idx [3,m] i32, seed [3]         emd/<name>/a, b, ref, f64, e_ref
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import metrics_oracle as MO  # noqa: E402
from tests.ref_fps_emd_util import RefFpsEmd  # noqa: E402
from tests.test_gpu_metrics import lidar_like_clouds  # noqa: E402

RUNGS = [1, 2, 3, 5, 8, 17, 33, 70, 130, 300, 513, 1000, 1025, 2048]
EMD_PAIRS = [(1, 1), (2, 3), (4, 4), (64, 64), (96, 32), (50, 150), (100, 30), (520, 1030), (1030, 520)]
THRESH = np.float32(1e-3)
TARGETS = [np.nextafter(THRESH, np.float32(0)), THRESH, np.nextafter(THRESH, np.float32(1))]
MARGIN = 1e-5


def twice(fn, *args):
    r1, r2 = fn(*args), fn(*args)
    if not np.array_equal(r1, r2):
        raise SystemExit("the reference's kernel returned two different results for the same input: not written")
    return r1


# ---------------------------------------------------------------------------------------------- FPS clouds
def fps_f64(xyz, m):
    """furthest point sampling of one cloud replayed in float64 -> (idx, decided, contraction_independent);
    decided[j] is False where every remaining candidate is at distance 0 (all picked already: the tie order alone chooses)"""
    x = xyz.astype(np.float64)
    n = x.shape[0]
    mag32 = (xyz[:, 0] * xyz[:, 0] + xyz[:, 1] * xyz[:, 1]) + xyz[:, 2] * xyz[:, 2]
    mag64 = (x * x).sum(1)
    cand = mag32.astype(np.float64) > 1e-3
    exact = np.isin(mag32, np.array(TARGETS + [np.float32(0)]))  # built to be exact: see the module docstring
    if (np.abs(mag64[~exact] - 1e-3) <= MARGIN * 1e-3).any():
        return None, None, False
    temp = np.full(n, 1e10)
    idx, decided = np.zeros(m, np.int64), np.ones(m, bool)
    old = 0
    for j in range(1, m):
        temp = np.minimum(temp, ((x - x[old]) ** 2).sum(1))
        if not cand.any():
            old = 0
        else:
            t = np.where(cand, temp, -1.0)
            old = int(np.argmax(t))
            v1 = t[old]
            if v1 > 0.0:
                tied = np.flatnonzero(t == v1)
                if not (xyz[tied] == xyz[old]).all():
                    return None, None, False
                rest = t[(t < v1) & cand]
                if rest.size and v1 - rest.max() <= MARGIN * v1:
                    return None, None, False
            else:
                decided[j] = False
        idx[j] = old
    return idx, decided, True


def lattice_clouds(n, rng):
    T = MO.opt_n_threads(n)
    c0 = rng.integers(-2, 3, (n, 3))
    c0[(c0 == 0).all(1)] = (1, -2, 0)
    a = c0.astype(np.float32) * np.float32(2.0 ** -2)            # norms^2 >= 1/16
    c1 = rng.integers(-3, 4, (T, 3))
    c1[(c1 == 0).all(1)] = (0, 3, -1)
    b = c1[np.arange(n) % T].astype(np.float32) * np.float32(2.0 ** -3)   # norms^2 >= 1/64
    g = np.stack(np.meshgrid(*[np.arange(-6, 7)] * 3, indexing="ij"), -1).reshape(-1, 3)
    g = g[~(g == 0).all(1)][:n]
    c = g.astype(np.float32) * np.float32(2.0 ** -4)             # norms^2 >= 1/256
    out = np.stack([a, b, c])
    assert (((out.astype(np.float64)) ** 2).sum(-1) > 2e-3).all()
    return out


def special_points():
    """pool of points whose float32 squared norm is exactly a target -> (points [P,3], target index [P]: 0 lower
    neighbour, 1 float32(1e-3), 2 upper neighbour, 3 the origin); the two constructions of the module docstring, in
    every axis assignment and sign"""
    pts, cls = [], []
    s = np.float32(2.0 ** -17)
    for ti, t in enumerate(TARGETS):
        c = np.float32(math.sqrt(float(t)))
        for _ in range(64):
            c = np.nextafter(c, np.float32(0))
        singles = []
        for _ in range(128):
            c = np.nextafter(c, np.float32(1))
            if np.float32(c * c) == t:
                singles.append(c)
        reps = []   # (a, b, c) * 2^-17 with a^2 + b^2 < 2^24 (exact partial sum) and a^2 + b^2 + c^2 rounding to t
        N0 = int(round(float(t) * 2.0 ** 34))
        for a in range(2100, 2900, 7):
            for b in range(a + 1, 2900):
                if a * a + b * b >= 2 ** 24 or len(reps) >= 6:
                    break
                for N in (N0 - 1, N0, N0 + 1):
                    c2 = N - a * a - b * b
                    c = math.isqrt(c2) if c2 >= 0 else -1
                    if c >= 0 and c * c == c2 and c < 4096:
                        x, y, z = np.float32(a) * s, np.float32(b) * s, np.float32(c) * s
                        if np.float32(np.float32(np.float32(x * x) + np.float32(y * y)) + np.float32(z * z)) == t:
                            reps.append((x, y, z))
                            break
        assert len(reps) >= 3 and (singles or ti == 1), (ti, len(singles), len(reps))
        for c in singles[:2]:
            for ax in range(3):
                for sg in (1, -1):
                    v = [0, 0, 0]
                    v[ax] = sg * c
                    pts.append(v)
                    cls.append(ti)
        for x, y, z in reps:
            for sx in (1, -1):
                for sy in (1, -1):
                    pts.append([sx * x, sy * y, z])      # the order x, y, z is kept: x^2 + y^2 is the exact partial sum
                    cls.append(ti)
    pts.append([0, 0, 0])
    cls.append(3)
    return np.array(pts, np.float32), np.array(cls)


SPECIAL = special_points()


def thresh_cloud(n, seed, b):
    """one cloud: the cluster plus k special points, every target class present as soon as k >= 4"""
    rng = np.random.default_rng(seed)
    sp, cls = SPECIAL
    pts = (np.array([0.5, 0.1, -0.2]) + rng.uniform(-0.05, 0.05, (n, 3))).astype(np.float32)
    k = min(9, max(1, 2 * n // 3))
    want = np.roll(np.array([1, 0, 2, 3, 1, 0, 2, 1, 3]), -b)[:k]    # float32(1e-3) itself first
    pos = rng.choice(n, size=k, replace=False)
    if b == 1:
        pos[0] = 0 if 0 not in pos[1:] else pos[0]   # a threshold / skipped point FIRST: idx[0] = 0 is taken whatever it is
    for p_, c in zip(pos, want):
        pts[p_] = sp[rng.choice(np.flatnonzero(cls == c))]
    return pts


def scan_cloud(n, seed, b):
    return lidar_like_clouds(1, n, seed=seed)[0]


def searched(make, n, m, what):
    """three clouds, each from the first seed whose selection is contraction-independent"""
    clouds, seeds, sel, decs = [], [], [], []
    for b in range(3):
        for seed in range(10000 * n + 1000 * b, 10000 * n + 1000 * b + 1000):
            c = make(n, seed, b)
            idx, dec, ok = fps_f64(c, m)
            if ok:
                break
        else:
            raise SystemExit(f"no contraction-independent seed for {what} n={n} cloud {b}")
        clouds.append(c), seeds.append(seed), sel.append(idx), decs.append(dec)
    return np.stack(clouds), np.array(seeds, np.int64), (np.stack(sel), np.stack(decs))


# ---------------------------------------------------------------------------------------------- main
def main(out_path):
    assert torch.cuda.is_available()
    ref = RefFpsEmd.open()
    assert ref is not None, "build oracle/_ref/libref_fps_emd.so first (make -f oracle/Makefile.ref)"
    d = {"meta/made_by": "tests/golden/make_fps_emd_golden.py: the reference's furthest_point_sampling.cu and "
                         "earth_mover_distance.cu, hipified and built for gfx950 (oracle/Makefile.ref), run twice per case",
         "meta/device": torch.cuda.get_device_name(0), "meta/torch": torch.__version__, "meta/hip": str(torch.version.hip)}
    fps_names = []
    for n in RUNGS:
        m = min(n, 48)
        fams = {"lattice": (lattice_clouds(n, np.random.default_rng(77 + n)), np.full(3, -1, np.int64), None),
                "thresh": searched(thresh_cloud, n, m, "thresh"),
                "scan": searched(scan_cloud, n, m, "scan")}
        for fam, (xyz, seed, want64) in fams.items():
            name = f"{fam}_n{n}"
            idx = twice(ref.fps, xyz, m)
            assert idx.min() >= 0 and idx.max() < n and (idx[:, 0] == 0).all(), name
            if want64 is not None:   # tie-free up to duplicates: the picked POINTS are the float64 replay's
                for b in range(3):
                    dec = want64[1][b]
                    assert np.array_equal(xyz[b][idx[b]][dec], xyz[b][want64[0][b]][dec]), (name, b, idx[b], want64[0][b])
            fps_names.append(name)
            d[f"fps/{name}/xyz"], d[f"fps/{name}/idx"], d[f"fps/{name}/seed"] = xyz, idx.astype(np.int32), seed
            print("fps", name, "seeds", seed.tolist(), "idx[0][:8]", idx[0][:8].tolist(), flush=True)

    def emd_case(name, a, b):
        cost = twice(ref.emd, a, b)
        f64 = np.array([MO.emd_cost(a[i], b[i], dtype=np.float64) for i in range(a.shape[0])])
        d[f"emd/{name}/a"], d[f"emd/{name}/b"] = a, b
        d[f"emd/{name}/ref"], d[f"emd/{name}/f64"], d[f"emd/{name}/e_ref"] = cost, f64, np.abs(cost.astype(np.float64) - f64)
        rel = np.abs(cost - f64) / np.maximum(np.abs(f64), 1e-30)
        print("emd", name, "cost", cost[:3].tolist(), "f64", f64[:3].tolist(), "max e_ref", float(np.abs(cost - f64).max()),
              "max rel", float(rel.max()), flush=True)
        return name

    emd_names = []
    for n, m in EMD_PAIRS:
        emd_names.append(emd_case(f"p{n}_{m}", lidar_like_clouds(2, n, seed=3 * n + m, drop=0.05),
                                  lidar_like_clouds(2, m, seed=5 * m + n + 1, drop=0.05) * np.float32(0.9)))
    emd_names.append(emd_case("b35_8_8", lidar_like_clouds(35, 8, seed=35, drop=0.05),
                              lidar_like_clouds(35, 8, seed=36, drop=0.05) * np.float32(0.9)))
    far = lidar_like_clouds(2, 32, seed=9, drop=0.05) + np.float32([100.0, 0.0, 0.0])
    emd_names.append(emd_case("far_96_32", lidar_like_clouds(2, 96, seed=8, drop=0.05), far.astype(np.float32)))
    s = lidar_like_clouds(2, 64, seed=10, drop=0.05)
    emd_names.append(emd_case("self_64", s, s.copy()))
    A, Bc = lidar_like_clouds(3, 64, seed=21, drop=0.05), lidar_like_clouds(4, 64, seed=22, drop=0.05) * np.float32(0.9)
    emd_case("mat64_pairs", np.repeat(A, 4, axis=0), np.tile(Bc, (3, 1, 1)))
    for k in ("ref", "f64", "e_ref"):
        d[f"emd/mat64/{k}"] = d.pop(f"emd/mat64_pairs/{k}").reshape(3, 4)
    del d["emd/mat64_pairs/a"], d["emd/mat64_pairs/b"]
    d["emd/mat64/a"], d["emd/mat64/b"] = A, Bc
    d["meta/fps_cases"], d["meta/emd_cases"] = np.array(fps_names), np.array(emd_names)
    np.savez_compressed(out_path, **d)
    print("wrote", out_path, os.path.getsize(out_path), "bytes; every reference call ran twice, identical")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "fps_emd.npz"))
