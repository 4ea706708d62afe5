"""GPU parity tests for the validation-metric kernels: csrc/metrics.hip, point_fps.hip,
point_chamfer.hip and point_emd.hip through the C ABI and the host glue of dusty_gan_amd/utils/metrics against oracle/metrics_oracle.py and tests/golden/metrics.npz."""
import math

import numpy as np
import pytest
import torch

from oracle import metrics_oracle as MO
from tests.golden_util import load, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


def lidar_like_clouds(B, n, seed, drop=0.15):
    """points on a jittered spherical grid in unit space with dropped returns at the origin and a duplicate"""
    rng = np.random.default_rng(seed)
    pitch = rng.uniform(-0.43, 0.06, (B, n))
    yaw = rng.uniform(-math.pi, math.pi, (B, n))
    r = np.exp(rng.uniform(math.log(0.01), math.log(0.9), (B, n)))
    pts = np.stack([r * np.cos(pitch) * np.cos(yaw), r * np.cos(pitch) * np.sin(yaw), r * np.sin(pitch)], -1)
    pts[rng.random((B, n)) < drop] = 0.0
    pts[:, n // 2] = pts[:, n // 3]  # exact duplicates -> exact ties in the FPS arg-max
    return pts.astype(np.float32)


@pytest.mark.parametrize("n,m", [(70, 20), (512, 64), (1000, 128), (4096, 512), (8192, 100),
                                 (65536, 512)])  # last: a full 64x1024 scan to the validation size
def test_fps_matches_oracle_indices(n, m):
    """index-exact furthest point sampling incl. the reference launcher's tie order and the origin-skip rule, at the
    validation sizes, against the restatement that tests/golden/fps_emd.npz pins to the reference's own kernel"""
    from dusty_gan_amd.utils.sampling import downsample_point_clouds, furthest_point_sampling
    B = 3 if n < 60000 else 1
    pts = lidar_like_clouds(B, n, seed=n + m)
    idx = furthest_point_sampling(torch.from_numpy(pts).to(DEV), m).cpu().numpy()
    sub = downsample_point_clouds(torch.from_numpy(pts).to(DEV), m).cpu().numpy()
    for b in range(B):
        want = MO.fps(pts[b], m)
        assert idx[b].tolist() == want.tolist(), b
        assert np.array_equal(sub[b], pts[b][want])
    with pytest.raises(AssertionError):
        furthest_point_sampling(torch.from_numpy(pts), m)  # the reference asserts is_cuda too


def test_fps_degenerate_clouds():
    from dusty_gan_amd.utils.sampling import furthest_point_sampling
    z = torch.zeros(2, 300, 3, device=DEV)
    assert furthest_point_sampling(z, 5).cpu().tolist() == [[0] * 5] * 2  # nothing is a candidate
    one = z.clone()
    one[0, 17] = torch.tensor([0.3, 0.1, 0.0])
    assert furthest_point_sampling(one, 3).cpu()[0].tolist() == [0, 17, 17]


@pytest.mark.parametrize("Na,n,Nb,m", [(5, 512, 7, 512), (9, 100, 4, 333), (3, 1024, 6, 700), (2, 3000, 5, 2048),
                                       (70, 512, 33, 512)])
def test_chamfer_dir_matches_oracle(Na, n, Nb, m):
    """all-pairs directed Chamfer means (every wave-per-cloud layout of the kernel: 1, 2 and whole workgroups, ragged
    cloud sizes, partially filled last workgroup) against the restated nnsearch; tolerance 1e-5 relative"""
    from dusty_gan_amd.utils.metrics import chamfer_dir, chamfer_distance_matrix
    A = lidar_like_clouds(Na, n, seed=Na + n)
    B = lidar_like_clouds(Nb, m, seed=Nb + m + 1)
    L = chamfer_dir(torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)).cpu()
    want = MO.chamfer_dir(A, B)
    assert L.shape == (Na, Nb)
    assert float(((L - want).abs() / want.abs().clamp_min(1e-12)).max()) < 1e-5
    M = chamfer_distance_matrix(torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)).cpu()
    assert rel_l2(M, MO.pairwise_cd(A, B)) < 1e-5
    At = torch.from_numpy(A).to(DEV)
    S = chamfer_distance_matrix(At, At).cpu()
    assert torch.equal(S, S.t()) and float(S.diag().abs().max()) == 0.0
    with pytest.raises(RuntimeError):
        chamfer_dir(torch.from_numpy(A), torch.from_numpy(B))


def test_cov_mmd_1nna_matches_oracle():
    from dusty_gan_amd.utils.metrics import compute_cov_mmd_1nna
    gen = lidar_like_clouds(24, 256, seed=1) * 0.8
    ref = lidar_like_clouds(31, 256, seed=2)
    got = compute_cov_mmd_1nna(torch.from_numpy(gen).to(DEV), torch.from_numpy(ref).to(DEV), 512, ("cd",), verbose=False)
    want = MO.compute_cov_mmd_1nna(gen, ref)
    assert set(got) == set(want) == {"mmd-cd", "mmd-sample-cd", "cov-cd", "1-nn-tp-cd", "1-nn-fp-cd", "1-nn-fn-cd",
                                     "1-nn-tn-cd", "1-nn-precision-cd", "1-nn-recall-cd", "1-nn-accuracy_t-cd",
                                     "1-nn-accuracy_f-cd", "1-nn-accuracy-cd"}
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-5 * max(1.0, abs(want[k])), (k, got[k], want[k])
    with pytest.raises(NotImplementedError):
        compute_cov_mmd_1nna(torch.from_numpy(gen).to(DEV), torch.from_numpy(ref).to(DEV), 512, ("swd",))


def test_cov_mmd_1nna_matches_the_reference_functions():
    """`utils.metrics.compute_cov_mmd_1nna`, `_compute_cov_mmd`, `_compute_nna` (device tensors, the all-pairs Chamfer
    kernel) against tests/golden/covmmd.npz: the outputs of the reference's own functions (cov_mmd_1nna.py:55-148) with its
    own CPU Chamfer search underneath.  Furthest point sampling and the EMD, which the reference holds only as CUDA
    sources, are pinned by tests/golden/fps_emd.npz: the outputs of those kernels built for gfx950 (the two tests named
    `..._the_reference_kernel(s)`)."""
    from tests.golden_util import load, sub
    from dusty_gan_amd.utils.metrics import compute_cov_mmd_1nna
    from dusty_gan_amd.utils.metrics.cov_mmd_1nna import _compute_cov_mmd, _compute_nna
    from dusty_gan_amd.utils.metrics.distance import chamfer_distance_matrix
    g = load("covmmd")
    for tag in ("rand", "ties", "wide"):
        M_rr, M_rg, M_gg = (torch.from_numpy(g[f"mat/{tag}/{k}"]).to(DEV) for k in ("M_rr", "M_rg", "M_gg"))
        for k, v in _compute_cov_mmd(M_rg).items():
            if tag != "rand" and k == "cov":
                continue   # (argmin over tied minima: torch's CPU and device kernels may pick different ones, as they would
                           #  for the reference itself; the fixture was made on the CPU)
            assert abs(v - float(g[f"mat/{tag}/covmmd/{k}"])) <= 1e-6, (tag, k)
        for kk, sq in ((1, False), (3, False), (1, True)):
            s_ = _compute_nna(M_rr, M_rg, M_gg, k=kk, sqrt=sq)
            n_ref, n_gen = M_rg.shape
            assert s_["tp"] + s_["fn"] == n_ref and s_["fp"] + s_["tn"] == n_gen
            if tag == "rand":   # tie-free: exact; with ties the neighbour torch.topk returns is backend-dependent
                for k, v in s_.items():
                    assert abs(v - float(g[f"mat/{tag}/nna_k{kk}_sqrt{int(sq)}/{k}"])) <= 1e-6, (tag, kk, sq, k)
    ref, gen = torch.from_numpy(g["pcs_ref"]).to(DEV), torch.from_numpy(g["pcs_gen"]).to(DEV)
    assert rel_l2(chamfer_distance_matrix(ref, gen).cpu(), g["e2e_mat/M_rg"]) < 1e-5
    got = compute_cov_mmd_1nna(gen, ref, 5, ("cd",), verbose=False)
    want = sub(g, "e2e", as_torch=False)
    assert set(got) == set(want)
    for k, v in want.items():
        assert abs(got[k] - float(v)) <= 1e-5 * max(1.0, abs(float(v))), (k, got[k], float(v))


@pytest.mark.parametrize("n,m", [(64, 64), (200, 200), (96, 32), (50, 150)])
def test_emd_matches_oracle(n, m):
    """approxmatch + matchcost (earth_mover_distance.cu) fused: paired costs and the all-pairs matrix against the numpy
    restatement (itself held to the reference's kernels by tests/golden/fps_emd.npz, whose order of operations it follows;
    the kernel sums the cost per level instead of over a stored match matrix) -> 1e-3 relative"""
    from dusty_gan_amd.utils.metrics import earth_mover_distance
    from dusty_gan_amd.utils.metrics.distance import emd_distance_matrix
    a = lidar_like_clouds(4, n, seed=n, drop=0.05)
    b = lidar_like_clouds(4, m, seed=m + 7, drop=0.05) * 0.9
    got = earth_mover_distance(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)).cpu()
    want = torch.tensor([MO.emd_cost(a[i], b[i]) for i in range(4)])
    assert float(((got - want).abs() / want.abs().clamp_min(1e-9)).max()) < 1e-3, (got, want)
    if n == m:
        M = emd_distance_matrix(torch.from_numpy(a[:3]).to(DEV), torch.from_numpy(b).to(DEV)).cpu()
        assert M.shape == (3, 4) and rel_l2(M, MO.pairwise_emd(a[:3], b)) < 1e-3
        self_cost = earth_mover_distance(torch.from_numpy(a).to(DEV), torch.from_numpy(a).to(DEV)).cpu()
        assert float(self_cost.max()) < 1e-2 * float(want.min())  # a cloud matches itself at (almost) no cost


@pytest.mark.parametrize("family", ["lattice", "thresh", "scan"])
def test_fps_matches_the_reference_kernel(family):
    """`furthest_point_sampling` / `downsample_point_clouds` against what the reference's OWN kernel and launcher returned on
    an MI355X (tests/golden/fps_emd.npz): index-exact on every rung of the launcher's block-size ladder (n = 1 .. 2048,
    B = 3, m = min(n, 48)); lattice: exact arithmetic and ties everywhere (the tie order); thresh: points exactly at, just
    below and just above the origin-skip threshold; scan: dropped returns and a duplicate, selections that do not depend
    on multiply-add fusion.  Where oracle/_ref/libref_fps_emd.so has been built the reference's kernel is also run live,
    in this process, and must return the fixture bit for bit."""
    from dusty_gan_amd.utils.sampling import downsample_point_clouds, furthest_point_sampling
    from tests.ref_fps_emd_util import RefFpsEmd
    from tests.test_oracle_golden import FPS_RUNGS
    g = load("fps_emd")
    ref = RefFpsEmd.open()
    for n in FPS_RUNGS:
        name = f"{family}_n{n}"
        xyz, want = g[f"fps/{name}/xyz"], g[f"fps/{name}/idx"]
        m = want.shape[1]
        if ref is not None:
            assert np.array_equal(ref.fps(xyz, m), want), name
        x = torch.from_numpy(xyz).to(DEV)
        idx = furthest_point_sampling(x, m).cpu().numpy()
        sub = downsample_point_clouds(x, m).cpu().numpy()
        for b in range(3):
            assert idx[b].tolist() == want[b].tolist(), (name, b)
            assert np.array_equal(sub[b], xyz[b][want[b]]), (name, b)


def test_emd_matches_the_reference_kernels():
    """`earth_mover_distance` / `emd_distance_matrix` against the reference's OWN approxmatch + matchcost kernels as run on an
    MI355X (tests/golden/fps_emd.npz): integer and truncated n/m factors both ways, the 512-thread and 1024-point chunk
    edges, b = 35 (the 32-block grid stride), far-apart clouds (the 1e-9 guards decide), a cloud with itself.  Per pair
    the cost must lie within 2 * e_ref + 1e-6 * |cost| of the same algorithm in float64, e_ref being the reference's own
    distance from it.  Where oracle/_ref/libref_fps_emd.so has been built the reference's kernels are also run live and
    must return the recorded costs."""
    from dusty_gan_amd.utils.metrics import earth_mover_distance
    from dusty_gan_amd.utils.metrics.distance import emd_distance_matrix
    from tests.ref_fps_emd_util import RefFpsEmd
    from tests.test_oracle_golden import EMD_CASES
    g = load("fps_emd")
    ref = RefFpsEmd.open()
    bad = []
    for name in EMD_CASES:
        a, b = g[f"emd/{name}/a"], g[f"emd/{name}/b"]
        f64, e_ref = g[f"emd/{name}/f64"], g[f"emd/{name}/e_ref"]
        if ref is not None:
            assert np.array_equal(ref.emd(a, b), g[f"emd/{name}/ref"]), name
        got = earth_mover_distance(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)).cpu().numpy().astype(np.float64)
        for i in range(a.shape[0]):
            print(name, i, "f64", f64[i], "e_ref", e_ref[i], "|ours - f64|", abs(got[i] - f64[i]))
            if not abs(got[i] - f64[i]) <= 2.0 * e_ref[i] + 1e-6 * abs(f64[i]):
                bad.append((name, i, got[i], f64[i], e_ref[i]))
    A, B = g["emd/mat64/a"], g["emd/mat64/b"]
    f64, e_ref = g["emd/mat64/f64"], g["emd/mat64/e_ref"]
    if ref is not None:
        live = ref.emd(np.repeat(A, 4, axis=0), np.tile(B, (3, 1, 1))).reshape(3, 4)
        assert np.array_equal(live, g["emd/mat64/ref"])
    M = emd_distance_matrix(torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)).cpu().numpy().astype(np.float64)
    assert M.shape == (3, 4)
    for i in range(3):
        for j in range(4):   # the matrix holds compute_emd = cost / N
            print("mat64", i, j, "f64", f64[i, j], "e_ref", e_ref[i, j], "|ours - f64|", abs(M[i, j] * 64.0 - f64[i, j]))
            if not abs(M[i, j] * 64.0 - f64[i, j]) <= 2.0 * e_ref[i, j] + 1e-6 * abs(f64[i, j]):
                bad.append(("mat64", i, j, M[i, j] * 64.0, f64[i, j], e_ref[i, j]))
    assert not bad, bad


def test_cov_mmd_1nna_emd_matches_oracle():
    from dusty_gan_amd.utils.metrics import compute_cov_mmd_1nna
    gen = lidar_like_clouds(7, 64, seed=11) * 0.8
    ref = lidar_like_clouds(9, 64, seed=12)
    got = compute_cov_mmd_1nna(torch.from_numpy(gen).to(DEV), torch.from_numpy(ref).to(DEV), 512, ("cd", "emd"), verbose=False)
    want = MO.compute_cov_mmd_1nna(gen, ref, ("cd", "emd"))
    assert set(got) == set(want) and len(got) == 24
    for k in want:
        assert abs(got[k] - want[k]) <= 2e-3 * max(1.0, abs(want[k])), (k, got[k], want[k])


def test_jsd_matches_reference_golden():
    """utils/metrics/jsd.py: counters bit-exact, divergence to 1e-5, against the reference's own outputs"""
    from dusty_gan_amd.utils.metrics import compute_jsd
    from dusty_gan_amd.utils.metrics.jsd import grid_counters
    g = load("metrics")
    for name in ("gen", "ref"):
        c = grid_counters(torch.from_numpy(g[f"pcs_{name}"]).to(DEV)).cpu()
        assert torch.equal(c, torch.from_numpy(g[f"counters_{name}"])), name
    got = compute_jsd(torch.from_numpy(g["pcs_gen"]).to(DEV), torch.from_numpy(g["pcs_ref"]).to(DEV), verbose=False)
    assert abs(got - float(g["jsd"])) < 1e-5
    # a larger seeded case against the oracle (pinned to the same vectors on the CPU)
    a = lidar_like_clouds(40, 512, seed=5) / 2.0
    b = lidar_like_clouds(40, 512, seed=6) / 2.2
    ca = grid_counters(torch.from_numpy(a).to(DEV)).cpu()
    assert torch.equal(ca, MO.grid_counters(a))
    assert abs(compute_jsd(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)) - MO.compute_jsd(a, b)) < 1e-5


def test_swd_matches_reference_golden():
    """utils/metrics/swd.py: pyramid / patch kernels + projections, with the reference's captured random draws,
    against the reference's scores (1e-4) and level by level against the oracle's pyramid (1e-5)"""
    from dusty_gan_amd.utils.metrics import compute_swd
    from dusty_gan_amd.utils.metrics.swd import extract_patches, laplacian_pyramid
    from tests.test_oracle_golden import swd_rand
    g = load("metrics")
    rand, bs = swd_rand(g)
    i1, i2 = torch.from_numpy(g["swd/image1"]), torch.from_numpy(g["swd/image2"])
    got = compute_swd(i1.to(DEV), i2.to(DEV), batch_size=bs, rand=rand)
    assert set(got) == {"swd-16", "swd-32", "swd-mean"}
    for k, v in got.items():
        assert abs(v - float(g[f"swd/score/{k}"])) < 1e-4 * max(1.0, abs(v)), (k, v, float(g[f"swd/score/{k}"]))
    pyr = laplacian_pyramid(i1.to(DEV), 2)
    ref = MO.laplacian_pyramid(i1, 2)
    for a, b in zip(pyr, ref):
        assert a.shape == b.shape and rel_l2(a.cpu(), b) < 1e-5
    big = torch.randn(3, 2, 64, 256)  # 3 levels, 2 channels
    for a, b in zip(laplacian_pyramid(big.to(DEV), 3), MO.laplacian_pyramid(big, 3)):
        assert rel_l2(a.cpu(), b) < 1e-5
    inds = torch.tensor([0, 5, 58 * 250 - 1, 777])
    pa = extract_patches(big.to(DEV), (7, 7), 4, inds).cpu()
    assert torch.equal(pa, MO.extract_patches(big, (7, 7), inds))
    # own draws: finite, deterministic under a seeded device generator, ~0 for identical sets
    torch.manual_seed(0)
    s1 = compute_swd(big.to(DEV), (big * 0.5).to(DEV))
    torch.manual_seed(0)
    s2 = compute_swd(big.to(DEV), (big * 0.5).to(DEV))
    assert s1 == s2 and set(s1) == {"swd-16", "swd-32", "swd-64", "swd-mean"} and all(np.isfinite(v) for v in s1.values())
    # identical sets sampled at identical positions are at distance exactly 0
    counts = MO.swd_patch_counts(64, 256, 3)
    one = [torch.randperm(c)[:128] for c in counts]
    rand0 = {"inds": [[one, one]], "dirs": [[torch.randn(2 * 49, 128) for _ in range(4)] for _ in range(3)]}
    same = compute_swd(big.to(DEV), big.clone().to(DEV), rand=rand0)
    assert same["swd-mean"] == 0.0
