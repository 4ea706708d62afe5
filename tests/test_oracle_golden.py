"""The oracle (oracle/dusty_oracle.py) against the vectors generated from the reference's own modules."""
import numpy as np
import pytest
import torch

from oracle import dusty_oracle as O
from tests.golden_util import PL_CASES, STEP_CASES, load, meta_pl, rel_l2, step_rand, sub

TOL = 2e-5  # fp32 CPU vs fp32 CPU, same library: rounding-order differences only


@pytest.fixture(scope="module")
def ops():
    return load("ops")


def t(a):
    return torch.from_numpy(np.array(a))


@pytest.mark.parametrize("ring", [True, False])
def test_pad_and_blur(ops, ring):
    r = f"ring{int(ring)}"
    assert torch.equal(O.pad_ring(t(ops[f"pad/{r}/x"]), ring), t(ops[f"pad/{r}/y"]))
    assert rel_l2(O.blur_vh(t(ops[f"blurvh/{r}/x"]), ring), ops[f"blurvh/{r}/y"]) < 1e-6


@pytest.mark.parametrize("ring", [True, False])
@pytest.mark.parametrize("kind", ["up", "down"])
def test_up_down_fwd_bwd(ops, kind, ring):
    tag = f"{kind}/ring{int(ring)}"
    x = t(ops[f"{tag}/x"]).requires_grad_()
    w = t(ops[f"{tag}/param/1.module.weight"]).requires_grad_()
    b = t(ops[f"{tag}/param/2.bias"]).requires_grad_()
    y = (O.up if kind == "up" else O.down)(x, w, b, ring)
    assert rel_l2(y, ops[f"{tag}/y"]) < TOL
    gx, gw, gb = torch.autograd.grad(y, [x, w, b], t(ops[f"{tag}/gy"]))
    assert rel_l2(gx, ops[f"{tag}/gx"]) < TOL
    assert rel_l2(gw, ops[f"{tag}/grad/1.module.weight"]) < TOL
    assert rel_l2(gb, ops[f"{tag}/grad/2.bias"]) < TOL


def test_proj_and_head(ops):
    y = O.proj(t(ops["proj/x"]), t(ops["proj/param/0.module.weight"]), t(ops["proj/param/1.bias"]))
    assert rel_l2(y, ops["proj/y"]) < TOL
    x = t(ops["head/x"])
    for name in ("depth", "confidence"):
        y = O.head(x, t(ops[f"head/param/heads.{name}.1.module.weight"]), t(ops[f"head/param/heads.{name}.1.module.bias"]))
        assert rel_l2(y, ops[f"head/y/{name}"]) < TOL


@pytest.mark.parametrize("fname", ["brightness", "saturation", "contrast", "translation", "cutout"])
def test_augment_functions(ops, fname):
    rp = sub(ops, f"aug/{fname}")
    y = O.diff_augment(t(ops["aug/x"]), rp, policy=(fname,))
    assert rel_l2(y, ops[f"aug/{fname}/y"]) < 1e-6


def test_gumbel_sigmoid(ops):
    lg = t(ops["gumbel/logits"]).requires_grad_()
    y = O.gumbel_sigmoid(lg, t(ops["gumbel/noise"]), 1.0)
    assert torch.equal(y.detach(), t(ops["gumbel/y"]))
    assert set(np.unique(y.detach().numpy())) <= {0.0, 1.0}
    (g,) = torch.autograd.grad(y, lg, t(ops["gumbel/gy"]))
    assert rel_l2(g, ops["gumbel/glogits"]) < 1e-6


@pytest.mark.parametrize("metric", ["nsgan", "wgan", "lsgan", "hinge", "ragan", "rahinge", "ralsgan"])
def test_gan_loss(ops, metric):
    pr, pf = t(ops["ganloss/pred_real"]), t(ops["ganloss/pred_fake"])
    for mode in ("D", "G"):
        assert abs(float(O.gan_loss(metric, pr, pf, mode)) - float(ops[f"ganloss/{metric}/{mode}"])) < 1e-6
    with pytest.raises(NotImplementedError):
        O.gan_loss("nope", pr, pf, "D")
    with pytest.raises(ValueError):
        O.gan_loss("nsgan", pr, pf, "X")


def test_invert_depth(ops):
    pol = t(ops["invert_depth/pol"])
    inv, _ = O.fetch_reals(pol, torch.ones_like(pol))
    assert rel_l2((inv + 1) / 2, ops["invert_depth/inv"]) < 1e-6


TOL_STEP = TOL


@pytest.mark.parametrize("case", STEP_CASES + PL_CASES)
def test_train_step_matches_reference(case):
    g = load("step_" + case)
    arch, ring = str(g["meta/arch"]), bool(g["meta/ring"])
    cfg = O.StepConfig(arch=arch, ring=ring, gan_mode=str(g["meta/gan_mode"]), w_gp=float(g["meta/gp"]), w_pl=meta_pl(g),
                       lr_g=float(g["meta/lr"]), lr_d=float(g["meta/lr"]), beta1=float(g["meta/beta1"]),
                       beta2=float(g["meta/beta2"]), ema_decay=float(g["meta/ema_decay"]))
    G, D = sub(g, "init/G"), sub(g, "init/D")
    D = {k: v for k, v in D.items() if not k.endswith("kernel")}  # BlurVH buffers are constants
    G_ema = {k: v.clone() for k, v in G.items()}
    oG, oD = O.new_optim_state(G), O.new_optim_state(D)
    # with the path-length term the second step starts from parameters that carry the Adam sensitivity noted below
    TOL = TOL_STEP if cfg.w_pl == 0 else 10 * TOL_STEP
    for it in range(int(g["meta/steps"])):
        pre = f"s{it}"
        pol, mask = t(g[f"{pre}/pol"]), t(g[f"{pre}/mask"])
        x_real, _ = O.fetch_reals(pol, mask)
        assert rel_l2(x_real, g[f"{pre}/x_real"]) < 1e-6
        sc, ex = O.train_step(G, D, G_ema, oG, oD, it + 1, cfg, x_real, step_rand(g, it), return_grads=True)
        for k, v in sub(g, f"{pre}/scalar").items():
            assert abs(sc[k] - float(v)) <= 1e-4 * max(1.0, abs(float(v))), (k, sc[k], float(v))
        for k, v in sub(g, f"{pre}/synth").items():
            if k == "mask":
                assert torch.equal(ex["synth"][k], v)
            else:
                assert rel_l2(ex["synth"][k], v) < TOL, k
        assert rel_l2(ex["x_real_aug"], g[f"{pre}/x_real_aug"]) < TOL
        assert rel_l2(ex["x_fake_aug"], g[f"{pre}/x_fake_aug"]) < TOL
        assert rel_l2(ex["y_real"], g[f"{pre}/y_real"]) < TOL
        assert rel_l2(ex["y_fake2"], g[f"{pre}/y_fake2"]) < 1e-4
        if cfg.w_pl > 0:
            assert rel_l2(ex["pl_grads_z"], g[f"{pre}/pl/grads_z"]) < 1e-4
        if cfg.w_gp > 0:
            assert rel_l2(ex["r1_grads"], g[f"{pre}/r1_grads"]) < TOL
        for k, v in sub(g, f"{pre}/grad_D").items():
            assert rel_l2(ex["grad_D"][k], v) < 1e-4, k
        for k, v in sub(g, f"{pre}/grad_G").items():
            assert rel_l2(ex["grad_G"][k], v) < 1e-4, k
        for tag, cur in (("G", G), ("D", D), ("G_ema", G_ema)):
            for k, v in sub(g, f"{pre}/after/{tag}").items():
                if k.endswith("kernel"):
                    continue  # BlurVH buffers, not parameters
                # Adam turns a gradient element of the order of eps = 1e-8 into a step that moves with its rounding
                # noise (the path-length double backward leaves such nearly cancelled bias gradients): accept 2.5 % of
                # one lr step on single elements
                assert rel_l2(cur[k], v) < 1e-4 or float((cur[k] - v).abs().max()) < 5e-5, (tag, k)
    for tag, opt in (("G", oG), ("D", oD)):
        for k in opt:
            assert rel_l2(opt[k]["v"], g[f"final/optim_{tag}/{k}/exp_avg_sq"]) < 1e-4
            assert rel_l2(opt[k]["m"], g[f"final/optim_{tag}/{k}/exp_avg"]) < 1e-4


# ---------------------------------------------------------------------------------------------------------------
# data formats either side of the step: oracle/lidar_oracle.py
# ---------------------------------------------------------------------------------------------------------------
def test_scan_preprocess_matches_reference_kitti_dataset():
    """datasets/kitti.py:54-67 (KITTIOdometry.preprocess: norm, the three strict range tests, normalisation, zeroing) -
    the restatement in oracle/lidar_oracle.py against what the reference's own class returned (tests/golden/kitti_pre.npz,
    made by `make_golden.py kitti`: the file loaded by path with an empty torchvision placeholder).  Bit-exact, including
    the points that sit exactly on min_depth / max_depth.  At an identity output size the NEAREST resize of `transform`
    (torchvision, third party) is the identity, so the whole `scan_to_polar` is pinned there."""
    from oracle import lidar_oracle as LO
    g = load("kitti_pre")
    for k in range(3):
        pts = g[f"s{k}/points"]
        Hs, Ws = pts.shape[:2]
        out = LO.scan_to_polar(pts, (Hs, Ws), float(g["meta/min_depth"]), float(g["meta/max_depth"]))
        assert torch.equal(out["mask"][0], torch.from_numpy(g[f"s{k}/mask"])), k
        assert torch.equal(out["depth"][0], torch.from_numpy(g[f"s{k}/depth"])), k
        assert torch.equal(out["xyz"], torch.from_numpy(g[f"s{k}/xyz"]).permute(2, 0, 1)), k
        m = g[f"s{k}/mask"]
        assert 0.1 < m.mean() < 0.95 and (g[f"s{k}/depth"][~m] == 0).all()


def test_lidar_oracle_matches_reference():
    """utils/lidar.py restatement against vectors from the reference's LiDAR class (tests/golden/lidar.npz)"""
    from oracle import lidar_oracle as LO
    g = load("lidar")
    H, W = (int(v) for v in g["meta/shape"])
    mn, mx = float(g["meta/min_depth"]), float(g["meta/max_depth"])
    angle = LO.init_coordmap(t(g["angle_src"]), H, W)
    assert rel_l2(angle, g["angle"]) < 1e-6
    inv = t(g["inv"])
    live = inv[inv > 0]
    assert rel_l2(LO.revert_depth(live, mn, mx), g["revert_depth/norm"]) < 1e-6
    assert rel_l2(LO.revert_depth(live, mn, mx, norm=False), g["revert_depth/metric"]) < 1e-6
    pol = LO.revert_depth(live, mn, mx)
    back, _ = O.fetch_reals(pol, torch.ones_like(pol))
    assert rel_l2((back + 1) / 2, g["invert_depth"]) < 1e-6
    assert rel_l2(LO.pol_to_xyz(inv, angle), g["pol_to_xyz"]) < 1e-6
    pts = LO.inv_to_xyz(inv, angle, mn, mx)
    assert rel_l2(pts, g["points"]) < 1e-6
    assert torch.equal(pts[:, :1][inv == 0], torch.zeros_like(pts[:, :1][inv == 0]))  # dropped points sit at the origin
    out = LO.postprocess({"depth": t(g["gen_depth"]), "confidence": torch.zeros(1)}, angle, mn, mx)
    assert rel_l2(out["points"], g["gen_points"]) < 1e-6
    assert float(out["confidence"]) == 0.5
    assert float((out["normals"] - t(g["gen_normals"])).abs().max()) < 1e-6
    assert float((LO.xyz_to_normal(t(g["points"])) - t(g["normals"])).abs().max()) < 1e-6


def test_scan_to_polar_restatement_properties():
    """datasets/kitti.py:54-77 restatement (parity unpinned against the reference class, see the oracle header):
    hand-computed cells, range mask at the boundaries, zeroing, hflip-before-resize and the NEAREST index rule."""
    from oracle import lidar_oracle as LO
    Hs, Ws = 4, 16
    pts = np.zeros((Hs, Ws, 4), np.float32)
    pts[0, 0, :3] = (3.0, 4.0, 0.0)        # |.| = 5
    pts[0, 2, :3] = (0.0, 0.0, 0.5)        # below min_depth -> invalid
    pts[1, 4, :3] = (0.0, 120.0, 0.0)      # == max_depth -> invalid (strict <)
    pts[1, 6, :3] = (0.0, 0.9, 0.0)        # == min_depth -> invalid (strict >)
    pts[2, 14, :3] = (1.0, 2.0, 2.0)       # |.| = 3
    pts[..., 3] = 0.7                      # reflectance is ignored for the depth modality
    out = LO.scan_to_polar(pts, (4, 8))
    assert out["depth"].shape == (1, 4, 8) and out["mask"].dtype == torch.bool and out["xyz"].shape == (3, 4, 8)
    assert int(out["mask"].sum()) == 2
    assert abs(float(out["depth"][0, 0, 0]) - (5.0 - 0.9) / 119.1) < 1e-7    # source column 0 -> 0
    assert abs(float(out["depth"][0, 2, 7]) - (3.0 - 0.9) / 119.1) < 1e-7    # source column 14 -> 7 (src = 2 * dst)
    assert torch.allclose(out["xyz"][:, 2, 7], torch.tensor([1.0, 2.0, 2.0]) / 120.0)
    assert float(out["depth"][0, 0, 1]) == 0.0 and float(out["depth"][0, 1, 2]) == 0.0 and float(out["depth"][0, 1, 3]) == 0.0
    fl = LO.scan_to_polar(pts, (4, 8), flip=True)
    # flipped source column of (0,0) is 15 -> lands on an odd column that NEAREST (src = 2 * dst) never samples
    assert int(fl["mask"].sum()) == 0
    pts[0, 1, :3] = (3.0, 4.0, 0.0)
    fl = LO.scan_to_polar(pts, (4, 8), flip=True)
    assert bool(fl["mask"][0, 0, 7])       # flipped column 14 -> output column 7
    # non-integer ratio: torch's legacy nearest, src = floor(dst * in / out)
    out = LO.scan_to_polar(pts, (3, 5))
    src_w = [int(np.floor(i * np.float32(16 / 5))) for i in range(5)]
    src_h = [int(np.floor(i * np.float32(4 / 3))) for i in range(3)]
    full = LO.scan_to_polar(pts, (4, 16))
    assert torch.equal(out["depth"], full["depth"][:, src_h][:, :, src_w])


@pytest.mark.parametrize("n,world", [(10, 1), (10, 4), (3, 8), (257, 2)])
def test_sampler_restatement_matches_torch(n, world):
    """oracle sampler == torch.utils.data.distributed.DistributedSampler as the reference builds it (:88)"""
    from oracle import lidar_oracle as LO
    from torch.utils.data.distributed import DistributedSampler
    for rank in range(world):
        ref = list(DistributedSampler(range(n), num_replicas=world, rank=rank))
        assert LO.sampler_indices(n, world, rank) == ref
    idx = LO.sampler_indices(n, world, 0)
    bs = LO.batches(idx, 2)
    assert all(len(b) == 2 for b in bs) and len(bs) == len(idx) // 2


# ---------------------------------------------------------------------------------------------------------------
# validation metrics: oracle/metrics_oracle.py
# ---------------------------------------------------------------------------------------------------------------
def test_jsd_oracle_matches_reference():
    """utils/metrics/jsd.py restatement against the reference's own outputs (tests/golden/metrics.npz)"""
    from oracle import metrics_oracle as MO
    g = load("metrics")
    assert torch.equal(MO.unit_cube_grid(int(g["meta/resolution"])), t(g["grid"]))
    for name in ("gen", "ref"):
        assert torch.equal(MO.grid_counters(g[f"pcs_{name}"]), t(g[f"counters_{name}"]))
    assert abs(MO.compute_jsd(g["pcs_gen"], g["pcs_ref"]) - float(g["jsd"])) < 1e-6


def test_fps_and_chamfer_restatements():
    """restatements of the reference's CUDA extensions (pinned to its own code by tests/golden/chamfer.npz and
    fps_emd.npz): literal loops of the cited sources on tiny inputs against the vectorised oracle"""
    from oracle import metrics_oracle as MO
    rng = np.random.default_rng(3)
    xyz = rng.normal(0, 0.3, (70, 3)).astype(np.float32)
    xyz[5] = xyz[9] = 0.0                     # dropped points: never candidates (mag <= 1e-3)
    xyz[40] = xyz[12]                         # exact duplicate -> exact distance ties
    idx = MO.fps(xyz, 20)
    # literal thread-order emulation of furthest_point_sampling.cu:115-206 with T = opt_n_threads(70) = 64 threads
    T = MO.opt_n_threads(70)
    assert T == 64
    temp = np.full(70, 1e10, np.float32)
    old, want = 0, [0]
    for j in range(1, 20):
        best, besti = np.full(T, -1.0, np.float32), np.zeros(T, np.int64)
        for tid in range(T):
            for k in range(tid, 70, T):
                x2 = xyz[k]
                if (x2[0] * x2[0]) + (x2[1] * x2[1]) + (x2[2] * x2[2]) <= np.float32(1e-3):
                    continue
                dd = x2 - xyz[old]
                d = (dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]
                d2 = min(d, temp[k])
                temp[k] = d2
                if d2 > best[tid]:
                    best[tid], besti[tid] = d2, k
        w = T // 2
        while w >= 1:  # __update: keeps the lower thread unless the upper one is strictly greater
            for tid in range(w):
                if best[tid + w] > best[tid]:
                    best[tid], besti[tid] = best[tid + w], besti[tid + w]
            w //= 2
        old = int(besti[0])
        want.append(old)
    assert idx.tolist() == want
    assert len(set(idx.tolist())) == 20 and 5 not in idx and 9 not in idx
    assert MO.fps(np.zeros((10, 3), np.float32), 4).tolist() == [0, 0, 0, 0]  # nothing is a candidate: besti stays 0
    # Chamfer: literal nnsearch (chamfer_distance.cpp:41-66) on two tiny sets
    A = rng.normal(0, 0.3, (2, 9, 3)).astype(np.float32)
    B = rng.normal(0, 0.3, (3, 7, 3)).astype(np.float32)
    L = MO.chamfer_dir(A, B)
    for i in range(2):
        for j in range(3):
            tot = 0.0
            for p in A[i]:
                tot += min(float(np.float32(((q - p) * (q - p)).sum())) for q in B[j])
            assert abs(float(L[i, j]) - tot / 9) < 1e-6
    M = MO.pairwise_cd(A, A)
    assert torch.allclose(M, M.t()) and float(M.diag().abs().max()) == 0.0
    # EMD (approxmatch + matchcost): a cloud matches itself - in any point order - at zero cost; translating it by t
    # costs n * |t|^2 once the matching is (nearly) one to one
    pts = rng.normal(0, 0.3, (40, 3)).astype(np.float32)
    assert MO.emd_cost(pts, pts) < 1e-6 and MO.emd_cost(pts, pts[::-1].copy()) < 1e-6
    shift = np.float32([0.01, 0.0, 0.0])
    assert abs(MO.emd_cost(pts, pts + shift) / (40 * 1e-4) - 1.0) < 0.05
    assert MO.pairwise_emd(pts[None], (pts + shift)[None]).shape == (1, 1)
    # COV / MMD / 1-NNA on a hand-made matrix
    M_rg = torch.tensor([[0.1, 0.9, 0.8], [0.7, 0.2, 0.9]])
    r = MO.cov_mmd(M_rg)
    assert abs(r["mmd"] - 0.15) < 1e-6 and abs(r["mmd-sample"] - (0.1 + 0.2 + 0.8) / 3) < 1e-6 and r["cov"] == 1.0
    s = MO.nna(torch.tensor([[0.0, 0.5], [0.5, 0.0]]), M_rg, torch.tensor([[0.0, .3, .3], [.3, 0.0, .05], [.3, .05, 0.0]]))
    # nearest neighbours: r0 -> g0 (0.1), r1 -> g1 (0.2), g0 -> r0, g1 -> g2, g2 -> g1  => predictions 0,0,1,0,0
    assert (s["tp"], s["fp"], s["fn"], s["tn"]) == (0.0, 1.0, 2.0, 2.0) and abs(s["accuracy"] - 0.4) < 1e-6


def swd_rand(g):
    from oracle import metrics_oracle as MO
    bs, npatch, reps, nd = (int(v) for v in g["swd/meta"])
    B, C, H, W = g["swd/image1"].shape
    L = MO.swd_num_levels(H, W)
    inds = [[[t(g[f"swd/inds/{mb}/{w}/{l}"]) for l in range(L)] for w in range(2)] for mb in range(-(-B // bs))]
    dirs = [[t(g[f"swd/dirs/{l}/{r}"]) for r in range(reps)] for l in range(L)]
    return {"inds": inds, "dirs": dirs}, bs


def test_swd_oracle_matches_reference():
    """utils/metrics/swd.py restatement, fed the reference's own captured draws, against the reference's scores"""
    from oracle import metrics_oracle as MO
    g = load("metrics")
    rand, bs = swd_rand(g)
    got = MO.compute_swd(g["swd/image1"], g["swd/image2"], rand, batch_size=bs)
    assert set(got) == {"swd-16", "swd-32", "swd-mean"}
    for k, v in got.items():
        assert abs(v - float(g[f"swd/score/{k}"])) < 1e-6, k
    assert MO.swd_patch_counts(32, 64, 2) == [26 * 58, 10 * 26]


def test_chamfer_oracle_pinned_by_the_reference_nnsearch():
    """oracle/metrics_oracle.py `chamfer_dir` against the reference's OWN nearest-neighbour search: `nnsearch` of
    utils/metrics/distance/cd/chamfer_distance.cpp:39-66, compiled from the reference's source file by
    oracle/Makefile.ref into oracle/_ref/libref_cd.so.  Its outputs on these clouds are stored in tests/golden/chamfer.npz
    (make_golden.py chamfer); wherever the library has been built (__graft_entry__.build() with the reference's sources
    at hand) the fixture is also checked against it, bit for bit.  Ragged sizes, duplicate points (first index wins on
    ties), one-point clouds."""
    import ctypes
    import os
    from oracle import metrics_oracle as MO
    g = load("chamfer")
    so = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libref_cd.so")
    lib = ctypes.CDLL(so) if os.path.exists(so) else None
    vp = ctypes.c_void_p

    def ref_nnsearch(x1, x2):  # x1 [b,n,3], x2 [b,m,3] -> dist [b,n], idx [b,n]
        x1, x2 = np.ascontiguousarray(x1, np.float32), np.ascontiguousarray(x2, np.float32)
        b, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
        dist, idx = np.zeros((b, n), np.float32), np.zeros((b, n), np.int32)
        lib.ref_cd_nnsearch(b, n, m, x1.ctypes.data_as(vp), x2.ctypes.data_as(vp), dist.ctypes.data_as(vp), idx.ctypes.data_as(vp))
        return dist, idx
    for c in range(int(g["meta/cases"])):
        A, B = g[f"{c}/A"], g[f"{c}/B"]
        Na, Nb = A.shape[0], B.shape[0]
        dist, idx = g[f"{c}/dist"], g[f"{c}/idx"]   # [Na, Nb, n]: nnsearch(A[i], B[j])
        assert (B[:, -1] == B[:, 0]).all()          # duplicate points: ties
        if lib is not None:
            for i in range(Na):
                for j in range(Nb):
                    d, k = ref_nnsearch(A[i][None], B[j][None])
                    assert np.array_equal(d[0], dist[i, j]) and np.array_equal(k[0], idx[i, j]), (c, i, j)
        L = MO.chamfer_dir(A, B).numpy()
        for i in range(Na):
            for j in range(Nb):
                d = dist[i, j]
                assert abs(L[i, j] - d.mean()) <= 1e-6 * max(1.0, abs(d.mean())), (i, j)
        # compute_cd of cov_mmd_1nna.py:20-22 = dl.mean + dr.mean
        if Na == Nb:
            dist_rev = g[f"{c}/dist_rev"]           # [Na, m]: nnsearch(B[i], A[i])
            if lib is not None:
                for i in range(Na):
                    d, k = ref_nnsearch(B[i][None], A[i][None])
                    assert np.array_equal(d[0], dist_rev[i]) and np.array_equal(k[0], g[f"{c}/idx_rev"][i]), (c, i)
            M = MO.pairwise_cd(A, B).numpy()
            for i in range(Na):
                dl, dr = dist[i, i], dist_rev[i]
                assert abs(M[i, i] - (dl.mean() + dr.mean())) <= 1e-6 * max(1.0, abs(M[i, i]))


FPS_RUNGS = [1, 2, 3, 5, 8, 17, 33, 70, 130, 300, 513, 1000, 1025, 2048]
FPS_FAMILIES = ["lattice", "thresh", "scan"]
EMD_CASES = ["p1_1", "p2_3", "p4_4", "p64_64", "p96_32", "p50_150", "p100_30", "p520_1030", "p1030_520", "b35_8_8",
             "far_96_32", "self_64"]


def test_fps_oracle_pinned_by_the_reference_kernel():
    """oracle/metrics_oracle.py `fps` against the reference's OWN furthest_point_sampling kernel and launcher, hipified and
    run on an MI355X (tests/golden/fps_emd.npz, made by tests/golden/make_fps_emd_golden.py): index-exact on every rung of
    the launcher's 1..512 block-size ladder, on lattice clouds (exact arithmetic, ties everywhere: the tie order), on
    clouds with points exactly at, just below and just above the origin-skip threshold, and on scan-like clouds whose
    selection does not depend on multiply-add fusion.  No case is left out."""
    from oracle import metrics_oracle as MO
    g = load("fps_emd")
    assert list(g["meta/fps_cases"]) == [f"{fam}_n{n}" for n in FPS_RUNGS for fam in FPS_FAMILIES]
    for name in g["meta/fps_cases"]:
        xyz, idx = g[f"fps/{name}/xyz"], g[f"fps/{name}/idx"]
        assert xyz.shape[0] == 3 and idx.shape == (3, min(xyz.shape[1], 48))
        for b in range(3):
            assert MO.fps(xyz[b], idx.shape[1]).tolist() == idx[b].tolist(), (name, b)
    # the threshold clouds do hold what they are for: squared norms exactly float32(1e-3), its neighbours and 0, and the
    # reference picks points AT float32(1e-3) (it lies above the double 1e-3) but none below
    t0 = np.float32(1e-3)
    lo, hi = np.nextafter(t0, np.float32(0)), np.nextafter(t0, np.float32(1))
    picked = {float(v): 0 for v in (lo, t0, hi, np.float32(0))}
    for n in FPS_RUNGS[4:]:
        xyz, idx = g[f"fps/thresh_n{n}/xyz"], g[f"fps/thresh_n{n}/idx"]
        for b in range(3):
            mag = (xyz[b, :, 0] * xyz[b, :, 0] + xyz[b, :, 1] * xyz[b, :, 1]) + xyz[b, :, 2] * xyz[b, :, 2]
            assert all((mag == v).any() for v in (lo, t0, hi, np.float32(0))), (n, b)
            for k in idx[b][1:]:
                if float(mag[k]) in picked:
                    picked[float(mag[k])] += 1
    assert picked[float(t0)] > 0 and picked[float(hi)] > 0 and picked[float(lo)] == 0 and picked[0.0] == 0, picked


def test_emd_oracle_pinned_by_the_reference_kernels():
    """oracle/metrics_oracle.py `emd_cost` against the reference's OWN approxmatch + matchcost kernels, hipified and run on an
    MI355X at their <<<32, 512>>> launch (tests/golden/fps_emd.npz).  Per pair the fixture holds the reference's cost, the
    same algorithm in float64 and e_ref = |reference - float64|; the float32 restatement must lie within
    2 * e_ref + 1e-6 * |cost| of the float64 value (the 2x: its own float32 rounding, in another order, beside the
    reference's), and in float64 it must reproduce the recorded float64 value to 1e-12 relative.
    The float32 restatement follows the kernels' order of operations and fused multiply-adds (oracle/metrics_oracle.py
    `emd_costs`): the approximation is ill-conditioned on isolated points, and a float32 evaluation in any other order
    lies further from the kernels than they lie from float64 (unfused, BLAS-ordered sums and np.exp: p64_64[1] at
    3.0e-6 against its bound of 2.2e-6, e_ref 3.65e-7 on a cost of 1.4651).  As it stands it is within 3 ulp of the
    recorded reference cost on every pair, and the largest |oracle32 - f64| / bound is 0.48."""
    from oracle import metrics_oracle as MO
    g = load("fps_emd")
    assert list(g["meta/emd_cases"]) == EMD_CASES
    pairs = [(name, g[f"emd/{name}/a"][i], g[f"emd/{name}/b"][i], g[f"emd/{name}/f64"][i], g[f"emd/{name}/e_ref"][i])
             for name in EMD_CASES for i in range(g[f"emd/{name}/a"].shape[0])]
    A, B = g["emd/mat64/a"], g["emd/mat64/b"]
    pairs += [("mat64", A[i], B[j], g["emd/mat64/f64"][i, j], g["emd/mat64/e_ref"][i, j]) for i in range(3) for j in range(4)]
    bad = []
    for name, a, b, f64, e_ref in pairs:
        got64 = MO.emd_cost(a, b, dtype=np.float64)
        assert abs(got64 - f64) <= 1e-12 * abs(f64), (name, got64, f64)
        got32 = MO.emd_cost(a, b)
        print(name, "f64", f64, "e_ref", e_ref, "|oracle32 - f64|", abs(got32 - f64))
        if not abs(got32 - f64) <= 2.0 * e_ref + 1e-6 * abs(f64):
            bad.append((name, got32, f64, e_ref))
    assert not bad, bad


def test_oracle_matches_reference_at_full_width():
    """The benchmark's width - 64x1024, 512 latent, channels 64..512 (BASELINE configs 2-4), dusty2, B = 2, one step -
    as the REFERENCE's modules computed it (tests/golden/make_golden.py full): parameters and inputs are regenerated
    from the fixture's seed (280 MB of weights do not fit a fixture), the expectations are digests - three float64
    statistics and a strided 2048-element sample per tensor - of every output, logit, R1 gradient, parameter gradient
    and updated parameter.  Pins oracle == reference beyond the toy nets of the step_* fixtures."""
    from tests.golden_util import check_digest, full_case
    g = load("full_dusty2")
    if str(g["meta/torch"]) != torch.__version__:
        pytest.skip(f"fixture made with torch {g['meta/torch']}: the regenerated inputs need the same CPU generator")
    G, D, pol, mask, rand = full_case(g)
    G_ema = {k: v.clone() for k, v in G.items()}
    x_real, _ = O.fetch_reals(pol, mask)
    check_digest(g, "x_real", x_real, 1e-6)
    cfg = O.StepConfig(arch=str(g["meta/arch"]), ema_decay=float(g["meta/ema_decay"]))
    sc, ex = O.train_step(G, D, G_ema, O.new_optim_state(G), O.new_optim_state(D), 1, cfg, x_real, rand,
                          return_grads=True)
    for k, v in sub(g, "scalar").items():
        assert abs(sc[k] - float(v)) <= 1e-5 * max(1.0, abs(float(v))), (k, sc[k], float(v))
    tol = 1e-4
    for k, v in ex["synth"].items():
        if k == "mask":
            from tests.golden_util import digest
            stats, sample = digest(v)
            assert abs(stats[0] - g["synth/mask/stats"][0]) <= 2, "hard masks differ in more than two pixels"
            assert (sample != g["synth/mask/sample"]).mean() <= 1e-3
        else:
            check_digest(g, f"synth/{k}", v, tol)
    for key in ("x_real_aug", "x_fake_aug"):
        check_digest(g, key, ex[key], tol)
    check_digest(g, "r1_grads", ex["r1_grads"], tol)
    for key in ("y_real", "y_fake", "y_fake2"):
        assert rel_l2(ex[key], g[key]) <= tol, key
    for k, v in ex["grad_D"].items():
        check_digest(g, f"grad_D/{k}", v, tol, "grad_D")
    for k, v in ex["grad_G"].items():
        check_digest(g, f"grad_G/{k}", v, tol, "grad_G")
    for tag, net in (("G", G), ("D", D), ("G_ema", G_ema)):
        for k, v in net.items():
            check_digest(g, f"after/{tag}/{k}", v, tol, tag)


def test_bf16_emulating_oracle_within_the_reference_autocast_yardstick():
    """What bfloat16 costs the REFERENCE ITSELF at the benchmark's width: tests/golden/full_dusty2_autocast.npz is the step of
    full_dusty2.npz - same parameters, inputs, noise, DiffAugment draws - with the reference trainer's `enable_amp` regions
    (trainers/dcgan_amp.py:194-211,228-232,253-264) under torch.autocast("cpu", bfloat16), made by `make_golden.py autocast`
    from the reference's own modules.  Its per-tensor distance from the fp32 digests is the yardstick for the timed mode's
    checker: the oracle's bf16-EMULATING mode (StepConfig(emulate_bf16=True): rounding exactly where the engine stores
    bfloat16) must deviate from the reference's fp32 results by no more than the reference's own autocast does (x 1.5), tensor
    by tensor - and by more than fp32 noise, or the emulation is not switched on.  (Round-5 review, item 4: until now the
    timed mode's bounds were anchored to the builder's emulation only.)"""
    from tests.golden_util import full_case, sample_dev
    g, ga = load("full_dusty2"), load("full_dusty2_autocast")
    if str(g["meta/torch"]) != torch.__version__:
        pytest.skip(f"fixture made with torch {g['meta/torch']}: the regenerated inputs need the same CPU generator")
    assert str(ga["meta/autocast"]) == "bfloat16" and int(ga["meta/seed"]) == int(g["meta/seed"])
    for j in range(4):            # the two fixtures are ONE experiment: identical draws
        for k in ("u_b", "u_c", "t_h", "t_w", "o_x", "o_y"):
            assert np.array_equal(g[f"aug{j}/{k}"], ga[f"aug{j}/{k}"]), (j, k)
    ref_dev = {k[:-7]: rel_l2(ga[k], g[k]) for k in g.files if k.endswith("/sample") and k in ga.files}
    assert 5e-2 < ref_dev["r1_grads"] < 0.2 and 1e-3 < ref_dev["synth/depth_orig"] < 2e-2     # (what the fixture measured)
    G, D, pol, mask, rand = full_case(g)
    G_ema = {k: v.clone() for k, v in G.items()}
    x_real, _ = O.fetch_reals(pol, mask)
    cfg = O.StepConfig(arch=str(g["meta/arch"]), ema_decay=float(g["meta/ema_decay"]), emulate_bf16=True)
    sc, ex = O.train_step(G, D, G_ema, O.new_optim_state(G), O.new_optim_state(D), 1, cfg, x_real, rand, return_grads=True)
    report = {}
    for key, t in ([("synth/depth_orig", ex["synth"]["depth_orig"]), ("synth/confidence", ex["synth"]["confidence"]),
                    ("r1_grads", ex["r1_grads"])]
                   + [(f"grad_D/{k}", v) for k, v in ex["grad_D"].items()] + [(f"grad_G/{k}", v) for k, v in ex["grad_G"].items()]):
        dev = sample_dev(g, key, t)
        if t.numel() <= 4:
            # a head's bias gradient is ONE number: the sum of 131 072 signed per-pixel gradients that cancel to ~1e-3 of their
            # absolute sum - its relative error measures where each implementation rounds inside that sum, not the layer
            # (tests/test_gpu_configs.py holds it to its own documented bound)
            continue
        report[key] = (dev, ref_dev[key])
        assert dev <= 1.5 * ref_dev[key], (key, dev, ref_dev[key])
        assert dev >= 1e-4, (key, dev, "the emulation rounds nothing?")
    for k in ("loss/D/adversarial", "loss/D/gradient_penalty", "loss/G/adversarial"):
        d_ref = abs(float(ga[f"scalar/{k}"]) - float(g[f"scalar/{k}"]))
        assert abs(sc[k] - float(g[f"scalar/{k}"])) <= 1.5 * d_ref + 1e-4, (k, sc[k], float(g[f"scalar/{k}"]), d_ref)
    worst = max(report.items(), key=lambda kv: kv[1][0] / kv[1][1])
    print("emulating oracle vs reference autocast, worst ratio:", worst[0], "%.3e / %.3e" % worst[1])


def test_cov_mmd_1nna_oracle_pinned_by_the_reference_functions():
    """oracle/metrics_oracle.py `cov_mmd`, `nna` and `compute_cov_mmd_1nna` against what the reference's own
    `_compute_cov_mmd` / `_compute_nna` / `compute_cov_mmd_1nna` (utils/metrics/cov_mmd_1nna.py:55-148, loaded by path, its
    Chamfer distance = its own CPU `nnsearch`) returned: tests/golden/covmmd.npz, made by make_golden.py covmmd.  Crafted
    matrices with ties, k = 1 and 3, sqrt on and off; then clouds end to end incl. the three pairwise matrices.
    (FPS and EMD exist in the reference only as CUDA sources - furthest_point_sampling.cu, earth_mover_distance.cu - and
    are pinned by tests/golden/fps_emd.npz, recorded from those kernels built for gfx950.)"""
    from oracle import metrics_oracle as MO
    g = load("covmmd")
    for tag in ("rand", "ties", "wide"):
        M_rr, M_rg, M_gg = (torch.from_numpy(g[f"mat/{tag}/{k}"]) for k in ("M_rr", "M_rg", "M_gg"))
        for k, v in MO.cov_mmd(M_rg).items():
            assert abs(v - float(g[f"mat/{tag}/covmmd/{k}"])) <= 1e-6, (tag, k)
        for kk, sq in ((1, False), (3, False), (1, True)):
            for k, v in MO.nna(M_rr, M_rg, M_gg, k=kk, sqrt=sq).items():
                assert abs(v - float(g[f"mat/{tag}/nna_k{kk}_sqrt{int(sq)}/{k}"])) <= 1e-6, (tag, kk, sq, k)
    ref, gen = g["pcs_ref"], g["pcs_gen"]
    assert rel_l2(MO.pairwise_cd(ref, gen), g["e2e_mat/M_rg"]) < 1e-6
    assert rel_l2(MO.pairwise_cd(ref, ref), g["e2e_mat/M_rr"]) < 1e-6
    assert rel_l2(MO.pairwise_cd(gen, gen), g["e2e_mat/M_gg"]) < 1e-6
    got = MO.compute_cov_mmd_1nna(gen, ref)
    want = sub(g, "e2e", as_torch=False)
    assert set(got) == set(want)
    for k, v in want.items():
        assert abs(got[k] - float(v)) <= 1e-6 * max(1.0, abs(float(v))), (k, got[k], float(v))
