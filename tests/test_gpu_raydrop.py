"""The three ray-drop kernels (csrc/raydrop.hip: dg_pixel_winner, dg_raydrop_keep, dg_raydrop_gather) on the GPU against their
NumPy restatements (tests/raydrop_util.py), every comparison exact.  The kernels do not depend on the engine's H >= 32: the
LiDAR is a nominal angle grid at 8 x 48 (below one export chunk, H W no multiple of 256, the 4-pixel stores) and 7 x 331 (2317
pixels: three export chunks, the last one partial, H W no multiple of 4: the element-wise stores).  B = 3 clouds of different
length, one of them empty, about 10 points per pixel, a few exact duplicates."""
import functools

import numpy as np
import pytest
import torch

from tests import philox_ref as P
from tests import raydrop_util as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = [(8, 48), (7, 331)]
IDS = ["8x48", "7x331"]
MIN_DEPTH, MAX_DEPTH = 1.45, 80.0
B = 3
SEED = 0x5EED0123456789


def host(t):
    return t.detach().cpu().numpy()


def make_lidar(H, W):
    from dusty_gan_amd.utils.lidar import LiDAR
    return LiDAR(H, W, MIN_DEPTH, MAX_DEPTH).use_nominal_angles().to(torch.device(DEV))


def make_points(rng, n):
    """n unit-space points inside the field of view on raydrop_util's lattice, column 3 = the point's id"""
    yaw = rng.uniform(-np.pi, np.pi, n)
    pitch = np.radians(rng.uniform(-24.0, 1.5, n))
    r = rng.uniform(0.03, 0.97, n)
    xyz = np.stack([r * np.cos(pitch) * np.cos(yaw), r * np.cos(pitch) * np.sin(yaw), r * np.sin(pitch)], axis=1)
    return np.concatenate([R.quantise(xyz), np.arange(n, dtype=np.float32)[:, None]], axis=1)


@functools.lru_cache(maxsize=None)
def case(H, W):
    """the clouds of one size, their projection's idx (the GPU's: dg_points_to_depth is tested on its own) and the winner's
    restatement - made once, shared by the tests, never modified"""
    from dusty_gan_amd import raydrop
    HW = H * W
    N = 10 * HW
    rng = np.random.default_rng(HW)
    rec = np.zeros((B, N, 4), dtype=np.float32)
    counts = np.array([N, 0, N - 3 * HW], dtype=np.int32)      # cloud 1 is empty; cloud 2 is shorter
    for b in (0, 2):
        rec[b, :counts[b]] = make_points(rng, counts[b])
        src, dst = rng.choice(counts[b], (2, 40), replace=False)
        rec[b, dst, :3] = rec[b, src, :3]                      # exact duplicates (their ids stay their own)
    rec[1] = make_points(rng, N)                               # records behind counts[1] = 0: never read
    lidar = make_lidar(H, W)
    rec_d, counts_d = torch.from_numpy(rec).to(DEV), torch.from_numpy(counts).to(DEV)
    depth, valid, idx = lidar.points_to_depth(rec_d, counts=counts_d, return_index=True)
    idx_h = host(idx)
    want = R.winner(rec, idx_h, counts, HW)
    assert (want[1] == -1).all() and (want[0] >= 0).mean() > 0.9 and (want[2] >= 0).mean() > 0.9
    win = raydrop.pixel_winner(rec_d, idx, counts_d, H, W)
    return {"H": H, "W": W, "HW": HW, "N": N, "rec": rec, "counts": counts, "rec_d": rec_d, "counts_d": counts_d, "idx": idx,
            "idx_h": idx_h, "want_win": want, "win": win, "lidar": lidar}


# ---- winner -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES, ids=IDS)
def test_winner_equals_the_restatement(H, W):
    from dusty_gan_amd import raydrop
    from dusty_gan_amd.utils.render import _workspace
    c = case(H, W)
    got = host(c["win"])
    assert got.dtype == np.int32 and np.array_equal(got, c["want_win"])
    # ties were met: some pixel's winner has a duplicate of the same range binned into the same pixel
    r = R.ranges(c["rec"][0])
    tied = 0
    for p in np.nonzero(c["want_win"][0] >= 0)[0][:: max(1, c["HW"] // 400)]:
        mates = np.nonzero((c["idx_h"][0] == p) & (r == r[c["want_win"][0, p]]))[0]
        tied += len(mates) > 1
        assert mates.min() == c["want_win"][0, p]
    print(f"{H}x{W}: {tied} sampled pixels decided by the index")
    # the workspace words are zero again, and the same call gives the same bits
    ws = _workspace(c["rec_d"].device, B * c["HW"])
    assert not bool(ws.any())
    again = raydrop.pixel_winner(c["rec_d"], c["idx"], c["counts_d"], H, W)
    assert torch.equal(again, c["win"]) and not bool(ws.any())
    # stride 3 reads the same coordinates
    win3 = raydrop.pixel_winner(c["rec_d"][:, :, :3].contiguous(), c["idx"], c["counts_d"], H, W)
    assert torch.equal(win3, c["win"])


@pytest.mark.parametrize("H,W", SIZES, ids=IDS)
def test_winning_record_survives_a_permutation(H, W):
    """with distinct ranges the winner of a pixel is one record, wherever it lies in the cloud"""
    from dusty_gan_amd import raydrop
    c = case(H, W)
    rec = c["rec"][0]
    _, first = np.unique(R.ranges(rec), return_index=True)
    rec = rec[np.sort(first)]                                  # one point per float32 range: no ties anywhere
    perm = np.random.default_rng(7).permutation(len(rec))
    both = torch.from_numpy(np.stack([rec, rec[perm]])).to(DEV)
    _, _, idx = c["lidar"].points_to_depth(both, return_index=True)
    win = host(raydrop.pixel_winner(both, idx, None, H, W))
    assert np.array_equal(win[0] >= 0, win[1] >= 0) and (win[0] >= 0).mean() > 0.9
    hit = win[0] >= 0
    a, b = rec[win[0][hit]], rec[perm][win[1][hit]]
    assert np.array_equal(R.bits(a), R.bits(b))
    assert not np.array_equal(win[0][hit], win[1][hit])       # (the indices did move)


# ---- keep ---------------------------------------------------------------------------------------------------------------------------
def clear_of_zero(x, margin=1e-3):
    """push the float32 values within `margin` of zero out to +-2 margin"""
    x = x.astype(np.float32)
    near = np.abs(x) < margin
    x[near] = np.where(x[near] < 0, -2 * margin, 2 * margin).astype(np.float32)
    return x


def logits_clear_of(noise, rng, C, H, W):
    """conf [B,C,H,W] such that |h1 + noise_k| >= 1e-3 for every realisation k and |h2| >= 1e-3: there the kernel's rule
    (head_px_fwd: 1 / (1 + __expf(-l / tau)) > 0.5, tau in [1, 2]) and the restatement's l > 0 provably agree - for l >= 1e-3 the
    exponential is at most e^-0.0005 (1 + 2^-20) < 1, so the sigmoid exceeds 1/2, and the mirror image for l <= -1e-3 - and no
    pixel is excused"""
    conf = (rng.normal(size=(B, C, H, W)) * 2).astype(np.float32)
    for _ in range(8):
        s = conf[:, None, 0] + noise[:, :, 0]
        bad = (np.abs(s) < 1e-3).any(axis=1)
        if not bad.any():
            break
        conf[:, 0][bad] += np.float32(0.0137)
    assert (np.abs(conf[:, None, 0] + noise[:, :, 0]) >= 1e-3).all()
    if C == 2:
        conf[:, 1] = clear_of_zero(conf[:, 1])
    return conf


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("H,W", SIZES, ids=IDS)
def test_keep_with_injected_noise(H, W, C, K):
    from dusty_gan_amd import raydrop
    c = case(H, W)
    rng = np.random.default_rng(100 * C + K)
    u = rng.uniform(1e-6, 1 - 1e-6, (B, K, 1, H, W))
    noise = np.log(u / (1 - u)).astype(np.float32)
    conf = logits_clear_of(noise, rng, C, H, W)
    want = R.keep(conf, c["want_win"], noise)
    for tau in (1.0, 2.0):
        got, used = raydrop.sample_keep(torch.from_numpy(conf).to(DEV), c["win"], f"dusty{C}", tau, realisations=K,
                                        noise=torch.from_numpy(noise).to(DEV), return_noise=True)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (B, K, H, W)
        assert np.array_equal(host(got), want), (tau, int((host(got) != want).sum()))
        assert np.array_equal(R.bits(host(used)), R.bits(noise))
    assert 0.15 < want[0].mean() < 0.8 and not want[1].any()
    if K == 3:
        assert (want[0, 0] != want[0, 1]).any()


def philox_noise(HW, first_index, nb, K):
    """the documented layout: scan first_index + b, realisation k = the logistic draw of HW elements at counter offset
    (first_index + b) 2 ceil(HW / 4) of stream word (15 | k << 32) -> float64 [nb,K,HW]"""
    from dusty_gan_amd.raydrop import STREAM_RAYDROP
    assert STREAM_RAYDROP == 15
    n4 = P.groups(HW)
    return np.stack([np.stack([P.logistic(SEED, STREAM_RAYDROP | (k << 32), (first_index + b) * 2 * n4, HW) for k in range(K)])
                     for b in range(nb)])


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("H,W", SIZES, ids=IDS)
def test_keep_with_philox_noise(H, W, C):
    from dusty_gan_amd import raydrop
    c = case(H, W)
    HW, K = c["HW"], 4
    rng = np.random.default_rng(5 + C)
    any_conf = torch.zeros(B, C, H, W, device=DEV)
    _, drawn = raydrop.sample_keep(any_conf, c["win"], f"dusty{C}", 1.0, realisations=K, seed=SEED, first_index=3, return_noise=True)
    noise = host(drawn)
    # (a) the numbers: the host generator at the documented counters, within dg_logistic_noise's bound
    want = philox_noise(HW, 3, B, K)
    got = noise.reshape(B, K, HW).astype(np.float64)
    assert np.isfinite(got).all()
    ratio = float((np.abs(got - want) / P.logistic_bound(want)).max())
    print(f"{H}x{W} C{C}: worst error {ratio:.3f} of the bound")
    assert ratio <= 1.0
    # (b) keep = the rule on the RETURNED noise (the noise does not depend on the logits: these are chosen clear of it)
    conf = logits_clear_of(noise, rng, C, H, W)
    conf_d = torch.from_numpy(conf).to(DEV)
    keep, again = raydrop.sample_keep(conf_d, c["win"], f"dusty{C}", 1.0, realisations=K, seed=SEED, first_index=3, return_noise=True)
    assert torch.equal(again, drawn)
    assert np.array_equal(host(keep), R.keep(conf, c["want_win"], noise))
    # (c) scan 5 alone = row 2 of the batch that starts at scan 3
    alone, n1 = raydrop.sample_keep(conf_d[2:3], c["win"][2:3], f"dusty{C}", 1.0, realisations=K, seed=SEED, first_index=5,
                                    return_noise=True)
    assert torch.equal(n1[0], drawn[2]) and torch.equal(alone[0], keep[2]) and bool(alone.any())
    # (d) realisation 1 of K = 2 = realisation 1 of K = 4
    two, n2 = raydrop.sample_keep(conf_d, c["win"], f"dusty{C}", 1.0, realisations=2, seed=SEED, first_index=3, return_noise=True)
    assert torch.equal(n2, drawn[:, :2]) and torch.equal(two, keep[:, :2])
    # another seed, another field
    other = raydrop.sample_keep(conf_d, c["win"], f"dusty{C}", 1.0, realisations=K, seed=SEED + 1, first_index=3)
    assert not torch.equal(other, keep)


# ---- gather -------------------------------------------------------------------------------------------------------------------------
SENTINEL = 0x7FC0BEEF   # (a NaN's bits as a float)


@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("H,W", SIZES, ids=IDS)
def test_gather(H, W, stride):
    from dusty_gan_amd import raydrop
    c = case(H, W)
    HW, N, K = c["HW"], c["N"], 3
    rng = np.random.default_rng(11)
    keep = (rng.uniform(size=(B, K, H, W)) < np.array([0.5, 0.9, 0.0])[None, :, None, None]).astype(np.uint8)
    keep[1, 0] = 1                                             # kept pixels of the EMPTY cloud: nothing comes out
    keep[2, 1] = 1                                             # everything that has a winner
    rec = np.ascontiguousarray(c["rec"][:, :, :stride]) * np.float32(MAX_DEPTH)   # "metres": ANY buffer of the layout
    labels = rng.integers(0, 2 ** 32, (B, N), dtype=np.int64)
    want = R.gather(rec, c["want_win"], keep, labels)
    out = (torch.full((B, K, HW, 4), float("nan"), device=DEV), torch.full((B, K, HW), SENTINEL, dtype=torch.int32, device=DEV),
           torch.full((B, K, HW), SENTINEL, dtype=torch.int32, device=DEV))
    out[0].view(torch.int32).fill_(SENTINEL)
    args = (torch.from_numpy(rec).to(DEV), c["win"], torch.from_numpy(keep).to(DEV), torch.from_numpy(labels).to(DEV))
    got_rec, got_lab, got_idx, got_cnt = raydrop.gather(*args, out=out)
    cnt = host(got_cnt)
    assert np.array_equal(cnt, (keep.reshape(B, K, HW) & (c["want_win"][:, None] >= 0)).sum(axis=2))
    assert cnt[1].tolist() == [0, 0, 0] and cnt[:, 2].tolist() == [0, 0, 0] and cnt[2, 1] == (c["want_win"][2] >= 0).sum()
    g_rec, g_lab, g_idx = host(got_rec).view(np.int32), host(got_lab), host(got_idx)
    for (b, k), (w_rec, w_lab, w_idx) in want.items():
        n = int(cnt[b, k])
        assert n == len(w_idx)
        assert np.array_equal(g_rec[b, k, :n], R.bits(w_rec)), (b, k)
        assert np.array_equal(g_lab[b, k, :n].view(np.uint32), w_lab), (b, k)
        assert np.array_equal(g_idx[b, k, :n], w_idx), (b, k)
        assert (g_rec[b, k, n:] == SENTINEL).all() and (g_lab[b, k, n:] == SENTINEL).all() and (g_idx[b, k, n:] == SENTINEL).all()
    # without labels, fresh outputs, twice: the same bytes
    r1, l1, i1, c1 = raydrop.gather(args[0], args[1], args[2])
    r2, _, i2, c2 = raydrop.gather(args[0], args[1], args[2])
    assert l1 is None and torch.equal(c1, got_cnt) and torch.equal(c1, c2)
    for b in range(B):
        for k in range(K):
            n = int(cnt[b, k])
            assert torch.equal(r1[b, k, :n].view(torch.int32), r2[b, k, :n].view(torch.int32)) and torch.equal(i1[b, k, :n], i2[b, k, :n])
            assert np.array_equal(host(r1[b, k, :n]).view(np.int32), g_rec[b, k, :n])


def test_argument_checks():
    from dusty_gan_amd import raydrop
    c = case(8, 48)
    conf = torch.zeros(B, 1, 8, 48, device=DEV)
    with pytest.raises(RuntimeError, match="GPU only"):
        raydrop.pixel_winner(c["rec_d"].cpu(), c["idx"], None, 8, 48)
    with pytest.raises(RuntimeError, match="GPU only"):
        raydrop.sample_keep(conf.cpu(), c["win"], "dusty1", 1.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        raydrop.gather(c["rec_d"].cpu(), c["win"], torch.ones(B, 1, 8, 48, dtype=torch.uint8))
    with pytest.raises(ValueError, match="nothing to transfer"):
        raydrop.sample_keep(conf, c["win"], "none", 1.0)
    with pytest.raises(ValueError, match="labels"):
        raydrop.gather(c["rec_d"], c["win"], torch.ones(B, 1, 8, 48, dtype=torch.uint8, device=DEV),
                       torch.zeros(B, c["N"] - 1, dtype=torch.int64, device=DEV))
