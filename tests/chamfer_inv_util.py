"""Shared pieces of the Chamfer-inversion tests (tests/golden/chamfer_inversion.npz, made by
tests/golden/make_chamfer_inversion_golden.py): the stand-alone cloud pairs of the nearest-neighbour search (built from an
integer hash, so the fixture stores their float64 matches only), the synthetic angle grid, the float64 brute-force search
and the restatement of the reference's Chamfer extension (nnsearch and backward, chamfer_distance.cpp:39-62,82-140) as a
torch.autograd.Function."""
import math

import numpy as np
import torch

MIN_DEPTH, MAX_DEPTH, TOL = 0.9, 120.0, 1e-8
ARCHS = ("none", "dusty1", "dusty2")
# (case name, arch, distance)
CASES = (("none_chamfer", "none", ("chamfer",)), ("dusty1_chamfer", "dusty1", ("chamfer",)),
         ("dusty2_chamfer", "dusty2", ("chamfer",)), ("dusty2_l1_chamfer", "dusty2", ("l1", "chamfer")))
# stand-alone search pairs: name -> (n, m)
RANDOM_PAIRS = {"p1_1": (1, 1), "p7_513": (7, 513), "p512_512": (512, 512), "p513_1500": (513, 1500),
                "p2048_700": (2048, 700), "p1500_2048": (1500, 2048)}
DYADIC, ORIGIN = ("dyadic", (700, 1100)), ("origin", (1000, 1300))
PAIR_NAMES = tuple(RANDOM_PAIRS) + (DYADIC[0], ORIGIN[0])


def _hash(seed, n):
    """n x 3 32-bit words of an integer hash (splitmix64's finaliser) of (seed, index): the same on every platform"""
    with np.errstate(over="ignore"):
        k = np.arange(n * 3, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        k = (k ^ (k >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        k = (k ^ (k >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    k = k ^ (k >> np.uint64(31))
    return (k >> np.uint64(32)).astype(np.uint32).reshape(n, 3)


def cloud(seed, n):
    """n float32 points inside the unit ball: the cube [-1,1]^3 / sqrt(3), coordinates on a 2^-23 grid times 0.577"""
    u = (_hash(seed, n) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)   # exact
    return torch.from_numpy((u * np.float32(0.577)).astype(np.float32))


def dyadic_cloud(seed, n):
    """coordinates k / 8, k = -4 .. 3: every difference, square and sum is exact in float32; 512 distinct points, so
    duplicates and exact ties abound"""
    k = (_hash(seed, n) >> np.uint32(29)).astype(np.float32) - np.float32(4.0)
    return torch.from_numpy((k / np.float32(8.0)).astype(np.float32))


def pair(name, seed):
    """the stand-alone pair `name` of the fixture's checked `seed`: (A [n,3], B [m,3]) float32"""
    if name == DYADIC[0]:
        n, m = DYADIC[1]
        return dyadic_cloud(seed, n), dyadic_cloud(seed + 1, m)
    if name == ORIGIN[0]:
        n, m = ORIGIN[1]
        a, b = cloud(seed, n), cloud(seed + 1, m)
        a[::2] = 0.0   # half of both clouds is the origin (dropped pixels)
        b[1::2] = 0.0
        return a, b
    n, m = RANDOM_PAIRS[name]
    return cloud(seed, n), cloud(seed + 1, m)


def angle_grid(H, W):
    """[1,2,H,W] float32: elevation linear over the rows, azimuth linear over the columns (as the LiDAR fixtures)"""
    pitch = torch.linspace(0.05, -0.42, H, dtype=torch.float64)[:, None].expand(H, W)
    yaw = torch.linspace(math.pi, -math.pi, W + 1, dtype=torch.float64)[:W][None, :].expand(H, W)
    return torch.stack([pitch, yaw])[None].float().contiguous()


def sqdist(a, b):
    """[n,m] squared distances, squared differences summed in coordinate order (chamfer_distance.cpp:49-52)"""
    d = a[:, None, :] - b[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nn_first(a, b):
    """nnsearch (chamfer_distance.cpp:39-62) of one pair in the tensors' dtype: (dist [n], idx [n]), the FIRST minimum"""
    d = sqdist(a, b)
    best = d.min(dim=1).values
    ar = torch.arange(b.shape[0]).expand_as(d)
    idx = torch.where(d == best[:, None], ar, torch.full_like(ar, b.shape[0])).min(dim=1).values
    return best, idx


def runner_up_ratio(a, b):
    """per point of a (float64): the distance of the nearest point of b that does NOT coincide with the first minimum's
    point, over the minimum (inf where no such point exists or the ratio is x / 0)"""
    a, b = a.double(), b.double()
    d = sqdist(a, b)
    best, idx = nn_first(a, b)
    same = (b[None, :, :] == b[idx][:, None, :]).all(dim=2)
    second = torch.where(same, torch.full_like(d, float("inf")), d).min(dim=1).values
    return torch.where(best > 0, second / best.clamp_min(1e-300), torch.where(second > 0, torch.full_like(best, float("inf")),
                                                                                 torch.ones_like(best)))


class ChamferFn(torch.autograd.Function):
    """The reference's ChamferDistanceFunction on the CPU: nnsearch both ways, and the backward of
    chamfer_distance.cpp:82-140.  xyz1 [B,n,3], xyz2 [B,m,3] -> dist1 [B,n], dist2 [B,m].  `record`: a list that receives
    (xyz1, xyz2) of every forward (the generator checks the searches' margins on them)."""
    record = None

    @staticmethod
    def forward(ctx, xyz1, xyz2):
        if ChamferFn.record is not None:
            ChamferFn.record.append((xyz1.detach().clone(), xyz2.detach().clone()))
        r1 = [nn_first(x, y) for x, y in zip(xyz1, xyz2)]
        r2 = [nn_first(y, x) for x, y in zip(xyz1, xyz2)]
        d1, i1 = torch.stack([r[0] for r in r1]), torch.stack([r[1] for r in r1])
        d2, i2 = torch.stack([r[0] for r in r2]), torch.stack([r[1] for r in r2])
        ctx.save_for_backward(xyz1, xyz2, i1, i2)
        return d1, d2

    @staticmethod
    def backward(ctx, g1, g2):
        xyz1, xyz2, i1, i2 = ctx.saved_tensors
        gx1, gx2 = torch.zeros_like(xyz1), torch.zeros_like(xyz2)
        for b in range(xyz1.shape[0]):
            t = (2 * g1[b])[:, None] * (xyz1[b] - xyz2[b][i1[b]])
            gx1[b] += t
            gx2[b].index_add_(0, i1[b], -t)
            t = (2 * g2[b])[:, None] * (xyz2[b] - xyz1[b][i2[b]])
            gx2[b] += t
            gx1[b].index_add_(0, i2[b], -t)
        return gx1, gx2


def flatten(t):
    """utils.flatten (utils/__init__.py:213-214)"""
    return t.flatten(2).permute(0, 2, 1).contiguous()


def fixture_case(g, name):
    """(params, gumbel, inv_ref, mask, latent0, noise [S,B,nz], num_step) of case `name`"""
    pre = str(g[name + "/meta/inputs"]) + "/"   # (dusty2's two cases share one generator, target and perturbations)
    params = {k[len(pre) + 7:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre + "init/G/")}
    t = lambda k: torch.from_numpy(g[pre + k])
    mask = torch.from_numpy(np.unpackbits(g[pre + "mask_bits"])[:t("inv_ref").numel()].astype(np.float32)).view_as(t("inv_ref"))
    return params, t("gumbel"), t("inv_ref"), mask, t("latent0"), t("noise"), int(g[name + "/meta/num_step"])
