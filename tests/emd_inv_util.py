"""Shared pieces of the EMD-inversion tests (tests/golden/emd_inversion.npz, made by
tests/golden/make_emd_inversion_golden.py): the cases, the targets (built from an integer hash on a 2^-14 grid, so the
fixture stores seeds and results only), the restatement of the reference's EarthMoverDistanceFunction
(utils/metrics/distance/emd/earth_mover_distance.py:16-32) as a torch.autograd.Function over tests/emd_grad_util, and a
float64 furthest-point selection that reports how close its closest decision was."""
import numpy as np
import torch

from tests import chamfer_inv_util as CU
from tests import emd_grad_util as EU

H, W = 32, 64
HW = H * W
# (case name, arch, distance, K, the case of chamfer_inversion.npz whose generator, Gumbel noise, latent and perturbations it
# runs, the LiDAR's max_depth).  At 120 m the sampler takes no point nearer than 3.8 m, so the targets lie at 4 m .. 21 m, far
# from what the fixture generators emit (1.4 m .. 2.5 m).  The Chamfer searches keep their margin only between clouds that
# overlap, so the case with a Chamfer term has its target in the generators' range, seen by a LiDAR of 20 m - where that range
# holds candidates (0.9 m / 20 m squared is 2e-3).
CASES = (("none_emd", "none", ("emd",), 64, "none_chamfer", 120.0),
         ("dusty1_emd", "dusty1", ("emd",), 64, "dusty1_chamfer", 120.0),
         ("dusty2_emd", "dusty2", ("emd",), 700, "dusty2_chamfer", 120.0),
         ("dusty2_l1_emd", "dusty2", ("l1", "emd"), 64, "dusty2_chamfer", 120.0),
         ("dusty2_chamfer_emd", "dusty2", ("chamfer", "emd"), 64, "dusty2_chamfer", 20.0))
SINGLE = tuple(c for c in CASES if c[2] == ("emd",))
FPS_MARGIN = 2.0 ** -18   # the relative gap every furthest-point decision keeps (the Chamfer fixture's search margin)


def target(seeds, max_depth=120.0):
    """(inv_ref [B,1,H,W], mask) float32 of the per-scan seeds: inverse depth on a 2^-14 grid, a fifth of the rays dropped -
    0.035 .. 0.215 (4 m .. 21 m at 0.9 / 120 m) for the 120 m LiDAR, 0.35 .. 0.65 (the fixture generators' range) otherwise:
    either way every kept pixel is a furthest-point candidate.  Scan 0's pixel 0 is dropped (the sampler's first index is then
    an origin point), scan 1's is kept."""
    lo, n = (573, 2950) if max_depth == 120.0 else (5734, 4916)
    inv, mask = [], []
    for b, seed in enumerate(seeds):
        w = CU._hash(int(seed), HW)
        q = np.uint32(lo) + (w[:, 0] >> np.uint32(8)) % np.uint32(n)               # 573 / 2^14 = 0.035, 3522 / 2^14 = 0.215
        keep = ((w[:, 1] >> np.uint32(8)) % np.uint32(5) != 0).astype(np.float32)
        if b == 0:
            keep[0] = 0.0
        elif b == 1:
            keep[0] = 1.0
        inv.append(q.astype(np.float32) * np.float32(2.0 ** -14) * keep)
        mask.append(keep)
    shape = (len(seeds), 1, H, W)
    return torch.from_numpy(np.stack(inv)).view(shape), torch.from_numpy(np.stack(mask)).view(shape)


def target_points(inv_ref, dtype=torch.float32, max_depth=120.0):
    """the target's point map [B,HW,3] in `dtype` through oracle.lidar_oracle.inv_to_xyz (Coordinate.inv_to_xyz) on
    chamfer_inv_util's angle grid"""
    from oracle import lidar_oracle as LO
    angle = CU.angle_grid(H, W).to(dtype)
    return CU.flatten(LO.inv_to_xyz(inv_ref.to(dtype), angle, CU.MIN_DEPTH, max_depth, 0.0, CU.TOL))


def candidates(points32):
    """[B] the furthest-point candidates per scan: float32 |p|^2 > 1e-3 (the double literal: oracle.metrics_oracle.fps)"""
    p = points32.numpy().astype(np.float32)
    mag = (p[..., 0] * p[..., 0]) + (p[..., 1] * p[..., 1]) + (p[..., 2] * p[..., 2])
    return (mag.astype(np.float64) > 1e-3).sum(axis=1)


def fps_margin(points64, points32, m):
    """furthest-point selection of one cloud [n,3] in float64 (candidates by the float32 rule) -> (idx [m], the smallest
    relative gap (best - runner-up) / best over its m - 1 decisions).  With every gap above the float32 rounding of the
    distances the selection does not depend on the tie rule."""
    x = np.asarray(points64, np.float64)
    p = np.asarray(points32, np.float32)
    mag = (p[:, 0] * p[:, 0]) + (p[:, 1] * p[:, 1]) + (p[:, 2] * p[:, 2])
    cand = mag.astype(np.float64) > 1e-3
    temp = np.full(x.shape[0], 1e10)
    idx = np.zeros(m, np.int64)
    gap, old = np.inf, 0
    for j in range(1, m):
        d = ((x - x[old]) ** 2).sum(axis=1)
        temp = np.where(cand, np.minimum(d, temp), -1.0)
        old = int(np.argmax(temp))
        best = temp[old]
        second = np.partition(temp, -2)[-2]
        gap = min(gap, (best - second) / best if best > 0 else 0.0)
        idx[j] = old
    return idx, gap


class EmdFn(torch.autograd.Function):
    """The reference's EarthMoverDistanceFunction on the CPU.  xyz1 [B,n,3], xyz2 [B,m,3] -> cost [B]: approxmatch and matchcost
    as tests/emd_grad_util restates them (float32 tensors: the kernels' order of sums; float64: the same algorithm), the
    backward matchcostgrad1 / matchcostgrad2 over the SAVED match - a constant, as in the reference.
    frozen: a match [B,n,m] to use instead of approxmatch's (the self-check: the cost is then quadratic in the points).
    record: a list that receives (xyz1, xyz2) of every forward."""
    frozen = None
    record = None

    @staticmethod
    def forward(ctx, xyz1, xyz2):
        a, b = xyz1.detach().numpy(), xyz2.detach().numpy()
        if EmdFn.record is not None:
            EmdFn.record.append((a.copy(), b.copy()))
        if EmdFn.frozen is None:
            match, d2 = EU.approxmatch(a, b, a.dtype)
            cost = EU.matchcost(match, d2)
        else:
            match = np.asarray(EmdFn.frozen)
            diff = a[:, :, None, :].astype(np.float64) - b[:, None, :, :].astype(np.float64)
            cost = (match * (diff * diff).sum(axis=3)).sum(axis=(1, 2))
        ctx.save_for_backward(xyz1, xyz2, torch.from_numpy(np.ascontiguousarray(match)))
        return torch.from_numpy(np.asarray(cost)).to(xyz1.dtype)

    @staticmethod
    def backward(ctx, grad_cost):
        xyz1, xyz2, match = ctx.saved_tensors
        g1, g2 = EU.match_grads(xyz1.detach().numpy(), xyz2.detach().numpy(), match.numpy(), grad_cost.detach().numpy())
        return torch.from_numpy(g1).to(xyz1.dtype), torch.from_numpy(g2).to(xyz2.dtype)


def fixture_case(g, gc, name):
    """(params, gumbel, inv_ref, mask, latent0, noise [S,B,nz], num_step, idx [B,K], max_depth) of case `name`: g = emd_inversion.npz,
    gc = chamfer_inversion.npz (the generator, Gumbel noise, latent and perturbations, by name)"""
    params, gumbel, _, _, latent0, noise, S = CU.fixture_case(gc, str(g[name + "/meta/inputs"]))
    max_depth = float(g[name + "/meta/max_depth"])
    inv_ref, mask = target(g[name + "/meta/target_seeds"].tolist(), max_depth)
    idx = torch.from_numpy(g[name + "/idx"].astype(np.int64))
    return params, gumbel, inv_ref, mask, latent0, noise, int(g[name + "/meta/num_step"]), idx, max_depth
