"""Chamfer distance between sets of point clouds -- reference: utils/metrics/distance/cd/ (CUDA extension) as used by
utils/metrics/cov_mmd_1nna.py:20-52.  The reference evaluates one row of the distance matrix per Python iteration;
here a whole [Na,Nb] matrix of directed means is one launch (csrc/point_chamfer.hip chamfer_dir_kernel).
The two distances are also differentiable, under the reference's names (utils/metrics/distance/__init__.py):
chamfer_distance / ChamferDistanceFunction / ChamferDistance and earth_mover_distance / EarthMoverDistanceFunction /
EarthMoverDistance, with the explicit forms chamfer_backward and earth_mover_distance_grad underneath."""
import torch

from ... import _lib as L


def _prep(pcs):
    assert pcs.ndim == 3 and pcs.size(2) == 3, "expected (B,N,3), but got {}".format(tuple(pcs.shape))
    if not pcs.is_cuda:
        raise RuntimeError("chamfer distance runs on the GPU only (no CPU fallback)")
    return pcs.contiguous().float()


def chamfer_dir(pcs_1, pcs_2):
    """L[i,j] = mean_{p in pcs_1[i]} min_{q in pcs_2[j]} |p - q|^2  -> [B_1,B_2]"""
    a, b = _prep(pcs_1), _prep(pcs_2)
    out = torch.empty(a.size(0), b.size(0), dtype=torch.float32, device=a.device)
    L.check(L.lib().dg_chamfer_dir(L.ptr(a), a.size(0), a.size(1), L.ptr(b), b.size(0), b.size(1), L.ptr(out),
                                   L.stream_ptr()), "dg_chamfer_dir")
    return out


def chamfer_distance_matrix(pcs_1, pcs_2):
    """M[i,j] = compute_cd(pcs_1[i], pcs_2[j]) = dl.mean + dr.mean (cov_mmd_1nna.py:20-22), all pairs"""
    if pcs_1 is pcs_2:
        d = chamfer_dir(pcs_1, pcs_1)
        return d + d.t()
    return chamfer_dir(pcs_1, pcs_2) + chamfer_dir(pcs_2, pcs_1).t()


def chamfer_paired(pcs_1, pcs_2):
    """L[i] = mean_{p in pcs_1[i]} min_{q in pcs_2[i]} |p - q|^2 -> [B] (the diagonal of chamfer_dir, one launch)"""
    a, b = _prep(pcs_1), _prep(pcs_2)
    assert a.size(0) == b.size(0)
    out = torch.empty(a.size(0), dtype=torch.float32, device=a.device)
    L.check(L.lib().dg_chamfer_paired(L.ptr(a), a.size(1), L.ptr(b), b.size(1), a.size(0), L.ptr(out), L.stream_ptr()),
            "dg_chamfer_paired")
    return out


def compute_cd(pcs_1, pcs_2):
    """compute_cd (utils/metrics/cov_mmd_1nna.py:19-21) of paired sets: cloud i against cloud i -> [B]"""
    return chamfer_paired(pcs_1, pcs_2) + chamfer_paired(pcs_2, pcs_1)


def _emd_cost(a, b):
    out = torch.empty(a.size(0), dtype=torch.float32, device=a.device)
    L.check(L.lib().dg_emd(L.ptr(a), a.size(0), a.size(1), L.ptr(b), b.size(0), b.size(1), 1, L.ptr(out),
                           L.stream_ptr()), "dg_emd")
    return out


def earth_mover_distance(xyz1, xyz2):
    """cost[b] of the approximate matching between xyz1[b] and xyz2[b] (reference: utils/metrics/distance/emd/,
    EarthMoverDistanceFunction.forward): approxmatch + matchcost in one kernel (csrc/point_emd.hip emd_kernel).  With an input
    that requires grad the cost is a node of the autograd graph (EarthMoverDistanceFunction); otherwise the launch is the same
    and nothing is recorded."""
    a, b = _prep(xyz1), _prep(xyz2)
    assert a.size(0) == b.size(0)
    if torch.is_grad_enabled() and (a.requires_grad or b.requires_grad):
        return EarthMoverDistanceFunction.apply(a, b)
    return _emd_cost(a, b)


def _pair(xyz1, xyz2):
    """shapes first, for both clouds, then the device: argument errors come before anything is launched"""
    for t in (xyz1, xyz2):
        assert t.ndim == 3 and t.size(2) == 3, "expected (B,N,3), but got {}".format(tuple(t.shape))
    assert xyz1.size(0) == xyz2.size(0), "paired clouds: {} against {}".format(xyz1.size(0), xyz2.size(0))


def earth_mover_distance_grad(xyz1, xyz2, grad_cost=None):
    """(cost [B], grad1 [B,n,3], grad2 [B,m,3]): earth_mover_distance and its gradient times grad_cost [B] (None: ones) in
    one launch (dg_emd_grad), explicit - no autograd.  The reference's EarthMoverDistanceFunction.backward: the match
    matrix is a constant, and here it is never stored.  cost = earth_mover_distance(xyz1, xyz2), bit for bit."""
    _pair(xyz1, xyz2)
    if grad_cost is not None:
        assert grad_cost.ndim == 1 and grad_cost.size(0) == xyz1.size(0), \
            "expected grad_cost ({},), but got {}".format(xyz1.size(0), tuple(grad_cost.shape))
    a, b = _prep(xyz1.detach()), _prep(xyz2.detach())
    gc = None
    if grad_cost is not None:
        if not grad_cost.is_cuda:
            raise RuntimeError("earth mover's distance runs on the GPU only (no CPU fallback)")
        gc = grad_cost.detach().contiguous().float()
    cost = torch.empty(a.size(0), dtype=torch.float32, device=a.device)
    g1, g2 = torch.empty_like(a), torch.empty_like(b)
    L.check(L.lib().dg_emd_grad(L.ptr(a), a.size(1), L.ptr(b), b.size(1), a.size(0), L.ptr(gc), L.ptr(cost), L.ptr(g1),
                                L.ptr(g2), L.stream_ptr()), "dg_emd_grad")
    return cost, g1, g2


class EarthMoverDistanceFunction(torch.autograd.Function):
    """utils/metrics/distance/emd/earth_mover_distance.py:16-32.  forward is dg_emd (what earth_mover_distance launches
    for inputs that need no gradient); backward is one dg_emd_grad launch on the saved clouds, which produces the match
    again instead of reading a saved [B,m,n] matrix."""

    @staticmethod
    def forward(ctx, xyz1, xyz2):
        _pair(xyz1, xyz2)
        a, b = _prep(xyz1), _prep(xyz2)
        ctx.save_for_backward(a, b)
        return _emd_cost(a, b)

    @staticmethod
    def backward(ctx, grad_cost):
        a, b = ctx.saved_tensors
        _, g1, g2 = earth_mover_distance_grad(a, b, grad_cost)
        return g1, g2


class EarthMoverDistance(torch.nn.Module):
    def forward(self, input1, input2, eps=None, iters=None):
        """eps and iters are ignored, as in the reference (earth_mover_distance.py:35-37)"""
        return EarthMoverDistanceFunction.apply(input1, input2)


# ---- the Chamfer extension as an autograd function (utils/metrics/distance/cd/chamfer_distance.py)
_CHAMFER_ACC = {}   # device index -> the scatter words of dg_chamfer_backward (int64, zero at rest, grown on demand)


def _chamfer_acc(device, words):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    t = _CHAMFER_ACC.get(idx)
    if t is None or t.numel() < words:
        t = _CHAMFER_ACC[idx] = torch.zeros(words, dtype=torch.int64, device=device)
    return t


def _chamfer_nn(a, b):
    """(dist [B,n], idx [B,n] int32) of every point of a[i] in b[i]: dg_chamfer_nn on packed clouds"""
    B, n, m = a.size(0), a.size(1), b.size(1)
    dist = torch.empty(B, n, dtype=torch.float32, device=a.device)
    idx = torch.empty(B, n, dtype=torch.int32, device=a.device)
    L.check(L.lib().dg_chamfer_nn(L.ptr(a), 3 * n, 3, 1, n, L.ptr(b), 3 * m, 3, 1, m, B, L.ptr(dist), L.ptr(idx),
                                  L.stream_ptr()), "dg_chamfer_nn")
    return dist, idx


def chamfer_backward(xyz1, xyz2, g1, g2, idx1, idx2):
    """(grad1 [B,n,3], grad2 [B,m,3]) of the Chamfer extension (chamfer_distance.cpp:82-140) from the gradients g1 [B,n],
    g2 [B,m] of its two distance vectors and the neighbour indices of its forward: explicit, no autograd
    (dg_chamfer_backward; bit-identical run to run).  The scatter words are one buffer per device, shared by every call on it:
    calls on different streams of one device must not overlap."""
    _pair(xyz1, xyz2)
    B, n, m = xyz1.size(0), xyz1.size(1), xyz2.size(1)
    for t, k, what in ((g1, n, "g1"), (idx1, n, "idx1"), (g2, m, "g2"), (idx2, m, "idx2")):
        assert tuple(t.shape) == (B, k), "expected {} ({},{}), but got {}".format(what, B, k, tuple(t.shape))
    a, b = _prep(xyz1.detach()), _prep(xyz2.detach())
    if not (g1.is_cuda and g2.is_cuda and idx1.is_cuda and idx2.is_cuda):
        raise RuntimeError("chamfer distance runs on the GPU only (no CPU fallback)")
    g1, g2 = g1.detach().contiguous().float(), g2.detach().contiguous().float()
    idx1, idx2 = idx1.contiguous().int(), idx2.contiguous().int()
    grad1, grad2 = torch.empty_like(a), torch.empty_like(b)
    acc = _chamfer_acc(a.device, B * (n + m) * 4)
    L.check(L.lib().dg_chamfer_backward(L.ptr(a), n, L.ptr(b), m, B, L.ptr(g1), L.ptr(g2), L.ptr(idx1), L.ptr(idx2),
                                        L.ptr(grad1), L.ptr(grad2), L.ptr(acc), L.stream_ptr()), "dg_chamfer_backward")
    return grad1, grad2


class ChamferDistanceFunction(torch.autograd.Function):
    """utils/metrics/distance/cd/chamfer_distance.py:16-61: (dist1 [B,n], dist2 [B,m]), the squared distance of every point
    to its nearest neighbour in the paired cloud, both ways (two dg_chamfer_nn searches); backward is dg_chamfer_backward"""

    @staticmethod
    def forward(ctx, xyz1, xyz2):
        _pair(xyz1, xyz2)
        a, b = _prep(xyz1), _prep(xyz2)
        dist1, idx1 = _chamfer_nn(a, b)
        dist2, idx2 = _chamfer_nn(b, a)
        ctx.save_for_backward(a, b, idx1, idx2)
        return dist1, dist2

    @staticmethod
    def backward(ctx, graddist1, graddist2):
        a, b, idx1, idx2 = ctx.saved_tensors
        return chamfer_backward(a, b, graddist1, graddist2, idx1, idx2)


class ChamferDistance(torch.nn.Module):
    def forward(self, xyz1, xyz2):
        return ChamferDistanceFunction.apply(xyz1, xyz2)


chamfer_distance = ChamferDistanceFunction.apply


def emd_distance_matrix(pcs_1, pcs_2):
    """M[i,j] = compute_emd(pcs_1[i], pcs_2[j]) = cost / N (cov_mmd_1nna.py:12-17), all pairs in one launch"""
    a, b = _prep(pcs_1), _prep(pcs_2)
    assert a.size(1) == b.size(1)
    out = torch.empty(a.size(0), b.size(0), dtype=torch.float32, device=a.device)
    L.check(L.lib().dg_emd(L.ptr(a), a.size(0), a.size(1), L.ptr(b), b.size(0), b.size(1), 0, L.ptr(out),
                           L.stream_ptr()), "dg_emd")
    return out / float(a.size(1))
