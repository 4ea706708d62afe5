"""Yardsticks of the point-set distance gradients (tests/test_emd_grad_cpu.py, tests/test_gpu_point_distance_grad.py,
tests/golden/make_emd_grad_golden.py).

EMD.  The reference differentiates matchcost only (utils/metrics/distance/emd/earth_mover_distance.cu:305-388, behind
EarthMoverDistanceFunction.backward): `match` is a constant,
    grad1[k] = grad_cost * sum_l 2 match[l][k] (x1_k - x2_l)        grad2[l] = grad_cost * sum_k 2 match[l][k] (x2_l - x1_k).
oracle.metrics_oracle.emd_costs restates approxmatch + matchcost but returns only the cost, so `approxmatch` below walks the
same loop, in the order that function documents (float32: the kernels' order of sums, their fused multiply-adds, their
__expf; float64: the same algorithm as the yardstick), and KEEPS the match matrix.  The gradient formula is then applied in
float64 to either matrix: what separates the two results is the float32 rounding of `match` alone, which is the
reference's own distance from the float64 algorithm (`e_ref`).

Chamfer.  `chamfer_backward_f64` is chamfer_distance.cpp:82-140 in float64 from GIVEN indices, and per entry the sum of
|terms| and the number of terms it received (what the GPU test's error bound is made of)."""
import numpy as np

EMD_GRAD_CASES = ["p1_1", "p2_3", "p4_4", "p64_64", "p96_32", "p50_150", "p100_30", "p520_1030", "p1030_520", "b35_8_8",
                  "far_96_32", "self_64"]


def approxmatch(x1, x2, dtype=np.float64):
    """x1 [P,n,3], x2 [P,m,3] -> (match [P,n,m] (match[p][k][l] = the reference's match[l][k]), d2 [P,n,m]) in `dtype`"""
    f = np.dtype(dtype).type
    x1, x2 = np.asarray(x1, np.float32).astype(f), np.asarray(x2, np.float32).astype(f)
    P, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    if f is np.float32:
        def fma(a, b, c):   # float32 products are exact in float64; the sum then rounds once
            return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f)
    else:
        def fma(a, b, c):
            return a * b + c
    multiL, multiR = (1.0, float(n // m)) if n >= m else (float(m // n), 1.0)
    remainL, remainR = np.full((P, n), multiL, f), np.full((P, m), multiR, f)
    guard = np.full((1, 1), np.float32(1e-9), f)
    diff = x2[:, None, :, :] - x1[:, :, None, :]
    d2 = fma(diff[..., 1], diff[..., 1], diff[..., 0] * diff[..., 0]) + diff[..., 2] * diff[..., 2]
    match = np.zeros((P, n, m), f)
    for j in range(7, -3, -1):
        level = f(0.0) if j == -2 else f(-(4.0 ** j))
        with np.errstate(under="ignore"):
            if f is np.float32:
                E = np.exp2(((level * d2) * np.float32(1.4426950408889634)).astype(np.float64)).astype(f)
            else:
                E = np.exp(level * d2)
        suml = np.broadcast_to(guard, (P, n))
        for l in range(m):
            suml = fma(E[:, :, l], remainR[:, l:l + 1], suml)
        ratioL = remainL / suml
        sumr = np.zeros((P, m), f)
        for k in range(n):
            sumr = fma(E[:, k, :], ratioL[:, k:k + 1], sumr)
        consumption = np.minimum(remainR / fma(sumr, remainR, guard), f(1.0))
        ratioR = consumption * remainR
        remainR = np.maximum(f(0.0), fma(-sumr, remainR, remainR))
        Wl = E * ratioL[:, :, None]
        suml = np.zeros((P, n), f)
        for l in range(m):
            suml = fma(Wl[:, :, l], ratioR[:, l:l + 1], suml)
        match = fma(Wl, ratioR[:, None, :], match)
        remainL = np.maximum(f(0.0), remainL - suml)
    return match, d2


def matchcost(match, d2):
    """matchcost<<<32, 512>>> (:218-262) in the order of oracle.metrics_oracle.emd_costs -> [P] float64"""
    f = match.dtype.type
    P, n, m = match.shape
    if f is np.float32:
        def fma(a, b, c):
            return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f)
    else:
        def fma(a, b, c):
            return a * b + c
    sub = np.zeros((P, 512), f)
    for k0 in range(0, n, 512):
        k1 = min(n, k0 + 512)
        s = sub[:, :k1 - k0]
        for l in range(m):
            s = fma(match[:, k0:k1, l], d2[:, k0:k1, l], s)
        sub[:, :k1 - k0] = s
    while sub.shape[1] > 1:
        sub = sub[:, 0::2] + sub[:, 1::2]
    return sub[:, 0].astype(np.float64)


def match_grads(x1, x2, match, grad_cost=None):
    """matchcostgrad1 / matchcostgrad2 (:305-388) in float64 over a given match [P,n,m] -> (g1 [P,n,3], g2 [P,m,3])"""
    a, b, w = np.asarray(x1, np.float64), np.asarray(x2, np.float64), 2.0 * np.asarray(match, np.float64)
    g1 = a * w.sum(2)[..., None] - np.einsum("pkl,plc->pkc", w, b)
    g2 = b * w.sum(1)[..., None] - np.einsum("pkl,pkc->plc", w, a)
    if grad_cost is not None:
        gc = np.asarray(grad_cost, np.float64).reshape(-1, 1, 1)
        g1, g2 = g1 * gc, g2 * gc
    return g1, g2


def emd_grads(x1, x2, dtype=np.float64):
    """(cost [P], g1 [P,n,3], g2 [P,m,3]) float64: approxmatch in `dtype`, the gradient formula in float64"""
    match, d2 = approxmatch(x1, x2, dtype)
    g1, g2 = match_grads(x1, x2, match)
    return matchcost(match, d2), g1, g2


def match_grads_ref_layout(x1, x2, match_flat):
    """the same formula over the buffer the reference's approxmatch kernel fills: match[i n m + l n + k]"""
    P, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    return match_grads(x1, x2, np.asarray(match_flat).reshape(P, m, n).transpose(0, 2, 1))


def chamfer_backward_f64(x1, x2, g1, g2, idx1, idx2):
    """chamfer_distance_backward (chamfer_distance.cpp:82-140) in float64 from given indices.
    -> (grad1 [B,n,3], grad2 [B,m,3], abs1, abs2 (the sums of |terms| per entry), cnt1 [B,n], cnt2 [B,m] (terms per point))"""
    a, b = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    g1, g2 = np.asarray(g1, np.float64), np.asarray(g2, np.float64)
    B, n, m = a.shape[0], a.shape[1], b.shape[1]
    grad1, grad2 = np.zeros_like(a), np.zeros_like(b)
    abs1, abs2 = np.zeros_like(a), np.zeros_like(b)
    cnt1, cnt2 = np.zeros((B, n)), np.zeros((B, m))
    for i in range(B):
        j1, j2 = np.asarray(idx1[i], np.int64), np.asarray(idx2[i], np.int64)
        t = 2.0 * g1[i][:, None] * (a[i] - b[i][j1])            # point j of cloud 1 and its neighbour j1[j] in cloud 2
        grad1[i] += t
        abs1[i] += np.abs(t)
        cnt1[i] += 1
        np.add.at(grad2[i], j1, -t)
        np.add.at(abs2[i], j1, np.abs(t))
        np.add.at(cnt2[i], j1, 1)
        t = 2.0 * g2[i][:, None] * (b[i] - a[i][j2])
        grad2[i] += t
        abs2[i] += np.abs(t)
        cnt2[i] += 1
        np.add.at(grad1[i], j2, -t)
        np.add.at(abs1[i], j2, np.abs(t))
        np.add.at(cnt1[i], j2, 1)
    return grad1, grad2, abs1, abs2, cnt1, cnt2


def chamfer_bound(abs_terms, cnt):
    """per entry 2^-21 sum |terms| + 2^-39 count: a term is three float32 roundings (<= 3 * 2^-24 relative), the fixed-point
    sum adds 2^-40 per term, the result is rounded to float32 once (2^-24 of |sum| <= sum |terms|); the total 4 * 2^-24
    sum |terms| + 2^-40 count, doubled"""
    return 2.0 ** -21 * abs_terms + 2.0 ** -39 * cnt[..., None]
