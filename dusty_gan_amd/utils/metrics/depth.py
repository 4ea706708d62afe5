"""Depth error / accuracy of reconstructions -- reference: utils/metrics/depth.py.  One launch per batch computes every
metric (csrc/inversion.hip dg_depth_metrics); `depth_metrics` also fuses revert_depth (utils/lidar.py:38-47) of the
normalised inverse depths and the drop ratios of the evaluation CSV (evaluate_reconstruction.py:121-152)."""
import torch

from ... import _lib as L

KEYS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "accuracy_1", "accuracy_2", "accuracy_3", "drop_gen", "drop_ref")


def depth_metrics(inv_ref, inv_gen, mask, min_depth, max_depth, keep=None, keep_is_depth=False, tol=0.0):
    """every per-sample metric of the reconstruction CSV -> {key: [B]} from the normalised inverse depths (min_depth /
    max_depth: the sensor's range; max_depth = 0: the maps are depths already).  keep: the generator's keep mask [B,k,H,W]
    (drop_gen = sum(1 - keep) / HW) or, with keep_is_depth, its depth image (kept where |x| > tol); default: all kept"""
    if not inv_gen.is_cuda:
        raise RuntimeError("depth metrics run on the GPU only (no CPU fallback)")
    ir, ig, m = (t.contiguous().float() for t in (inv_ref, inv_gen, mask))
    assert ir.ndim == ig.ndim == m.ndim == 4 and ir.shape == ig.shape == m.shape and ir.shape[1] == 1
    B, HW = ir.shape[0], ir.shape[2] * ir.shape[3]
    if keep is None:
        keep, keep_is_depth = torch.ones_like(ir), False
    keep = keep.contiguous().float()
    out = torch.empty(B, len(KEYS), dtype=torch.float32, device=ig.device)
    L.check(L.lib().dg_depth_metrics(L.ptr(ir), L.ptr(ig), L.ptr(m), L.ptr(keep), keep.shape[1], int(keep_is_depth),
                                     float(tol), B, HW, float(min_depth), float(max_depth), L.ptr(out), L.stream_ptr()),
            "dg_depth_metrics")
    return {k: out[:, i] for i, k in enumerate(KEYS)}


def compute_depth_error(depth_ref, depth_gen, mask=None):
    """utils/metrics/depth.py:4-25: depth maps [B,1,H,W] (metres) -> {abs_rel, sq_rel, rmse, rmse_log} per sample"""
    mask = torch.ones_like(depth_ref) if mask is None else mask
    d = depth_metrics(depth_ref, depth_gen, mask, 0.0, 0.0)
    return {k: d[k] for k in ("abs_rel", "sq_rel", "rmse", "rmse_log")}


def compute_depth_accuracy(depth_ref, depth_gen, mask=None):
    """utils/metrics/depth.py:28-43 -> {accuracy_1, accuracy_2, accuracy_3} per sample"""
    mask = torch.ones_like(depth_ref) if mask is None else mask
    d = depth_metrics(depth_ref, depth_gen, mask, 0.0, 0.0)
    return {k: d[k] for k in ("accuracy_1", "accuracy_2", "accuracy_3")}
