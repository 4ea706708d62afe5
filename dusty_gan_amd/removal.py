"""Label-driven object removal: the restoration experiment with a mask that comes from the scene.

The pixels of the classes to remove (and `dilate` pixels around them) are taken out of the inversion's target, G explains the
static scene alone, and where an object stood the result takes G's generated background - if G measures the ray at all.
Removal is per PIXEL, as the ray-drop transfer's drops are (raydrop.py): every point binned into a removed pixel leaves the
cloud, whatever its own label, because the range image holds one return per ray and G's background replaces that ray.
The reference's repository holds no such command; the kernels are csrc/object_removal.hip and run on the GPU only.

    label_resize     a label image at the dataset's size -> the model's, by dg_scan_to_polar's own nearest rule
    remove_mask      classes + dilation radius -> the removal mask and the per-class pixel counts
    compose          target + generated background -> the result's inverse depth, source map, label image and counts
    cloud_remove     the records of a cloud whose pixel is not removed, in input order, bit for bit
"""
import torch

from . import _lib as L
from .raydrop import _gpu, _label_bits, _records

MAX_DILATE = 8


def class_table(classes, device):
    """class numbers -> the 256-byte table dg_remove_mask reads (1 = remove)"""
    t = torch.zeros(256, dtype=torch.uint8)
    for c in classes:
        if not 0 <= int(c) <= 255:
            raise ValueError(f"class {c}: 0..255")
        t[int(c)] = 1
    return t.to(device)


def _sem(sem, what):
    _gpu(sem, what)
    if sem.ndim != 3 or sem.dtype != torch.uint8:
        raise ValueError(f"{what}: a label image batch is uint8 [B,H,W], got {sem.dtype} {tuple(sem.shape)}")
    return sem.contiguous()


def _plane(t, shape, what):
    """[B,1,H,W] or [B,H,W] -> contiguous float32 [B,H,W]"""
    _gpu(t, what)
    if t.ndim == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: expected {tuple(shape)}, got {tuple(t.shape)}")
    return t.float().contiguous()


def label_resize(sem, H, W):
    """sem [B,Hs,Ws] uint8 -> [B,H,W] uint8: out[h, w] = sem[src(h), src(w)], src = min(floor(dst * in / out), in - 1) in
    float32 - the cell dg_scan_to_polar reads the pixel's point from (dg_label_resize)"""
    sem = _sem(sem, "label_resize")
    B, Hs, Ws = sem.shape
    out = torch.empty(B, int(H), int(W), dtype=torch.uint8, device=sem.device)
    L.check(L.lib().dg_label_resize(L.ptr(sem), B, Hs, Ws, int(H), int(W), L.ptr(out), L.stream_ptr()), "dg_label_resize")
    return out


def remove_mask(sem, valid, table, dilate=1):
    """sem [B,H,W] uint8, valid [B,(1,)H,W] (non-zero = measured), table: 256 bytes (class_table) -> (remove [B,H,W] uint8,
    class_pixels [B,256] int32): remove = 1 within `dilate` pixels (a square; columns wrap, rows do not) of a valid pixel
    whose class the table marks; class_pixels counts the valid pixels of every class (dg_remove_mask)"""
    sem = _sem(sem, "remove_mask")
    B, H, W = sem.shape
    valid = _plane(valid, sem.shape, "remove_mask")
    if not 0 <= int(dilate) <= MAX_DILATE:
        raise ValueError(f"remove_mask: dilate 0..{MAX_DILATE}, got {dilate}")
    table = _gpu(table, "remove_mask").contiguous()
    assert table.dtype == torch.uint8 and table.numel() == 256, (table.dtype, table.shape)
    remove = torch.empty_like(sem)
    class_pixels = torch.zeros(B, 256, dtype=torch.int32, device=sem.device)
    L.check(L.lib().dg_remove_mask(L.ptr(sem), L.ptr(valid), L.ptr(table), B, H, W, int(dilate), L.ptr(remove),
                                   L.ptr(class_pixels), L.stream_ptr()), "dg_remove_mask")
    return remove, class_pixels


def compose(tgt_inv, valid, gen_inv, keep, remove, sem, *, keep_is_depth=False, tol=0.0, fill_label=0):
    """the result of a removal, per pixel: the target's inverse depth where it is measured and not removed, the generated
    one where it is removed and G keeps the ray (keep != 0, or keep > tol with keep_is_depth: evaluate_batch's two rules),
    0 elsewhere.  -> (inv_out [B,1,H,W] float32 carrying the selected input's bits, source [B,H,W] uint8 (0 empty, 1 measured,
    2 generated), sem_out [B,H,W] uint8 (sem, fill_label, 0), counts [B,3] int32 = removed valid pixels, filled pixels,
    filled pixels nearer than what was measured there) (dg_compose_removed)"""
    sem = _sem(sem, "compose")
    B, H, W = sem.shape
    tgt_inv, valid = _plane(tgt_inv, sem.shape, "compose"), _plane(valid, sem.shape, "compose")
    gen_inv, keep = _plane(gen_inv, sem.shape, "compose"), _plane(keep, sem.shape, "compose")
    remove = _sem(remove, "compose")
    if remove.shape != sem.shape:
        raise ValueError(f"compose: remove must be {tuple(sem.shape)}, got {tuple(remove.shape)}")
    if not 0 <= int(fill_label) <= 255:
        raise ValueError(f"compose: fill_label 0..255, got {fill_label}")
    dev = sem.device
    inv_out = torch.empty(B, 1, H, W, dtype=torch.float32, device=dev)
    source, sem_out = torch.empty_like(sem), torch.empty_like(sem)
    counts = torch.zeros(B, 3, dtype=torch.int32, device=dev)
    L.check(L.lib().dg_compose_removed(L.ptr(tgt_inv), L.ptr(valid), L.ptr(gen_inv), L.ptr(keep), int(bool(keep_is_depth)),
                                       float(tol), L.ptr(remove), L.ptr(sem), int(fill_label), B, H, W, L.ptr(inv_out),
                                       L.ptr(source), L.ptr(sem_out), L.ptr(counts), L.stream_ptr()), "dg_compose_removed")
    return inv_out, source, sem_out, counts


def cloud_remove(records, counts, idx, remove, labels=None):
    """records [B,N,3|4] float32 (ANY buffer of the cloud's layout: the command passes the records in metres), counts [B] or
    None, idx [B,N] as LiDAR.points_to_depth returned it, remove [B,H,W] uint8, labels [B,N] optional -> (out_records
    [B,N,4], out_labels [B,N] int32 holding the uint32 bits (or None), out_index [B,N] int32, out_counts [B] int32): per cloud
    the records whose pixel is not removed (a record that took no part in the image stays), in input order, bit for bit; rows
    at and beyond the count are not written (dg_cloud_remove)"""
    x = _records(records, "cloud_remove")
    B, N, stride = x.shape
    remove = _sem(remove, "cloud_remove")
    if remove.shape[0] != B:
        raise ValueError(f"cloud_remove: remove must be [B,H,W] with B = {B}, got {tuple(remove.shape)}")
    _, H, W = remove.shape
    if tuple(idx.shape) != (B, N):
        raise ValueError(f"cloud_remove: idx must be [B,N] = {(B, N)}, got {tuple(idx.shape)}")
    idx = _gpu(idx, "cloud_remove").to(torch.int32).contiguous()
    if counts is not None:
        if tuple(counts.shape) != (B,):
            raise ValueError(f"cloud_remove: counts must be [B] = [{B}], got {tuple(counts.shape)}")
        counts = counts.to(device=x.device, dtype=torch.int32).contiguous()
    lab = None
    if labels is not None:
        if tuple(labels.shape) != (B, N):
            raise ValueError(f"cloud_remove: labels must be [B,N] = {(B, N)}, one per record, got {tuple(labels.shape)}")
        lab = _label_bits(labels.to(device=x.device)).contiguous()
    dev = x.device
    out_rec = torch.empty(B, N, 4, dtype=torch.float32, device=dev)
    out_lab = torch.empty(B, N, dtype=torch.int32, device=dev) if lab is not None else None
    out_idx = torch.empty(B, N, dtype=torch.int32, device=dev)
    out_counts = torch.empty(B, dtype=torch.int32, device=dev)
    chunks = torch.empty(B * ((N + L.EXPORT_CHUNK - 1) // L.EXPORT_CHUNK), dtype=torch.int32, device=dev)
    L.check(L.lib().dg_cloud_remove(L.ptr(x), N * stride, stride, L.ptr(counts), L.ptr(idx), L.ptr(remove), L.ptr(lab), B, N, H, W,
                                    L.ptr(chunks), L.ptr(out_rec), L.ptr(out_lab), L.ptr(out_idx), L.ptr(out_counts),
                                    L.stream_ptr()), "dg_cloud_remove")
    return out_rec, out_lab, out_idx, out_counts
