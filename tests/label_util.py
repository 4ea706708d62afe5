"""Plain numpy restatements for the label-image and object-removal tests, and the reader of
tests/golden/label_image.npz.  Nothing here touches the code under test.

The label projection restates the reference's far-to-near scatter (process_kitti.py:60-73, :85-86, :124-126) with the
engine's documented tie rule made explicit: of two points of one cell with the same float32 range the LOWER index wins
(the reference's unstable argsort leaves that open; the golden inputs contain no such tie).
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "label_image.npz")
SCANS = ("prefix_w256", "rings50_w512", "rings67_w256")   # of tests/golden/raw_scan.npz
H = 64


def load():
    return np.load(GOLDEN)


def depth32(points):
    """np.linalg.norm(xyz, ord=2, axis=1) in float32, as process_kitti.py:85"""
    return np.linalg.norm(np.asarray(points, dtype=np.float32)[:, :3], ord=2, axis=1)


def scatter_far_to_near(row, col, depth, values, H, W, fill=0):
    """[H,W] image of `values`: points written far to near, later writes win, the lower index last among equal ranges.
    row / col: integer arrays [N] (row already wrapped into [0, H)); points with row < 0 or col < 0 take no part"""
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    depth = np.asarray(depth, dtype=np.float32)
    values = np.asarray(values)
    img = np.full((H, W), fill, dtype=values.dtype)
    idx = np.arange(len(row))
    order = np.lexsort((-idx, -depth.astype(np.float64)))    # range descending, then index descending
    order = order[(row[order] >= 0) & (col[order] >= 0)]
    for i in order:                                          # (a loop: the order of duplicate writes is the point)
        img[row[i], col[i]] = values[i]
    return img


def winner_image(row, col, depth, H, W):
    """[H,W] int64: the index of every cell's winner, -1 for an empty cell"""
    return scatter_far_to_near(row, col, depth, np.arange(len(row), dtype=np.int64), H, W, fill=-1)


def label_images(row, col, depth, labels, lut, H, W):
    """(sem [H,W] uint8, inst [H,W] uint16) of raw uint32 label words"""
    labels = np.asarray(labels).view(np.uint32) if np.asarray(labels).dtype != np.uint32 else np.asarray(labels)
    win = winner_image(row, col, depth, H, W)
    sem = np.zeros((H, W), dtype=np.uint8)
    inst = np.zeros((H, W), dtype=np.uint16)
    on = win >= 0
    sem[on] = np.asarray(lut, dtype=np.uint8)[labels[win[on]] & 0xFFFF]
    inst[on] = (labels[win[on]] >> 16).astype(np.uint16)
    return sem, inst


def kitti_grid(points, W):
    """(row, col) of a raw KITTI scan as process_kitti.py:88-113 forms them, rows wrapped like numpy's negative index.
    float32 throughout; meant for scans whose points keep clear of the column edges (a 1-ulp difference in atan2 moves a
    point on an edge one column over)"""
    x, y = points[:, 0], points[:, 1]
    quads = np.zeros(len(x), dtype=np.int64)
    quads[(x < 0) & (y >= 0)] = 1
    quads[(x < 0) & (y < 0)] = 2
    quads[(x >= 0) & (y < 0)] = 3
    start = (np.roll(quads, 1) - quads) == 3
    c = np.cumsum(start)
    L = int(start.sum())
    row = np.where(c == 0, 0, H - L + c - 1)
    assert row.min() >= -H
    yaw = -np.arctan2(y, x)
    g = (yaw / np.float32(np.pi) + np.float32(1)) / np.float32(2) % np.float32(1)
    col = np.floor(g * np.float32(W)).astype(np.int64)
    return row % H, col


def nearest_src(in_size, out_size):
    """[out_size] source indices of torch's legacy nearest: min(floor(dst * float32(in) / float32(out)), in - 1), in float32"""
    scale = np.float32(in_size) / np.float32(out_size)
    s = np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(s, in_size - 1)


def label_resize(sem, H, W):
    """[B,Hs,Ws] -> [B,H,W], nearest, no flip"""
    hs, ws = nearest_src(sem.shape[1], H), nearest_src(sem.shape[2], W)
    return sem[:, hs][:, :, ws]


def remove_mask(sem, valid, table, r):
    """(remove [B,H,W] uint8, class_pixels [B,256] uint32): remove = 1 where any pixel within |dh| <= r, |dw| <= r is valid
    and of a class with table[class] != 0; columns wrap, rows outside the image take no part"""
    sem, valid, table = np.asarray(sem, dtype=np.uint8), np.asarray(valid) != 0, np.asarray(table, dtype=np.uint8)
    B, H, W = sem.shape
    flag = valid & (table[sem] != 0)
    remove = np.zeros((B, H, W), dtype=bool)
    for dh in range(-r, r + 1):
        if abs(dh) >= H:                             # every source row lies outside the image
            continue
        for dw in range(-r, r + 1):
            src = np.roll(flag, dw, axis=2)          # src[.., w] = flag[.., w - dw]: the ring
            if dh >= 0:
                remove[:, dh:] |= src[:, :H - dh]    # remove[h] |= src[h - dh]
            else:
                remove[:, :H + dh] |= src[:, -dh:]
    counts = np.stack([np.bincount(sem[b][valid[b]], minlength=256) for b in range(B)]).astype(np.uint32)
    return remove.astype(np.uint8), counts


def compose(tgt_inv, valid, gen_inv, keep, keep_is_depth, tol, remove, sem, fill_label):
    """(inv_out, source, sem_out, counts [B,3] = removed, filled, in_front); inv_out carries the selected input's bits"""
    tgt_inv, gen_inv = np.asarray(tgt_inv, dtype=np.float32), np.asarray(gen_inv, dtype=np.float32)
    v, rm = np.asarray(valid) != 0, np.asarray(remove) != 0
    keep = np.asarray(keep, dtype=np.float32)
    kp = keep > np.float32(tol) if keep_is_depth else keep != 0
    measured, filled = ~rm & v, rm & kp
    inv_out = np.where(measured, tgt_inv.view(np.uint32), np.where(filled, gen_inv.view(np.uint32), np.uint32(0))).view(np.float32)
    source = np.where(measured, 1, np.where(filled, 2, 0)).astype(np.uint8)
    sem_out = np.where(measured, sem, np.where(filled, fill_label, 0)).astype(np.uint8)
    front = filled & v & (gen_inv > tgt_inv)
    B = tgt_inv.shape[0]
    counts = np.stack([(rm & v).reshape(B, -1).sum(1), filled.reshape(B, -1).sum(1), front.reshape(B, -1).sum(1)], 1)
    return inv_out, source, sem_out, counts.astype(np.int32)


def cloud_remove(records, counts, idx, remove, labels):
    """per cloud b: (kept records [n,4] as uint32 words (column 3 = 0 for stride 3), labels [n], input indices [n]) of the
    records n < counts[b] with idx < 0, idx >= H W or remove[b, idx] == 0, in input order"""
    records = np.asarray(records, dtype=np.float32)
    B, N, stride = records.shape
    rm = np.asarray(remove).reshape(B, -1)
    out = []
    for b in range(B):
        n = np.arange(min(max(int(counts[b]), 0), N))
        i = np.asarray(idx[b], dtype=np.int64)[n]
        inside = (i >= 0) & (i < rm.shape[1])
        keep = ~inside | (rm[b][np.where(inside, i, 0)] == 0)
        n = n[keep]
        words = np.zeros((len(n), 4), dtype=np.uint32)
        words[:, :stride] = records[b, n].view(np.uint32)
        out.append((words, np.asarray(labels[b])[n], n.astype(np.int32)))
    return out
