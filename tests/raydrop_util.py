"""The three ray-drop kernels (csrc/raydrop.hip) restated in plain NumPy, written for the tests: the reference holds no code
for the transfer.  tests/test_raydrop_cpu.py pins these functions on hand-made cases without a GPU; the GPU tests hold the
kernels to them exactly.

Exactness of the winner's range: the kernel forms d_u = sqrt((x x + y y) + z z) in double, where the compiler may fuse a
product into the following sum; NumPy rounds every operation.  On coordinates that are multiples of 2^-12 below 2 in magnitude
(`quantise`) every product and sum is exact in double either way, and sqrt is correctly rounded on both sides, so the two
agree bit for bit before and after the rounding to float32.  The GPU tests draw their clouds on that lattice."""
import numpy as np

LATTICE = 4096.0   # coordinates are multiples of 1 / LATTICE


def quantise(xyz):
    return (np.round(np.asarray(xyz, dtype=np.float64) * LATTICE) / LATTICE).astype(np.float32)


def ranges(records):
    """[..., >= 3] float32 records -> float32 |xyz|: double arithmetic on the float32 coordinates, rounded once"""
    x = records[..., 0].astype(np.float64)
    y = records[..., 1].astype(np.float64)
    z = records[..., 2].astype(np.float64)
    return np.sqrt((x * x + y * y) + z * z).astype(np.float32)


def winner(records, idx, counts, HW):
    """records [B,N,3|4], idx [B,N] (the pixel of every point, -1: took no part), counts [B] or None -> win [B,HW] int32: per
    pixel the lexicographic minimum of (float32 range, point index) over the points binned into it, -1 for none"""
    B, N = idx.shape
    win = np.full((B, HW), -1, dtype=np.int32)
    for b in range(B):
        n = N if counts is None else int(min(max(counts[b], 0), N))
        ids = np.asarray(idx[b, :n])
        p = np.nonzero((ids >= 0) & (ids < HW))[0]
        r = ranges(records[b, :n])[p]
        o = p[np.lexsort((p, r))][::-1]          # descending (range, index): of repeated indices the LAST assignment stays
        win[b, ids[o]] = o
    return win


def keep(conf, win, noise):
    """conf [B,C,H,W] raw logits (C = 1: pixel; C = 2: pixel, image), win [B,HW], noise [B,K,1,H,W] -> keep [B,K,H,W] uint8 =
    win >= 0 and h1 + noise > 0 (one float32 addition) and, for C = 2, h2 > 0"""
    B, C, H, W = conf.shape
    l1 = conf[:, None, 0].astype(np.float32) + noise[:, :, 0].astype(np.float32)      # [B,K,H,W]
    k = (l1 > 0) & (win.reshape(B, 1, H, W) >= 0)
    if C == 2:
        k &= conf[:, None, 1] > 0
    return k.astype(np.uint8)


def gather(records, win, keep, labels=None):
    """-> {(b, k): (records [n,4] float32 - the input records' bits, column 3 zero for stride 3 -, labels [n] uint32 or None,
    index [n] int32)} over the kept pixels in row-major order"""
    B, K = keep.shape[:2]
    out = {}
    for b in range(B):
        for k in range(K):
            p = np.nonzero(keep[b, k].reshape(-1))[0]
            w = win[b, p]
            w = w[w >= 0]
            rec = np.zeros((len(w), 4), dtype=np.float32)
            rec[:, :records.shape[2]] = records[b, w]
            out[b, k] = (rec, None if labels is None else labels[b, w].astype(np.uint32), w.astype(np.int32))
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)
