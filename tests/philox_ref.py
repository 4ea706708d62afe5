"""The random inputs of a training step restated on the host (numpy, no GPU): Philox4x32-10 from its definition (Salmon,
Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11, and the Random123 distribution's philox.h) and the
draw transforms from the comments that define them in csrc/step_inputs.hip - what tests/test_gpu_draws.py holds every
draw entry point to, element by element.  tests/test_philox_ref_cpu.py pins this file without a GPU.

Counter layout of every draw: the 128-bit counter is (offset + i, stream id) as two 64-bit halves, low word first, the key
is the 64-bit seed; `offset + i` wraps at 2^64.  Uniforms and integers are exact (the fp32 operations that form them are);
everything transcendental is evaluated in float64 from the exact fp32 uniforms."""
import math

import numpy as np

from oracle import dusty_oracle as O

M0, M1 = 0xD2511F53, 0xCD9E8D57      # the two round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85      # the key schedule's increments (golden ratio, sqrt(3) - 1)
ROUNDS = 10
MASK32, MASK64 = 0xFFFFFFFF, 2**64 - 1
S24 = np.float32(2.0 ** -24)
EPS = 1e-10                          # GumbelSigmoid.eps


def philox_scalar(counter, key):
    """one block in python integers: counter 4 x 32 bit, key 2 x 32 bit -> 4 words.  A round multiplies words 0 and 2 by the
    two constants to 64 bits; the new words are (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key is bumped between rounds."""
    c, k = list(counter), list(key)
    for r in range(ROUNDS):
        if r:
            k = [(k[0] + W0) & MASK32, (k[1] + W1) & MASK32]
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK32, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK32]
    return c


def words_scalar(seed, stream, offset, n4):
    """[n4,4] words of counters offset .. offset + n4 - 1 (mod 2^64), one python-integer block at a time"""
    out = np.empty((n4, 4), dtype=np.uint32)
    for i in range(n4):
        lo = (offset + i) & MASK64
        out[i] = philox_scalar([lo & MASK32, lo >> 32, stream & MASK32, (stream >> 32) & MASK32],
                               [seed & MASK32, (seed >> 32) & MASK32])
    return out


def counters(offset, n4):
    """offset + i for i < n4 as uint64, wrapping at 2^64"""
    return np.arange(n4, dtype=np.uint64) + np.array([int(offset) & MASK64], dtype=np.uint64)


def philox4x32_10(seed, ctr_lo, ctr_hi):
    """vectorised over 64-bit counter halves (arrays or integers, broadcast) -> uint32 [n,4].  Every word is held in a uint64
    lane below 2^32, so a 32 x 32 product fits its lane exactly."""
    lo, hi = np.broadcast_arrays(np.atleast_1d(np.asarray(ctr_lo, dtype=np.uint64)), np.atleast_1d(np.asarray(ctr_hi, dtype=np.uint64)))
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    c0, c1, c2, c3 = lo & m32, lo >> s32, hi & m32, hi >> s32
    seed = int(seed) & MASK64
    k0, k1 = seed & MASK32, seed >> 32
    for r in range(ROUNDS):
        if r:
            k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def words(seed, stream, offset, n4):
    """[n4,4]: row i = the block of counter (offset + i, stream), key seed - dg_philox_bits"""
    return philox4x32_10(seed, counters(offset, n4), int(stream) & MASK64)


def groups(n):
    return (n + 3) // 4


# ---- the counters a draw consumes, as half-open intervals [first, last) ------------------------------------------------------
def fill_range(offset, n):
    return offset, offset + groups(n)


def logistic_range(offset, n):
    return offset, offset + 2 * groups(n)


def aug_range(offset, B):
    return offset, offset + 2 * B


# ---- the transforms ----------------------------------------------------------------------------------------------------------
def u24(w):
    """kind 0: (r >> 8) * 2^-24 in [0,1) - an integer below 2^24 times a power of two: exact in fp32"""
    return (w >> np.uint32(8)).astype(np.float32) * S24


def elements(w, n):
    """element o of a fill = word o % 4 of group o / 4"""
    return w.reshape(-1)[:n]


def uniform(seed, stream, offset, n):
    return elements(u24(words(seed, stream, offset, groups(n))), n)


def uniform_range(seed, stream, offset, n, lo, hi):
    """kind 2: lo + (hi - lo) u -> (twice rounded, once rounded): the product rounded to fp32 before the sum, or the fused
    multiply-add's single rounding.  hi - lo is an fp32 subtraction in both."""
    u = uniform(seed, stream, offset, n)
    lo, d = np.float32(lo), np.float32(hi) - np.float32(lo)
    twice = lo + d * u
    p = np.float64(d) * u.astype(np.float64)             # 24 x 24 bits: exact
    s = np.float64(lo) + p
    t = s - np.float64(lo)
    if np.any((np.float64(lo) - (s - t)) + (p - t) != 0):  # (two-sum's error term: the float64 sum is the real one)
        raise ValueError("lo + (hi - lo) u is not exact in float64 for this range")
    return twice, s.astype(np.float32)


def integers(seed, stream, offset, n, ilo, ihi):
    """kind 3: ilo + r % (ihi - ilo) as int32"""
    r = elements(words(seed, stream, offset, groups(n)), n).astype(np.int64)
    return (ilo + r % (ihi - ilo)).astype(np.int32)


def normal_of(w, n):
    """kind 1 on blocks w [n4,4]: Box-Muller on the word pairs (0,1) and (2,3) with u1 = 1 - uniform in (0,1] (exact in fp32:
    (2^24 - k) 2^-24) and u2 = uniform; the even element of a pair is rad cos(theta), the odd one rad sin(theta)
    -> (values, rad) in float64"""
    u = u24(w)
    u1 = (np.float32(1.0) - u[:, 0::2]).astype(np.float64)
    theta = 2.0 * math.pi * u[:, 1::2].astype(np.float64)
    rad = np.sqrt(-2.0 * np.log(u1))
    v = np.stack([rad * np.cos(theta), rad * np.sin(theta)], axis=2)      # [n4, pair, (cos, sin)]
    return v.reshape(-1)[:n], np.repeat(rad, 2, axis=1).reshape(-1)[:n]


def normal(seed, stream, offset, n):
    return normal_of(words(seed, stream, offset, groups(n)), n)


def logistic_of(u1, u2, eps=EPS):
    """GumbelSigmoid.logistic_noise on two fp32 uniform fields: -ln(ln(u1 + eps) / ln(u2 + eps) + eps); the two inner sums are
    correctly rounded fp32 additions, the rest float64"""
    e = np.float32(eps)
    a = (np.asarray(u1, dtype=np.float32) + e).astype(np.float64)
    b = (np.asarray(u2, dtype=np.float32) + e).astype(np.float64)
    return -np.log(np.log(a) / np.log(b) + np.float64(e))


def logistic(seed, stream, offset, n, eps=EPS):
    """U1 = the uniform fill at `offset`, U2 the one ceil(n / 4) counters further"""
    return logistic_of(uniform(seed, stream, offset, n), uniform(seed, stream, offset + groups(n), n), eps)


def aug_geometry(H, W):
    """(sh, sw, nx, ny): the translation half-ranges and the cutout offset ranges of the reference's utils/diff_augment.py -
    randint(-shift, shift + 1) per axis (:58-60), randint(0, size + (1 - cut % 2)) per axis (:85-87)"""
    sh, sw = O.translation_shift(H, W)
    ch, cw = O.cutout_size(H, W)
    return sh, sw, H + (1 - ch % 2), W + (1 - cw % 2)


def augment(seed, stream, offset, B, H, W):
    """one parameter set per sample from counters offset + 2 b and offset + 2 b + 1 -> (uf float32 [3,B], qi int32 [4,B]):
    uf = -1 + 2 u of words 0-2 of the first (exact in fp32: (k - 2^23) 2^-23), qi = (t_h, t_w, o_x, o_y) from the four words of
    the second with ranges 2 sh + 1, 2 sw + 1, nx, ny"""
    w = words(seed, stream, offset, 2 * B)
    sh, sw, nx, ny = aug_geometry(H, W)
    uf = (np.float32(-1.0) + np.float32(2.0) * u24(w[0::2, :3])).T
    r = w[1::2].astype(np.int64)
    qi = np.stack([-sh + r[:, 0] % (2 * sh + 1), -sw + r[:, 1] % (2 * sw + 1), r[:, 2] % nx, r[:, 3] % ny]).astype(np.int32)
    return np.ascontiguousarray(uf), qi


# ---- the bounds of tests/test_gpu_draws.py -------------------------------------------------------------------------------------
# normals: fp32(2 pi u2) is off by at most 2.4e-7 (half an ulp below 2 pi) plus the constant's own rounding, sinf / cosf by at
# most 2 ulp, rad = sqrtf(-2 logf(u1)) by at most 3 ulp relative: below 9e-7 rad together; 2^-20 = 9.54e-7
NORMAL_TOL = 2.0 ** -20
# logistic noise: ~3 ulp relative on the quotient, half an ulp on q + eps, 1 ulp on the outer log, whose ABSOLUTE error is its
# argument's relative error
LOGISTIC_TOL = 2.0 ** -20


def normal_bound(rad):
    return NORMAL_TOL * np.maximum(rad, 1.0)


def logistic_bound(want):
    return LOGISTIC_TOL * np.maximum(1.0, np.abs(want))
