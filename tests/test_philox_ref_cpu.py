"""tests/philox_ref.py on the CPU: the generator against the Random123 known answers, vectorised against scalar across the
2^32 carry and the 2^64 wrap, the edge offsets tests/test_gpu_draws.py relies on - and the written proof of the gap: every
defect a shared draw body can have passes what the suite checked before (the mean / standard-deviation bounds of
tests/test_gpu_ops.py::test_philox_known_answer, the value ranges of test_diffaug's draw, the self-comparison of
test_logistic_noise_in_one_launch) and fails the per-element comparison with the host reference."""
import math

import numpy as np
import pytest

from oracle import philox as OP
from tests import philox_ref as P

SEED, STREAM = 20240229, 5
# Found once by scanning word 0 of the counters 0, 1, 2, ... of (SEED, STREAM) (about 2^24 counters each, seconds in numpy):
EDGE_ZERO = 24486405     # word 0 >> 8 == 0:        uniform 0,         normal u1 = 1 (radius 0),          logistic ln(eps)
EDGE_ONES = 11156174     # word 0 >> 8 == 0xFFFFFF: uniform 1 - 2^-24, normal u1 = 2^-24 (largest radius)

N_OLD = 1 << 20          # the element count of test_philox_known_answer's distribution check
N_NEW = 1 << 16          # the element count of the per-element comparison


# ---- the generator -------------------------------------------------------------------------------------------------------------
KAT = [
    ([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]),
]


@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_known_answers(ctr, key, want):
    """Random123's kat_vectors for philox4x32-10, scalar and vectorised"""
    assert P.philox_scalar(ctr, key) == want
    got = P.philox4x32_10(key[0] | key[1] << 32, ctr[0] | ctr[1] << 32, ctr[2] | ctr[3] << 32)
    assert got.dtype == np.uint32 and got.tolist() == [want]


@pytest.mark.parametrize("offset", [0, 977, 2**32 - 5, 2**33 + 1, 2**64 - 3])
@pytest.mark.parametrize("stream", [0, 5, 2**32 + 7, 2**64 - 1])
def test_vectorised_equals_scalar_across_the_carry_and_the_wrap(offset, stream):
    """offset + i carries into the counter's second word at 2^32 and wraps to 0 at 2^64, inside one call"""
    for seed in (0, SEED, 2**63 + 11):
        w = P.words(seed, stream, offset, 9)
        assert np.array_equal(w, P.words_scalar(seed, stream, offset, 9))
        assert np.array_equal(w.reshape(-1), OP.bits(seed, stream, offset, 9))     # (the suite's earlier restatement)
    lo = P.counters(offset, 9)
    assert [int(v) for v in lo] == [(offset + i) % 2**64 for i in range(9)]


def test_counter_ranges():
    assert P.fill_range(7, 1) == (7, 8) and P.fill_range(7, 4) == (7, 8) and P.fill_range(7, 5) == (7, 9)
    assert P.logistic_range(3, 5) == (3, 7) and P.logistic_range(0, 4096) == (0, 2048)
    assert P.aug_range(10, 16) == (10, 42)


def test_transforms_on_hand_made_words():
    w = np.array([[0, 0xFFFFFFFF, 0x80000000, 0x000000FF]], dtype=np.uint32)
    assert P.u24(w).tolist() == [[0.0, 1.0 - 2.0 ** -24, 0.5, 0.0]]
    v, rad = P.normal_of(w, 4)
    # pair (0,1): u1 = 1 -> radius 0; pair (2,3): u1 = 0.5, u2 = 0 -> (sqrt(2 ln 2), 0)
    assert v[0] == 0.0 and v[1] == 0.0 and rad[0] == 0.0
    assert abs(v[2] - math.sqrt(2 * math.log(2))) < 1e-15 and v[3] == 0.0 and rad[2] == rad[3]
    lg = P.logistic_of(np.float32([0.0, 0.5]), np.float32([0.0, 0.25]))
    e = float(np.float32(1e-10))
    assert abs(lg[0] + math.log(1.0 + e)) < 1e-24 and abs(lg[1] + math.log(0.5 + e)) < 1e-9
    assert P.aug_geometry(64, 1024) == (4, 64, 65, 1025) and P.aug_geometry(7, 9) == (0, 1, 8, 9)
    assert P.aug_geometry(10, 36) == (1, 2, 10, 37) and P.aug_geometry(2, 2) == (0, 0, 2, 2)


def test_uniform_range_gives_both_roundings():
    twice, once = P.uniform_range(SEED, STREAM, 977, 4099, -0.75, 2.5)
    u = P.uniform(SEED, STREAM, 977, 4099).astype(np.float64)
    assert twice.dtype == once.dtype == np.float32
    assert np.abs(once.astype(np.float64) - (-0.75 + 3.25 * u)).max() <= 2.0 ** -23      # half an ulp below 4
    assert np.abs(twice.astype(np.float64) - (-0.75 + 3.25 * u)).max() <= 2.0 ** -22
    assert 0 < np.count_nonzero(twice != once) < 4099
    assert twice.min() >= -0.75 and twice.max() <= 2.5


# ---- the edge offsets ------------------------------------------------------------------------------------------------------------
def test_edge_offsets():
    """the constants the GPU tests rely on: word 0 of those two counters, and what each draw makes of it"""
    assert int(P.words(SEED, STREAM, EDGE_ZERO, 1)[0, 0]) >> 8 == 0
    assert int(P.words(SEED, STREAM, EDGE_ONES, 1)[0, 0]) >> 8 == 0xFFFFFF
    assert P.uniform(SEED, STREAM, EDGE_ZERO, 1)[0] == 0.0
    assert P.uniform(SEED, STREAM, EDGE_ONES, 1)[0] == np.float32(1.0 - 2.0 ** -24)
    v, rad = P.normal(SEED, STREAM, EDGE_ZERO, 2)
    assert rad[0] == 0.0 and v[0] == 0.0 and v[1] == 0.0
    v, rad = P.normal(SEED, STREAM, EDGE_ONES, 2)
    assert rad[0] == math.sqrt(2 * 24 * math.log(2)) and np.isfinite(v).all()          # 5.768: the largest radius there is
    lg = P.logistic(SEED, STREAM, EDGE_ZERO, 1)
    assert np.isfinite(lg).all()
    e = np.float32(1e-10)
    b = float(P.uniform(SEED, STREAM, EDGE_ZERO + 1, 1)[0] + e)                           # (an fp32 sum)
    assert abs(lg[0] + math.log(math.log(float(e)) / math.log(b) + float(e))) < 1e-12     # ln(u1 + eps) = ln(eps)


# ---- the criteria: what the suite checked before, and this comparison ---------------------------------------------------------------
def old_uniform_ok(u):
    """test_philox_known_answer on a uniform fill"""
    return 0.0 <= float(u.min()) and float(u.max()) < 1.0 and abs(float(u.mean()) - 0.5) < 2e-3


def old_normal_ok(z):
    """test_philox_known_answer on a normal fill"""
    return abs(float(z.mean())) < 5e-3 and abs(float(z.std(ddof=1)) - 1.0) < 5e-3


def old_aug_ok(uf, qi, H, W):
    """test_diffaug's check of the drawn parameters: in range"""
    sh, sw = P.O.translation_shift(H, W)
    return bool(np.abs(uf).max() <= 1 and np.abs(qi[0]).max() <= sh and np.abs(qi[1]).max() <= sw
                and qi[2].min() >= 0 and qi[2].max() <= H and qi[3].max() <= W)


def new_normal_ok(got, want, rad):
    return bool(np.all(np.abs(got - want) <= P.normal_bound(rad)))


def new_logistic_ok(got, want):
    return bool(np.isfinite(got).all() and np.all(np.abs(got - want) <= P.logistic_bound(want)))


def device_like(x):
    """a correct device result: the float64 reference rounded to fp32"""
    return x.astype(np.float32).astype(np.float64)


def mutant_words(seed, stream, offset, n4, trunc32=False, drop_stream_hi=False):
    lo = P.counters(offset, n4)
    if trunc32:
        lo = lo & np.uint64(P.MASK32)                   # `offset + i` formed in 32 bits
    if drop_stream_hi:
        stream &= P.MASK32                              # the stream id's high word never reaches the counter
    return P.philox4x32_10(seed, lo, stream)


def mutant_normal(w, n, swap=False, one_angle=False):
    u = P.u24(w)
    u1 = (np.float32(1.0) - u[:, 0::2]).astype(np.float64)
    u2 = u[:, 1::2].astype(np.float64)
    if one_angle:
        u2 = np.repeat(u2[:, :1], 2, axis=1)            # the second pair turned by the first pair's angle
    theta, rad = 2.0 * math.pi * u2, np.sqrt(-2.0 * np.log(u1))
    c, s = rad * np.cos(theta), rad * np.sin(theta)
    return np.stack([s, c] if swap else [c, s], axis=2).reshape(-1)[:n]


def test_the_criteria_accept_a_correct_device():
    want, rad = P.normal(SEED, STREAM, 977, N_NEW)
    assert new_normal_ok(device_like(want), want, rad)
    lg = P.logistic(SEED, STREAM, 977, N_NEW)
    assert new_logistic_ok(device_like(lg), lg)
    assert old_uniform_ok(P.uniform(123, 0, 0, N_OLD)) and old_normal_ok(P.normal(123, 1, 0, N_OLD)[0])


WORD_MUTANTS = {
    # name: (offset, stream, keyword of mutant_words)
    "counter truncated to 32 bits": (2**32 + 977, STREAM, dict(trunc32=True)),
    "stream id's high word ignored": (977, 2**32 + 7, dict(drop_stream_hi=True)),
}


@pytest.mark.parametrize("name", list(WORD_MUTANTS) + ["words permuted"])
def test_mutants_of_the_words(name):
    """wrong blocks, or the right blocks on the wrong elements: every distribution bound holds, the bits do not"""
    if name == "words permuted":
        offset, stream = 977, STREAM
        mut = lambda n4: P.words(SEED, stream, offset, n4)[:, [1, 0, 3, 2]]
    else:
        offset, stream, kw = WORD_MUTANTS[name]
        mut = lambda n4: mutant_words(SEED, stream, offset, n4, **kw)
    w = mut(N_OLD // 4)
    assert old_uniform_ok(P.u24(w).reshape(-1)) and old_normal_ok(P.normal_of(w, N_OLD)[0])
    n4 = N_NEW // 4
    good = P.words(SEED, stream, offset, n4)
    assert not np.array_equal(w[:n4], good)
    assert not np.array_equal(P.u24(w[:n4]), P.u24(good))
    want, rad = P.normal_of(good, N_NEW)
    assert not new_normal_ok(device_like(P.normal_of(w[:n4], N_NEW)[0]), want, rad)
    # the streams that test_philox_known_answer reads - offset 0, stream ids 0 and 1 - are the same with and without the defect
    if name != "words permuted":
        assert np.array_equal(mutant_words(123, 1, 0, 64, **WORD_MUTANTS[name][2]), P.words(123, 1, 0, 64))


@pytest.mark.parametrize("kw", [dict(swap=True), dict(one_angle=True)], ids=["sin and cos swapped", "both pairs from one angle"])
def test_mutants_of_box_muller(kw):
    w = P.words(123, 1, 0, N_OLD // 4)
    assert old_normal_ok(mutant_normal(w, N_OLD, **kw))
    want, rad = P.normal_of(w[:N_NEW // 4], N_NEW)
    got = device_like(mutant_normal(w[:N_NEW // 4], N_NEW, **kw))
    assert np.isfinite(got).all() and not new_normal_ok(got, want, rad)
    assert new_normal_ok(device_like(mutant_normal(w[:N_NEW // 4], N_NEW)), want, rad)      # (the unmutated restatement passes)


def test_mutant_u2_one_counter_early():
    """U2 read from ceil(n / 4) - 1: its first group is U1's last.  The earlier check - the launch against two fills of the
    same entry point and the oracle's formula on THOSE fields - sees nothing: the fields move with the defect."""
    n = N_NEW
    u1 = P.uniform(SEED, STREAM, 977, n)
    u2_bad = P.uniform(SEED, STREAM, 977 + P.groups(n) - 1, n)
    assert old_uniform_ok(P.uniform(SEED, STREAM, 977 + P.groups(N_OLD) - 1, N_OLD))
    got = device_like(P.logistic_of(u1, u2_bad))
    assert np.isfinite(got).all()
    assert np.abs(got - P.logistic_of(u1, u2_bad)).max() <= 1e-5 * np.abs(got).max()       # the old comparison: with itself
    assert not new_logistic_ok(got, P.logistic(SEED, STREAM, 977, n))
    # a short draw, where U2 then IS U1 (n <= 4: one group each): the noise would be -ln(1 + eps) everywhere
    assert np.array_equal(P.uniform(SEED, STREAM, 977 + P.groups(3) - 1, 3), P.uniform(SEED, STREAM, 977, 3))


def test_mutant_translation_range_short_by_one():
    """randint(-sh, sh + 1) has 2 sh + 1 values; with 2 sh the shift + sh is never drawn and every other one moves"""
    B, H, W = N_NEW, 64, 1024
    uf, qi = P.augment(SEED, STREAM, 977, B, H, W)
    sh, sw, nx, ny = P.aug_geometry(H, W)
    r = P.words(SEED, STREAM, 977, 2 * B)[1::2].astype(np.int64)
    bad = qi.copy()
    bad[0] = -sh + r[:, 0] % (2 * sh)
    assert old_aug_ok(uf, qi, H, W) and old_aug_ok(uf, bad, H, W)
    assert not np.array_equal(bad, qi) and bad[0].max() == sh - 1 and qi[0].max() == sh


def test_augment_draws_reach_both_ends_of_every_range():
    """B = 4096 at 7 x 9 (tests/test_gpu_draws.py, same seed and offset): each integer field attains both ends of its range -
    the largest has 9 values, so an end is missed with probability 2 (8/9)^4096 < 1e-180 - and nothing outside it; the
    uniform(-1, 1) draws stay in [-1, 1)"""
    B, H, W = 4096, 7, 9
    uf, qi = P.augment(SEED, STREAM, 977, B, H, W)
    sh, sw, nx, ny = P.aug_geometry(H, W)
    assert uf.shape == (3, B) and qi.shape == (4, B) and uf.dtype == np.float32 and qi.dtype == np.int32
    for row, (lo, hi) in zip(qi, ((-sh, sh), (-sw, sw), (0, nx - 1), (0, ny - 1))):
        assert row.min() == lo and row.max() == hi
    assert uf.min() >= -1.0 and uf.max() < 1.0
    # the sample's two counters: the parameters of sample b alone are those of the batch
    u1, q1 = P.augment(SEED, STREAM, 977 + 2 * 5, 1, H, W)
    assert np.array_equal(u1[:, 0], uf[:, 5]) and np.array_equal(q1[:, 0], qi[:, 5])
