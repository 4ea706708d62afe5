"""The gated DiffAugment draw restated on the host (numpy, no GPU) from tests/philox_ref.py's functions: the seven numbers of
`philox_ref.augment`, then the two gates of sample b from ONE more Philox block at the sample's first counter, offset + 2 b, under
the stream STREAM_AUG_GATE | stream id << 32 (the caller's stream id in the high word) - word 0 gates the translation, word 1 the cutout, a stage is ON iff u < p with u the 24-bit uniform
(word >> 8) 2^-24 compared in float32.  A stage that is off gets OFF in t_h / o_x (csrc/step_inputs.hip, include/dusty_gan_hip.h)."""
import numpy as np

from tests import philox_ref as P

STREAM_AUG_GATE = 16
OFF = -2 ** 31


def gate_uniforms(seed, stream, offset, B):
    """[B, 2] float32: the translation's and the cutout's uniform of samples 0 .. B - 1"""
    ctr = (np.arange(B, dtype=np.uint64) * np.uint64(2)) + np.array([int(offset) & P.MASK64], dtype=np.uint64)
    return P.u24(P.philox4x32_10(seed, ctr, (STREAM_AUG_GATE | (int(stream) << 32)) & P.MASK64)[:, :2])


def gates(seed, stream, offset, B, p):
    """(translation on [B], cutout on [B])"""
    u = gate_uniforms(seed, stream, offset, B)
    on = u < np.float32(p)
    return on[:, 0], on[:, 1]


def augment_p(seed, stream, offset, B, H, W, p):
    """dg_aug_draw_p: (uf float32 [3,B], qi int32 [4,B]) with the sentinels in place; p == 1: philox_ref.augment itself"""
    uf, qi = P.augment(seed, stream, offset, B, H, W)
    if p != 1.0:
        g_t, g_c = gates(seed, stream, offset, B, p)
        qi = qi.copy()
        qi[0, ~g_t] = OFF
        qi[2, ~g_c] = OFF
    return uf, qi
