"""The controller's arithmetic (tests/ada_ref.py, the float32 restatement tests/test_gpu_ada.py holds csrc/ada.hip to): windows,
the clamp at 0 and at 1, and r_t == target, where the sign is 0 and p does not move.  No GPU."""
import numpy as np

from tests.ada_ref import Ada, F, signs


def test_signs_are_torch_signs_and_non_finite_counts_zero():
    import torch
    y = np.array([0.0, -0.0, 1e-30, -1e-30, 3.0, -2.0, np.inf, -np.inf, np.nan], dtype=np.float32)
    assert signs(y) == 0 and signs(y[:5]) == 1 and signs(y[6:]) == 0
    fin = y[np.isfinite(y)]
    assert signs(fin) == int(torch.sign(torch.from_numpy(fin)).sum())


def test_windows_move_p_once_per_interval():
    a = Ada(0.5, target=0.6, interval=4, kimg=0.04, batch_size=2)     # step = 2 * 4 / 40 = 0.2
    ps = []
    for it in range(12):
        y = np.ones(2, dtype=np.float32) if it < 8 else -np.ones(2, dtype=np.float32)
        rt, p = a.update(y)
        assert rt == (1.0 if it < 8 else -1.0)
        ps.append(float(p))
    want = [0.5] * 3 + [float(F(0.5) + F(0.2))] * 4 + [float(F(F(0.5) + F(0.2)) + F(0.2))] * 4
    want.append(float(F(F(F(0.5) + F(0.2)) + F(0.2)) - F(0.2)))
    assert ps == want and a.state()["steps"] == 12 and a.state()["count"] == 0 and a.state()["sign_sum"] == 0
    # mid-window: the sums are the window's
    a = Ada(0.5, interval=4, kimg=0.04, batch_size=2)
    for _ in range(6):
        a.update(np.array([1.0, -1.0, 1.0], dtype=np.float32))
    assert a.state()["steps"] == 6 and a.state()["count"] == 6 and a.state()["sign_sum"] == 2


def test_clamp_at_zero_and_at_one():
    up = Ada(0.9, target=0.0, interval=1, kimg=0.001, batch_size=1)   # step 1: one window reaches the clamp
    assert float(up.update(np.ones(4, dtype=np.float32))[1]) == 1.0
    assert float(up.update(np.ones(4, dtype=np.float32))[1]) == 1.0
    dn = Ada(0.1, target=0.0, interval=1, kimg=0.001, batch_size=1)
    assert float(dn.update(-np.ones(4, dtype=np.float32))[1]) == 0.0
    assert float(dn.update(-np.ones(4, dtype=np.float32))[1]) == 0.0
    assert float(dn.update(np.ones(4, dtype=np.float32))[1]) == 1.0


def test_rt_equal_to_target_does_not_move_p():
    a = Ada(0.37, target=0.5, interval=2, kimg=0.04, batch_size=4)
    y = np.array([1.0, 1.0, 1.0, -1.0], dtype=np.float32)              # mean sign 0.5 == target, exactly
    for _ in range(4):
        rt, p = a.update(y)
        assert rt == F(0.5) and p == F(0.37)
    a = Ada(0.37, target=0.0, interval=1, kimg=0.04, batch_size=4)
    assert a.update(np.array([np.nan, np.inf, 0.0, -0.0], dtype=np.float32))[1] == F(0.37)


def test_micro_batches_and_ranks_add_before_the_iteration_ends():
    """several calls per iteration (gradient accumulation, or ranks whose pending sums were added): one step, one window"""
    a, b = Ada(0.5, interval=1, kimg=0.04, batch_size=4), Ada(0.5, interval=1, kimg=0.04, batch_size=4)
    a.add(2, 2)
    a.add(-1, 2)
    b.add(1, 4)
    assert a.advance() == b.advance() and a.state() == b.state() and a.state()["steps"] == 1
