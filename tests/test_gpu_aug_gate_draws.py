"""dg_aug_draw_p / dg_aug_draw_p_dev and the step prologue's gated draw against the host restatement (tests/aug_gate_draw_ref.py):
the seven old numbers bit-equal wherever no sentinel stands, the gates a function of (seed, the sample's counter) alone, the counter
untouched by the draw, the device-resident p followed by a captured graph, and gate counts equal to the restatement's exactly."""
import numpy as np
import pytest
import torch

from tests import aug_gate_draw_ref as G
from tests import philox_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, STREAM = 0x1234_5678_9ABC_DEF1, 5
H, W = 64, 256
EPS = 2.0 ** -24
PS = [0.0, EPS, 0.3, 1.0 - EPS, 1.0]
BS = [1, 5, 256, 4096]
GUARD = 64


@pytest.fixture(scope="module")
def L():
    from dusty_gan_amd import _lib
    _lib.lib()
    assert _lib.DG_STREAM_AUG_GATE == G.STREAM_AUG_GATE and _lib.DG_AUG_OFF == G.OFF
    return _lib


def bufs(B):
    uf = torch.full((3 * B + GUARD,), -7.0, dtype=torch.float32, device=DEV)
    qi = torch.full((4 * B + GUARD,), -7, dtype=torch.int32, device=DEV)
    return uf, qi


def read(uf, qi, B):
    torch.cuda.synchronize()
    u, q = uf.cpu().numpy(), qi.cpu().numpy()
    assert (u[3 * B:] == -7.0).all() and (q[4 * B:] == -7).all(), "wrote behind its arrays"
    return u[:3 * B].reshape(3, B), q[:4 * B].reshape(4, B)


def draw(L, how, offset, B, p):
    """one gated draw through entry point `how` -> (uf [3,B], qi [4,B])"""
    lib = L.lib()
    uf, qi = bufs(B)
    ctr = torch.tensor([offset], dtype=torch.int64, device=DEV)
    if how == "host":
        L.check(lib.dg_aug_draw_p(SEED, STREAM, offset, B, H, W, p, uf.data_ptr(), qi.data_ptr(), None), "dg_aug_draw_p")
    elif how == "dev":
        pd = torch.tensor([p], dtype=torch.float32, device=DEV)
        L.check(lib.dg_aug_draw_p_dev(SEED, STREAM, ctr.data_ptr(), B, H, W, pd.data_ptr(), uf.data_ptr(), qi.data_ptr(), None),
                "dg_aug_draw_p_dev")
    else:   # the step prologue's kind-2 job, p a plain field or a device scalar
        d = L.DgDraw()
        d.kind, d.seed, d.stream_id, d.offset_dev, d.base = 2, SEED, STREAM, ctr.data_ptr(), 0
        d.B, d.H, d.W, d.uf, d.qi, d.p = B, H, W, uf.data_ptr(), qi.data_ptr(), p
        if how == "prologue_dev":
            pd = torch.tensor([p], dtype=torch.float32, device=DEV)
            d.p, d.p_dev = 1.0, pd.data_ptr()
        L.step_prologue([], [d])
    out = read(uf, qi, B)
    assert int(ctr.item()) == offset          # a draw never advances the counter: its caller does, by 2 per sample
    return out


@pytest.mark.parametrize("p", PS, ids=[f"p{i}" for i in range(len(PS))])
@pytest.mark.parametrize("B", BS)
def test_gated_draws_match_the_host_restatement(L, B, p):
    p32 = float(np.float32(p))
    for offset in (977, 2**32 - 5):
        uf_w, qi_w = G.augment_p(SEED, STREAM, offset, B, H, W, p32)
        uf_o, qi_o = P.augment(SEED, STREAM, offset, B, H, W)
        for how in ("host", "dev", "prologue", "prologue_dev"):
            uf, qi = draw(L, how, offset, B, p32)
            assert np.array_equal(uf, uf_w) and np.array_equal(qi, qi_w), (how, offset)
            # the seven old numbers, wherever no sentinel stands
            keep = qi != G.OFF
            assert np.array_equal(uf, uf_o) and np.array_equal(qi[keep], qi_o[keep]), (how, offset)
            assert not (qi[1] == G.OFF).any() and not (qi[3] == G.OFF).any()
            # gate counts: the restatement's, exactly
            g_t, g_c = G.gates(SEED, STREAM, offset, B, p32)
            assert int((qi[0] != G.OFF).sum()) == int(g_t.sum()) and int((qi[2] != G.OFF).sum()) == int(g_c.sum())
            if p == 1.0:
                assert keep.all()
            if p == 0.0:
                assert (qi[0] == G.OFF).all() and (qi[2] == G.OFF).all()
    if B == 4096 and p == 0.3:        # neither gate is the other's, and the rate is p's (a sanity line, not the criterion)
        g_t, g_c = G.gates(SEED, STREAM, 977, B, p32)
        print(f"[aug-gate-draws] B 4096 p 0.3: translation on {int(g_t.sum())}, cutout on {int(g_c.sum())}, both {int((g_t & g_c).sum())}")
        assert not np.array_equal(g_t, g_c)


def test_the_edge_uniforms_decide_as_u_less_than_p(L):
    """u < p on the host restatement's own uniforms: p = 2^-24 switches on exactly the samples with u == 0, p = 1 - 2^-24 switches
    off exactly those with u == 1 - 2^-24 (whether or not this seed has any: the draw test above holds the kernel to the same)"""
    u = G.gate_uniforms(SEED, STREAM, 977, 4096)
    lo = u < np.float32(EPS)
    hi = u < np.float32(1.0 - EPS)
    assert np.array_equal(lo, u == 0) and np.array_equal(~hi, u == np.float32(1.0 - EPS))


def test_streams_of_one_seed_gate_apart(L):
    """the caller's stream id is part of the gate block's key: the same seed and counters on another stream draw other gates, the
    host restatement's for that stream"""
    lib = L.lib()
    B, offset, p = 256, 977, float(np.float32(0.5))
    got = {}
    for stream in (STREAM, STREAM + 1):
        uf, qi = bufs(B)
        L.check(lib.dg_aug_draw_p(SEED, stream, offset, B, H, W, p, uf.data_ptr(), qi.data_ptr(), None), "dg_aug_draw_p")
        _, q = read(uf, qi, B)
        assert np.array_equal(q, G.augment_p(SEED, stream, offset, B, H, W, p)[1]), stream
        got[stream] = (q[0] == G.OFF, q[2] == G.OFF)
    assert not np.array_equal(got[STREAM][0], got[STREAM + 1][0]) and not np.array_equal(got[STREAM][1], got[STREAM + 1][1])


def test_old_entry_points_draw_no_gates(L):
    lib = L.lib()
    B, offset = 256, 977
    uf_w, qi_w = P.augment(SEED, STREAM, offset, B, H, W)
    uf, qi = bufs(B)
    L.check(lib.dg_aug_draw(SEED, STREAM, offset, B, H, W, uf.data_ptr(), qi.data_ptr(), None))
    u, q = read(uf, qi, B)
    assert np.array_equal(u, uf_w) and np.array_equal(q, qi_w)
    for bad in (-0.1, 1.5, float("nan")):
        assert lib.dg_aug_draw_p(SEED, STREAM, offset, B, H, W, bad, uf.data_ptr(), qi.data_ptr(), None) == L.DG_EINVAL


def test_gates_depend_on_the_samples_counter_alone(L):
    """sample b's gates are the same in a batch of 5 and of 4096, and at every position of a draw_sets(n) launch: set k, sample b
    sits at counter offset + 2 (k B + b), whichever launch draws it"""
    from dusty_gan_amd.utils.diff_augment import DiffAugment
    p, offset = 0.3, 977
    _, q_big = draw(L, "host", offset, 4096, p)
    _, q_small = draw(L, "host", offset, 5, p)
    assert np.array_equal(q_small, q_big[:, :5])
    A = DiffAugment(p=p, seed=SEED)
    B, n = 6, 4
    sets = A.draw_sets(n, B, H, W, DEV)
    assert A.rng(DEV).offset == 2 * n * B          # the counter advance is p = 1's
    A2 = DiffAugment(p=p, seed=SEED)
    for k in range(n):
        one = A2.draw(B, H, W, DEV)
        for key in one:
            assert torch.equal(one[key], sets[k][key]), (k, key)
        _, qw = G.augment_p(SEED, 5, 2 * k * B, B, H, W, float(np.float32(p)))
        assert np.array_equal(torch.stack([one[x] for x in ("t_h", "t_w", "o_x", "o_y")]).cpu().numpy(), qw)
    assert A2.rng(DEV).offset == 2 * n * B
    # p = 1: the module draws what it always drew
    A1, A0 = DiffAugment(p=1.0, seed=SEED), DiffAugment(seed=SEED)
    a, b = A1.draw(B, H, W, DEV), A0.draw(B, H, W, DEV)
    assert all(torch.equal(a[k], b[k]) for k in a) and not any(bool((a[k] == G.OFF).any()) for k in ("t_h", "o_x"))


def test_constructor_takes_p_in_range():
    from dusty_gan_amd.utils.diff_augment import DiffAugment
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError):
            DiffAugment(p=bad)
    assert DiffAugment(p=0.0).p == 0.0 and DiffAugment(p=0.5).p == 0.5


def test_params_to_device_passes_the_sentinel_through():
    from dusty_gan_amd.utils.diff_augment import AUG_OFF, DiffAugment
    rp = {"t_h": torch.tensor([G.OFF, 1]), "t_w": torch.tensor([3, 4]), "o_x": torch.tensor([2, G.OFF]), "o_y": torch.tensor([0, 0]),
          "u_b": torch.tensor([0.5, -0.5], dtype=torch.float64)}
    out = DiffAugment.params_to_device(rp, DEV)
    assert AUG_OFF == G.OFF and out["t_h"].dtype == torch.int32 and out["t_h"].tolist() == [G.OFF, 1] and out["o_x"].tolist() == [2, G.OFF]


def test_dev_form_in_a_captured_graph_follows_p(L):
    """p is read when the draw runs: a graph captured once draws with whatever the memory holds at each replay"""
    lib = L.lib()
    B, offset = 256, 977
    uf, qi = bufs(B)
    ctr = torch.tensor([offset], dtype=torch.int64, device=DEV)
    pd = torch.tensor([1.0], dtype=torch.float32, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        L.check(lib.dg_aug_draw_p_dev(SEED, STREAM, ctr.data_ptr(), B, H, W, pd.data_ptr(), uf.data_ptr(), qi.data_ptr(),
                                      L.stream_ptr()))   # (warm-up: the module is loaded before the capture)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        L.check(lib.dg_aug_draw_p_dev(SEED, STREAM, ctr.data_ptr(), B, H, W, pd.data_ptr(), uf.data_ptr(), qi.data_ptr(),
                                      L.stream_ptr()))
    for p in (1.0, 0.3, 0.0, 0.7):
        pd.fill_(p)
        g.replay()
        u, q = read(uf, qi, B)
        uf_w, qi_w = G.augment_p(SEED, STREAM, offset, B, H, W, float(np.float32(p)))
        if p == 1.0:     # (the device form always draws its gates: at p = 1 none is off)
            uf_w, qi_w = P.augment(SEED, STREAM, offset, B, H, W)
        assert np.array_equal(u, uf_w) and np.array_equal(q, qi_w), p
