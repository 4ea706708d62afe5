"""Every Philox draw of the training path - csrc/step_inputs.hip's three bodies through each of their entry points, the
consumers that call the host-offset entry, and a whole Trainer.step - against the host reference (tests/philox_ref.py), element
by element: raw bits, uniforms and integers bit for bit, normals and logistic noise to bounds derived from the fp32 operations
that form them.  The worst error seen is printed as a fraction of its bound."""
import functools

import numpy as np
import pytest
import torch

from tests import philox_ref as P
from tests.test_philox_ref_cpu import EDGE_ONES, EDGE_ZERO, SEED, STREAM

pytestmark = pytest.mark.gpu

DEV = "cuda"
OFFSETS = [977, 2**32 - 2, EDGE_ZERO, EDGE_ONES]
OFFSET_IDS = ["977", "carry", "edge-zero", "edge-ones"]
SIZES = [1, 2, 3, 4, 5, 1023, 4099]
NMAX = max(SIZES)
MARGIN = 4
WORST = {"normal": (0.0, 0.0), "logistic": 0.0}


@pytest.fixture(scope="module")
def L():
    from dusty_gan_amd import _lib
    _lib.lib()
    return _lib


def host(t):
    return t.detach().cpu().numpy()


def check_normal(got, want, rad, what):
    """|got - want| <= 2^-20 max(rad, 1) per element (philox_ref.NORMAL_TOL: how the bound is built)"""
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    ratio = float((err / P.normal_bound(rad)).max())
    rel = float((err / np.maximum(rad, 1e-30))[rad > 0].max()) if (rad > 0).any() else 0.0
    WORST["normal"] = (max(WORST["normal"][0], ratio), max(WORST["normal"][1], rel))
    print(f"normal {what}: worst error {ratio:.3f} of the bound, |err| / rad {rel:.3e}"
          f" (so far {WORST['normal'][0]:.3f}, {WORST['normal'][1]:.3e})")
    assert ratio <= 1.0, (what, ratio)


def check_logistic(got, want, what):
    """finite, and |got - want| <= 2^-20 max(1, |want|) per element (philox_ref.LOGISTIC_TOL)"""
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), what
    ratio = float((np.abs(got - want) / P.logistic_bound(want)).max())
    WORST["logistic"] = max(WORST["logistic"], ratio)
    print(f"logistic {what}: worst error {ratio:.3f} of the bound (so far {WORST['logistic']:.3f})")
    assert ratio <= 1.0, (what, ratio)


# ---- raw bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 977, 2**32 - 5, 2**33 + 1, 2**64 - 3])
def test_raw_bits(L, offset):
    """dg_philox_bits over three blocks (two full, one partial); 2^32 - 5 carries into the counter's second word and 2^64 - 3
    wraps to 0 inside the launch"""
    lib, n4 = L.lib(), 600
    out = torch.empty(4 * n4 + MARGIN, dtype=torch.int32, device=DEV)
    for stream in (0, 5, 2**32 + 7, 2**64 - 1):
        for seed in (0, SEED, 2**63 + 11):
            out.fill_(-7)
            L.check(lib.dg_philox_bits(seed, stream, offset, n4, out.data_ptr(), None), "dg_philox_bits")
            got = host(out)
            assert np.array_equal(got[:4 * n4].view(np.uint32), P.words(seed, stream, offset, n4).reshape(-1)), (stream, seed)
            assert (got[4 * n4:] == -7).all()


# ---- fills -------------------------------------------------------------------------------------------------------------------------
KIND3 = [(-3, 19), (0, 2**31 - 1)]      # (the second: corruption.random_rows' own range)
LO, HI = -0.75, 2.5


@functools.lru_cache(maxsize=None)
def fill_ref(offset):
    """every kind at NMAX elements from `offset`, made once; element o of a fill does not depend on n"""
    return {"u": P.uniform(SEED, STREAM, offset, NMAX), "range": P.uniform_range(SEED, STREAM, offset, NMAX, LO, HI),
            "normal": P.normal(SEED, STREAM, offset, NMAX), "logistic": {n: P.logistic(SEED, STREAM, offset, n) for n in LOGISTIC_SIZES},
            "int": [P.integers(SEED, STREAM, offset, NMAX, a, b) for a, b in KIND3]}


def fills(L, offset, kind, n, ilo=0, ihi=1):
    """dg_philox_fill and dg_philox_fill_dev on buffers with a margin behind n -> the two results (margins checked)"""
    lib = L.lib()
    dt = torch.int32 if kind == 3 else torch.float32
    ctr = torch.tensor([offset], dtype=torch.int64, device=DEV)
    a = torch.full((n + MARGIN,), -7, dtype=dt, device=DEV)
    b = a.clone()
    L.check(lib.dg_philox_fill(SEED, STREAM, offset, kind, LO, HI, ilo, ihi, n, a.data_ptr(), None), "dg_philox_fill")
    L.check(lib.dg_philox_fill_dev(SEED, STREAM, ctr.data_ptr(), kind, LO, HI, ilo, ihi, n, b.data_ptr(), None), "dg_philox_fill_dev")
    a, b = host(a), host(b)
    assert (a[n:] == -7).all() and (b[n:] == -7).all(), (kind, n)
    assert int(ctr.item()) == offset
    return a[:n], b[:n]


@pytest.mark.parametrize("offset", OFFSETS, ids=OFFSET_IDS)
def test_fills_exact_kinds(L, offset):
    """kind 0 and kind 3 bit for bit; kind 2 one of the two fp32 evaluations of lo + (hi - lo) u"""
    ref = fill_ref(offset)
    for n in SIZES:
        for got in fills(L, offset, 0, n):
            assert np.array_equal(got, ref["u"][:n]), n
        for (ilo, ihi), want in zip(KIND3, ref["int"]):
            for got in fills(L, offset, 3, n, ilo, ihi):
                assert np.array_equal(got, want[:n]), (n, ilo, ihi)
        twice, once = ref["range"]
        for got in fills(L, offset, 2, n):
            assert ((got == twice[:n]) | (got == once[:n])).all(), n
    if offset == EDGE_ZERO:
        assert fills(L, offset, 0, 1)[0][0] == 0.0
    if offset == EDGE_ONES:
        assert fills(L, offset, 0, 1)[0][0] == np.float32(1.0 - 2.0 ** -24)


@pytest.mark.parametrize("offset", OFFSETS, ids=OFFSET_IDS)
def test_fills_normal(L, offset):
    want, rad = fill_ref(offset)["normal"]
    for n in SIZES:
        for entry, got in zip(("host offset", "device offset"), fills(L, offset, 1, n)):
            check_normal(got, want[:n], rad[:n], f"offset {offset} n {n} {entry}")
            if offset == EDGE_ZERO:      # u1 = 1: the radius is sqrt(-2 ln 1) = 0 and both elements of the pair are 0
                assert rad[0] == 0.0 and got[0] == 0.0 and (n < 2 or got[1] == 0.0)
    if offset == EDGE_ONES:
        assert abs(rad[0] - 5.7682) < 1e-4   # u1 = 2^-24: the largest radius there is, covered by the loop above


# ---- logistic noise ----------------------------------------------------------------------------------------------------------------
LOGISTIC_SIZES = (1, 5, 315, 4099)


@pytest.mark.parametrize("offset", OFFSETS, ids=OFFSET_IDS)
def test_logistic_from_the_generator(L, offset):
    """dg_philox_logistic_dev: U2's counters start ceil(n / 4) behind U1's.  At the edge-zero offset element 0 has
    ln(u1 + eps) = ln(eps)."""
    lib = L.lib()
    ctr = torch.tensor([offset], dtype=torch.int64, device=DEV)
    for n in LOGISTIC_SIZES:
        out = torch.full((n + MARGIN,), -7.0, device=DEV)
        L.check(lib.dg_philox_logistic_dev(SEED, STREAM, ctr.data_ptr(), P.EPS, n, out.data_ptr(), None), "dg_philox_logistic_dev")
        got = host(out)
        assert (got[n:] == -7.0).all()
        check_logistic(got[:n], fill_ref(offset)["logistic"][n], f"offset {offset} n {n}")
    assert int(ctr.item()) == offset


def test_logistic_of_given_uniforms(L):
    """dg_logistic_noise on all 16 pairs of u in {0, 2^-24, 0.5, 1 - 2^-24} and 4 096 pairs of 24-bit uniforms"""
    edge = np.float32([0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24])
    u1 = np.concatenate([np.repeat(edge, 4), P.uniform(7, 2, 0, 4096)])
    u2 = np.concatenate([np.tile(edge, 4), P.uniform(7, 2, 1024, 4096)])
    n = u1.size
    a, b = torch.from_numpy(u1).to(DEV), torch.from_numpy(u2).to(DEV)
    out = torch.full((n + MARGIN,), -7.0, device=DEV)
    L.check(L.lib().dg_logistic_noise(a.data_ptr(), b.data_ptr(), P.EPS, n, out.data_ptr(), None), "dg_logistic_noise")
    got = host(out)
    assert (got[n:] == -7.0).all()
    want = P.logistic_of(u1, u2)
    check_logistic(got[:16], want[:16], "the 16 edge pairs")
    check_logistic(got[16:n], want[16:], "4096 pairs")


# ---- DiffAugment parameters ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(37, 64, 1024), (5, 10, 36), (4096, 7, 9), (3, 2, 2)])
def test_augment_draws(L, B, H, W):
    """dg_aug_draw and dg_aug_draw_dev bit for bit, geometry from the reference's own formulas (odd sizes: every rounding in
    it); 2^32 - 5: the carry between a sample's two counters"""
    lib = L.lib()
    for offset in (977, 2**32 - 5):
        uf_w, qi_w = P.augment(SEED, STREAM, offset, B, H, W)
        ctr = torch.tensor([offset], dtype=torch.int64, device=DEV)
        for dev in (False, True):
            uf = torch.full((3 * B + MARGIN,), -7.0, device=DEV)
            qi = torch.full((4 * B + MARGIN,), -77, dtype=torch.int32, device=DEV)
            if dev:
                L.check(lib.dg_aug_draw_dev(SEED, STREAM, ctr.data_ptr(), B, H, W, uf.data_ptr(), qi.data_ptr(), None), "dg_aug_draw_dev")
            else:
                L.check(lib.dg_aug_draw(SEED, STREAM, offset, B, H, W, uf.data_ptr(), qi.data_ptr(), None), "dg_aug_draw")
            uf, qi = host(uf), host(qi)
            assert np.array_equal(uf[:3 * B].reshape(3, B), uf_w) and np.array_equal(qi[:4 * B].reshape(4, B), qi_w), (offset, dev)
            assert (uf[3 * B:] == -7.0).all() and (qi[4 * B:] == -77).all()
            if B == 4096 and offset == 977:
                # each integer field reaches both ends of the REFERENCE's range and nothing outside it
                # (tests/test_philox_ref_cpu.py: the host reference does at this seed)
                sh, sw, nx, ny = P.aug_geometry(H, W)
                for row, (lo, hi) in zip(qi[:4 * B].reshape(4, B), ((-sh, sh), (-sw, sw), (0, nx - 1), (0, ny - 1))):
                    assert row.min() == lo and row.max() == hi


# ---- consumers of the host-offset entry -----------------------------------------------------------------------------------------------
def test_corruption_draws(L):
    """corruption._draw: scan first_index + b takes counters from (first_index + b) ceil(HW / 4) of the corruptions' stream"""
    from dusty_gan_amd import corruption as K
    from tests.corruption_util import mask_corrupt
    B, H, W, first, seed = 3, 5, 37, 5, 2
    HW, g4 = H * W, P.groups(H * W)
    like = torch.empty(B, 1, H, W, device=DEV)
    u, z = host(K._draw(0, seed, first, like)), host(K._draw(1, seed, first, like))
    for b in range(B):
        off = (first + b) * g4
        assert np.array_equal(u[b].reshape(-1), P.uniform(seed, K.STREAM_CORRUPT, off, HW)), b
        want, rad = P.normal(seed, K.STREAM_CORRUPT, off, HW)
        check_normal(z[b].reshape(-1), want, rad, f"corruption row {b}")
    mask = (torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(5)) < 0.7).float()
    got = K.dropout_noise(mask.to(DEV), 0.1, seed=seed, first_index=first)
    u_host = np.stack([P.uniform(seed, K.STREAM_CORRUPT, (first + b) * g4, HW) for b in range(B)]).reshape(B, 1, H, W)
    want = mask_corrupt(mask, u=torch.from_numpy(u_host), rate=0.1)
    assert torch.equal(got.cpu(), want) and 0 < float(want.sum()) < float(mask.sum())
    # random_lines' rows: a stable ascending order of H keys in [0, 2^31 - 1), the first int(H (1 - rate)) of them
    keys = P.integers(3, K.STREAM_CORRUPT, 0, 16, 0, 2**31 - 1)
    rows = np.argsort(keys, kind="stable")[:8]
    assert K.random_rows(16, 0.5, seed=3).tolist() == rows.tolist()


def test_inversion_draws(L):
    """inversion's latent and Gumbel-noise helpers: counter 0 of their own streams"""
    from dusty_gan_amd import inversion as I
    dev = torch.device(DEV)
    for n in (5, 315):
        want, rad = P.normal(SEED, I.STREAM_LATENT, 0, n)
        check_normal(host(I._draw_normal(SEED, I.STREAM_LATENT, n, dev)), want, rad, f"inversion latent n {n}")
        check_logistic(host(I._draw_logistic(SEED, I.STREAM_GUMBEL, n, P.EPS, dev)), P.logistic(SEED, I.STREAM_GUMBEL, 0, n),
                       f"inversion gumbel n {n}")


# ---- a whole step's counters -------------------------------------------------------------------------------------------------------------
STEPS = 5


def _maskers(tr):
    """G's Gumbel-sigmoid modules (G_ema is a copy of G: its modules are keyed like G's by construction)"""
    from dusty_gan_amd.models.dusty import GumbelSigmoid
    return [m for m in tr.G.modules() if isinstance(m, GumbelSigmoid)]


def _owned(tr):
    """{name: (seed, stream id)} of every generator the trainer owns (the fixed evaluation latents come from `rng`)"""
    out = {"rng": tr.rng, "augment": tr.A._rng if tr.A._rng is not None else tr.A.rng(tr.device)}
    for i, m in enumerate(_maskers(tr)):
        out[f"masker{i}"] = m.rng(tr.device)
    return {k: (r.seed, r.stream_id) for k, r in out.items()}


def _step_run(monkeypatch, graph, amp):
    """five steps of the issue's trainer; per step the counters before and after and every draw the step made, checked against
    the host reference -> what the graph run is compared with the eager run on"""
    from tests.test_gpu_step import make_trainer
    monkeypatch.setenv("DUSTY_GAN_GRAPH", "1" if graph else "0")
    torch.manual_seed(2024)
    tr = make_trainer("dusty2", True, (32, 64), 8, 4, 16, 4, amp=amp)
    B, nz, H, W = 4, 8, 32, 64
    made = []                                   # one entry per call of a drawing function: the tensors it filled

    def keep(pre):
        made.append({"z": pre["z"], "noise": pre["noise"], "aug": pre["aug"], "B": pre.get("B", B)})

    jobs, rand = tr._draw_jobs, tr._draw_rand

    def draw_jobs(n):
        out = jobs(n)
        keep(tr._predrawn)
        return out

    def draw_rand(n):
        out = rand(n)
        keep(dict(out, B=n))
        return out
    monkeypatch.setattr(tr, "_draw_jobs", draw_jobs)
    monkeypatch.setattr(tr, "_draw_rand", draw_rand)

    # The augment generator does not exist before the first step draws from it, and this test must not make it: a generator
    # queues its counter advances with the owner that is current when it is created (utils/rng.py), and one made here, outside
    # the trainer's entry points, would advance outside the captured step.
    r = tr.rng
    assert tr.A._rng is None
    aug_offset = lambda: 0 if tr.A._rng is None else tr.A._rng.offset
    # the fixed evaluation latents: the first draw of `rng`
    spans = {(r.seed, r.stream_id): [P.fill_range(0, B * nz)]}
    want, rad = P.normal(r.seed, r.stream_id, 0, B * nz)
    check_normal(host(tr.fixed_noise).reshape(-1), want, rad, "fixed evaluation latents")
    assert r.offset == spans[(r.seed, r.stream_id)][0][1]
    record = []
    for i in range(STEPS):
        before = (r.offset, aug_offset())
        n_made = len(made)
        tr.step(i)
        torch.cuda.synchronize()
        after = (r.offset, aug_offset())
        ra = tr.A._rng
        spans.setdefault((ra.seed, ra.stream_id), [])
        # a replayed step runs no Python: its draws land in the buffers of the captured call, the last one recorded
        calls = made[n_made:] if len(made) > n_made else made[-1:]
        replayed = len(made) == n_made
        assert replayed == (graph and i > 2), (i, len(made))
        at, at_aug, step_rec = before[0], before[1], {"before": before, "after": after}
        for c, call in enumerate(calls):
            assert call["B"] == B
            # (a) z, pixel noise, image noise: consecutive counter ranges of `rng`
            z = host(call["z"]).reshape(-1)
            want, rad = P.normal(r.seed, r.stream_id, at, B * nz)
            check_normal(z, want, rad, f"step {i} z")
            span = [P.fill_range(at, B * nz)]
            at = span[-1][1]
            assert set(call["noise"]) == {"pixel", "image"}
            for k, n in (("pixel", B * H * W), ("image", B)):
                check_logistic(host(call["noise"][k]).reshape(-1), P.logistic(r.seed, r.stream_id, at, n), f"step {i} {k} noise")
                span.append(P.logistic_range(at, n))
                at = span[-1][1]
            spans[(r.seed, r.stream_id)] += span
            # ... and the four DiffAugment sets: 2 counters per sample of the augment generator, set k sample b at 2 (k B + b)
            uf, qi = P.augment(ra.seed, ra.stream_id, at_aug, 4 * B, H, W)
            assert len(call["aug"]) == 4
            for k, s in enumerate(call["aug"]):
                sl = slice(k * B, (k + 1) * B)
                for j, name in enumerate(("u_b", "u_s", "u_c")):
                    assert np.array_equal(host(s[name]), uf[j, sl]), (i, k, name)
                for j, name in enumerate(("t_h", "t_w", "o_x", "o_y")):
                    assert np.array_equal(host(s[name]), qi[j, sl]), (i, k, name)
            spans[(ra.seed, ra.stream_id)].append(P.aug_range(at_aug, 4 * B))
            at_aug = spans[(ra.seed, ra.stream_id)][-1][1]
            step_rec[f"z{c}"], step_rec[f"pixel{c}"], step_rec[f"aug{c}"] = z, host(call["noise"]["pixel"]).copy(), (uf, qi)
        # the generator's input in its compute dtype: the last latents drawn
        zT = tr._g_engines()[0].zT
        assert zT.dtype == (torch.bfloat16 if amp else torch.float32)
        assert torch.equal(zT.view(-1), calls[-1]["z"].view(-1).to(zT.dtype)), i
        # (b) the counters end where the verified ranges end: nothing else was drawn
        assert after == (at, at_aug), (i, before, after, at, at_aug)
        record.append(step_rec)
    assert (tr._graph is not None) == graph
    # (c) the verified ranges of one (seed, stream id) are pairwise disjoint
    for key, sp in spans.items():
        sp = sorted(sp)
        assert all(a[0] < a[1] for a in sp) and all(a[1] <= b[0] for a, b in zip(sp, sp[1:])), (key, sp)
    own = _owned(tr)
    assert len(set(own.values())) == len(own), own
    return record


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16"])
def test_a_step_draws_what_the_host_reference_says(monkeypatch, amp):
    """(a) every tensor a step draws - latents with their copy in the compute dtype, pixel and image noise, four DiffAugment
    sets - is the host reference's at (seed, stream id, counter before the step + what the earlier draws took); (b) the
    counters end where those ranges end; (c) no two ranges of a generator overlap and no two generators share a (seed,
    stream id); (d) replayed from a hipGraph the step reads the same counters and draws the same bits as launched eagerly."""
    eager = _step_run(monkeypatch, False, amp)
    graph = _step_run(monkeypatch, True, amp)
    for i, (a, b) in enumerate(zip(eager, graph)):
        assert a["before"] == b["before"] and a["after"] == b["after"], i
        assert sorted(a) == sorted(b), i
        for k in a:
            if k[0] in "zp":
                assert np.array_equal(a[k], b[k]), (i, k)


def test_ranks_draw_from_distinct_streams(monkeypatch):
    """two ranks of one job (same job seed): no generator that feeds a training step shares its (seed, stream id) with any
    generator of the other rank.  (The maskers' own generators serve evaluation outside a step and are keyed by the process's
    torch seed, not by the rank: they are held apart from every rank-keyed one, not from their twin on the other rank.)"""
    from dusty_gan_amd.trainers import dcgan_amp
    from tests.test_gpu_step import make_trainer
    pairs = []
    for rank in (0, 1):
        monkeypatch.setattr(dcgan_amp, "_rank", lambda rank=rank: rank)
        torch.manual_seed(2024)
        pairs.append(_owned(make_trainer("dusty2", True, (32, 64), 8, 4, 16, 4)))
    step = [v for p in pairs for k, v in p.items() if not k.startswith("masker")]
    assert len(step) == 4 and len(set(step)) == 4, pairs
    maskers = {v for p in pairs for k, v in p.items() if k.startswith("masker")}
    assert maskers and not (maskers & set(step)), pairs
