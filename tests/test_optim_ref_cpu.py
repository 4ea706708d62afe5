"""tests/optim_ref.py on the CPU: (a) a float32 restatement of each formula - numpy float32, one operation at a time, no FMA, numpy's
float32 power and 1 / sqrt - stays inside every criterion on every input class and every step count tests/test_gpu_optim.py uses
(the reference and its bounds alone are consistent), and (b) every wrong variant an almost-right kernel produces fails a criterion,
with the written proof of the gap: which of them pass the rel-L2 thresholds of tests/test_gpu_ops.py::test_losses_fetch_reals_adam
on that test's own inputs.  Run with -s to read the lists."""
import numpy as np
import pytest
import torch

from dusty_gan_amd.inversion import adam_table
from tests import optim_ref as R
from tests.golden_util import rel_l2

F = np.float32
HOST_STEPS = (1, 2, 4, 100, 10 ** 6)
DEV_STEPS = (1, 2, 3, 4, 5, 6, 70, 100, 1000, 10 ** 6)
BETA1 = (0.0, 0.5, 0.9)
NUM_STEP = 20
SPHERE_K = (0, 1, 5, NUM_STEP, NUM_STEP + 3)
B1T, B2T, EPST = 0.9, 0.999, 1e-8                   # torch.optim.Adam's defaults, as the inversion passes them


# ---- the float32 restatements, with the wrong variants as switches ----------------------------------------------------------------
def adam_f32(inp, t, hp, dev, variant=None, has_m=True, has_ema=True):
    """adam_ema_kernel in numpy float32.  dev: the bias corrections from float32 power / 1 / sqrt at t, else the host's factors."""
    lr, b1, b2, eps, d, gs = (F(x) for x in (hp.lr, hp.b1, hp.b2, hp.eps, hp.d, hp.gscale))
    one = F(1)
    tt = {"t + 1": t + 1, "t - 1": t - 1}.get(variant, t)
    if dev:
        tf = F(tt)
        lr_bc1 = lr / (one - np.power(b1, tf)) if b1 > 0 else lr
        isb = one / np.sqrt(one - np.power(b2, tf))
    else:
        h = R.HP(hp.lr, hp.b1, hp.b2, hp.eps, hp.d, hp.gscale).host_factors(tt)
        lr_bc1, isb = F(h[0]), F(h[1])
    if variant == "no bc2":
        isb = one
    if variant == "bc1 ignored":
        lr_bc1 = lr
    g, v, p = inp.g, inp.v.copy(), inp.p
    if variant == "lane 3 reads lane 2's v":
        v[3::4] = inp.v[2::4]
    gg = g * gs
    m = inp.m if (has_m and inp.m is not None) else np.zeros_like(g)
    m1 = b1 * m + (one - b1) * gg
    gv = g if variant == "v' from the unscaled gradient" else gg
    v1 = b2 * v + ((one - b2) * gv) * gv
    if variant == "eps dropped":
        D = np.sqrt(v1) * isb
    elif variant == "eps inside the square root":
        D = np.sqrt(v1 + eps) * isb
    elif variant == "eps before the bias correction":
        D = (np.sqrt(v1) + eps) * isb
    else:
        D = np.sqrt(v1) * isb + eps
    with np.errstate(divide="ignore", invalid="ignore"):
        p1 = p - lr_bc1 * (m1 / D)
    out = {"p": p1, "v": v1, "m": m1 if has_m and inp.m is not None else None, "ema": None}
    if has_ema:
        if variant == "ema from the old p":
            out["ema"] = d * inp.ema + (one - d) * p
        elif variant == "d and 1 - d swapped":
            out["ema"] = (one - d) * inp.ema + d * p1
        else:
            out["ema"] = d * inp.ema + (one - d) * p1
    assert all(a is None or a.dtype == np.float32 for a in out.values())
    return out


def table_f32(x, g, m, v, row, variant=None):
    """alpha_adam_kernel / the first half of sphere_adam_kernel in numpy float32"""
    b1, b2, eps, one = F(B1T), F(B2T), F(EPST), F(1)
    step, bc2s = F(row[0]), F(row[1])
    m1 = m + (one - b1) * (g - m)
    v1 = v * b2 + ((one - b2) * g) * g
    return x - step * (m1 / (np.sqrt(v1) / bc2s + eps)), m1, v1


def sphere_f32(s, sched, k, variant=None):
    x1, m1, v1 = table_f32(s.latent, s.g, s.m, s.v, sched[min(k, NUM_STEP)])
    ms = np.add.reduce(x1 * x1, axis=1, keepdims=True) / F(x1.shape[1])
    sc = np.sqrt(ms if variant == "renormalisation without the 1e-9" else ms + F(1e-9))
    return {"latent": x1 / sc, "m": m1, "v": v1}


def sched_table():
    return adam_table(0.1, NUM_STEP, 0.05, 0.25).numpy()


# ---- (a) the restatement stays inside the criteria -----------------------------------------------------------------------------
@pytest.mark.parametrize("b1", BETA1)
@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_float32_restatement_of_adam_ema_is_inside_every_criterion(dev, b1):
    for d in (0.9, 1.0):
        hp = R.HP(b1=b1, d=d)
        for t in (DEV_STEPS if dev else HOST_STEPS):
            inp = R.Inputs(2800, 11 + t % 97, hp, with_m=True)
            for has_m in ((True,) if b1 > 0 else (True, False)):
                fac = {} if dev else dict(zip(("lr_bc1", "isb"), hp.host_factors(t)))
                r = R.adam_ref(inp.p, inp.g, inp.m if has_m else None, inp.v, inp.ema, t, hp, **fac)
                R.assert_normal(r)
                got = adam_f32(inp, t, hp, dev, has_m=has_m)
                q = R.check(f"float32 restatement t={t}", got, r, R.bounds(r, R.A_DEV if dev else R.A_HOST, R.POW_ULPS if dev else 0),
                            inp.cls)
                R.check_class_facts("float32 restatement", got, inp, hp, True)
                assert max(q.values()) <= 1.0
    # every class on every lane, in both halves
    seen = {(int(c), int(i) % 4, bool(z)) for c, i, z in zip(inp.cls[:64], np.arange(64), inp.p[:64] == 0)}
    assert {(c, ln) for c, ln, _ in seen} == {(c, ln) for c in range(7) for ln in range(4)}
    assert all(len({(c, ln) for c, ln, z in seen if z == zz}) == 28 for zz in (True, False))


def test_float32_restatement_of_the_fused_gradient_is_inside_its_bound():
    rng = np.random.default_rng(3)
    hp = R.HP()
    inp = R.Inputs(1024, 5, hp)
    for splits, acc, ws_n in ((0, 1, 0), (1, 0, 0), (9, 1, 0), (64, 0, 9), (129, 1, 0), (0, 0, 1)):
        w = rng.uniform(-1, 1, (max(splits, 1), 1)).astype(F)
        parts = (inp.g[None] * w).astype(F) if splits else None
        g0 = inp.g if acc else None
        src = (inp.g[None] * rng.uniform(-1, 1, (ws_n, 1))).astype(F) if ws_n else None
        coef = rng.uniform(0.5, 2, ws_n).astype(F) if ws_n else None
        want, bound = R.fused_grad_ref(parts, g0, src, coef, 0.25)
        acc32 = np.zeros(1024, F)
        for s in range(splits):
            acc32 = acc32 + parts[s]
        if acc:
            acc32 = acc32 + g0
        if ws_n:
            ws = np.zeros(1024, F)
            for b in range(ws_n):
                ws = ws + coef[b] * src[b]
            acc32 = acc32 + F(0.25) * ws
        bad, q = R.ratio_of(acc32, want, bound)
        assert not bad.any() and q <= 1.0, (splits, acc, ws_n, q)
        # a row left out, or the neighbouring element's row: outside
        if splits:
            assert R.ratio_of(acc32 - parts[-1], want, bound)[0].any()


@pytest.mark.parametrize("nz,B", [(1, 1), (100, 3), (257, 3), (1024, 70)])
def test_float32_restatement_of_sphere_and_alpha_adam_is_inside_every_criterion(nz, B):
    sched = sched_table()
    s = R.sphere_inputs(B, nz, 100 + nz)
    for k in SPHERE_K:
        r = R.sphere_ref(s.latent, s.g, s.m, s.v, sched, k, NUM_STEP, B1T, B2T, EPST)
        R.assert_normal(r)
        got = sphere_f32(s, sched, k)
        q = R.check_sphere(f"sphere restatement k={k}", got, r, R.sphere_bounds(r), s.cls)
        assert max(q.values()) <= 1.0
        if k in (0, NUM_STEP):                       # no step: the scale read back from the rows is the float32 scale that divided them
            assert "scale" in q
            x1 = s.latent
            sc = np.sqrt(np.add.reduce(x1 * x1, axis=1, keepdims=True) / F(nz) + F(1e-9))
            lo, hi = R.scale_interval(s.latent, got["latent"])
            assert bool(((lo <= sc) & (sc <= hi)).all())
            assert nz < 100 or float(((hi - lo) / sc).max()) < 2.0 ** -23
        # alpha: the same table, flat, with the p = 0 half
        inp = R.Inputs(B * nz, 7 + k, R.HP(0.0, B1T, B2T, EPST, 1.0, 1.0), with_m=True)
        row = sched[min(k, NUM_STEP)]
        ra = R.alpha_ref(inp.p, inp.g, inp.m, inp.v, row, B1T, B2T, EPST)
        R.assert_normal(ra)
        x1, m1, v1 = table_f32(inp.p, inp.g, inp.m, inp.v, row)
        q = R.check(f"alpha restatement k={k}", {"p": x1, "m": m1, "v": v1}, ra, R.bounds(ra, R.A_TABLE, 0), inp.cls)
        assert max(q.values()) <= 1.0
    assert float(sched[0][0]) == 0.0 and float(sched[NUM_STEP][0]) == 0.0   # lambda(0) = lambda(num_step) = 0: no step there


def test_bf16_rounding_and_ulp():
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-39 * 0 + 2.0 ** -126, 65280.0, 1.0 + 2.0 ** -8 + 2.0 ** -20], F)
    want = torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.bf16_rne_bits(x), want)
    rng = np.random.default_rng(0)
    y = (rng.standard_normal(100000) * 10.0 ** rng.uniform(-20, 20, 100000)).astype(F)
    assert np.array_equal(R.bf16_rne_bits(y), torch.from_numpy(y).bfloat16().view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(R.bf16_value(R.bf16_rne_bits(y)), torch.from_numpy(y).bfloat16().float().numpy())
    assert np.array_equal(R.u(y), np.abs(np.spacing(y)).astype(np.float64)) and R.u(0.0) == 0.0


# ---- (b) every wrong variant fails a criterion; which of them today's thresholds let through -------------------------------------
VARIANTS = ["eps dropped", "eps inside the square root", "eps before the bias correction", "t + 1", "t - 1", "no bc2",
            "v' from the unscaled gradient", "ema from the old p", "d and 1 - d swapped", "lane 3 reads lane 2's v"]


class _Today:
    """the inputs of tests/test_gpu_ops.py::test_losses_fetch_reals_adam"""

    def __init__(self):
        g = torch.Generator().manual_seed(1)
        p, gr, m, v, ema = (torch.randn(1000, generator=g) for _ in range(5))
        self.p, self.g, self.v, self.ema = p.numpy(), gr.numpy(), v.abs().numpy(), ema.numpy()
        self.m, self.cls, self.n = np.zeros(1000, F), np.full(1000, 4), 1000


def _passes_todays_thresholds(variant):
    """rel-L2 of p, v, ema against the float64 reference at step 3, all < 1e-6 (the thresholds of that test)"""
    hp, inp = R.HP(), _Today()
    r = R.adam_ref(inp.p, inp.g, None, inp.v, inp.ema, 3, hp)
    got = adam_f32(inp, 3, hp, False, variant, has_m=False)
    rl = {k: rel_l2(torch.from_numpy(got[k]), torch.from_numpy(r[k])) for k in ("p", "v", "ema")}
    return all(x < 1e-6 for x in rl.values()), rl


def test_every_wrong_variant_fails_a_criterion_and_three_pass_todays_thresholds(capsys):
    lines, passed_today = [], []
    ok, rl = _passes_todays_thresholds(None)
    assert ok, rl                                    # the right formula passes today's test, of course
    for variant in VARIANTS:
        caught = set()
        for dev in (False, True):
            for t in (2, 4, 100):
                hp = R.HP()
                inp = R.Inputs(2800, 11 + t, hp, with_m=True)
                fac = {} if dev else dict(zip(("lr_bc1", "isb"), hp.host_factors(t)))
                r = R.adam_ref(inp.p, inp.g, None, inp.v, inp.ema, t, hp, **fac)
                q = R.check(variant, adam_f32(inp, t, hp, dev, variant, has_m=False), r,
                            R.bounds(r, R.A_DEV if dev else R.A_HOST, R.POW_ULPS if dev else 0), inp.cls, fail=False)
                names = {k for k, x in q.items() if k != "failures" and x > 1.0}
                assert names, f"the wrong variant '{variant}' passes every criterion ({'dev' if dev else 'host'}, t = {t})"
                assert q["failures"] and "by class" in q["failures"][0] and "by index % 4" in q["failures"][0]
                caught |= names
        today, rl = _passes_todays_thresholds(variant)
        if today:
            passed_today.append(variant)
        lines.append(f"{variant:34s} caught by {sorted(caught)}; today's rel-L2 thresholds "
                     f"{'LET IT THROUGH' if today else 'catch it'} (rel-L2 of p = {rl['p']:.2g})")
    # beta1 > 0: the bias correction of the first moment ignored
    hp = R.HP(b1=0.9)
    inp = R.Inputs(2800, 5, hp, with_m=True)
    r = R.adam_ref(inp.p, inp.g, inp.m, inp.v, inp.ema, 4, hp)
    q = R.check("bc1 ignored", adam_f32(inp, 4, hp, True, "bc1 ignored"), r, R.bounds(r, R.A_DEV, R.POW_ULPS), inp.cls, fail=False)
    assert q["delta"] > 1.0 and q["p'"] > 1.0
    lines.append(f"{'bc1 ignored at beta1 = 0.9':34s} caught by {sorted(k for k, x in q.items() if k != 'failures' and x > 1.0)}; "
                 "no test runs beta1 > 0 today")
    # the lane variant shows as one bar of the lane histogram
    hp = R.HP()
    inp = R.Inputs(2800, 13, hp)
    r = R.adam_ref(inp.p, inp.g, None, inp.v, inp.ema, 4, hp)
    q = R.check("lane", adam_f32(inp, 4, hp, True, "lane 3 reads lane 2's v", has_m=False), r, R.bounds(r, R.A_DEV, R.POW_ULPS),
                inp.cls, fail=False)
    assert "by index % 4: 3:" in q["failures"][0]
    # the shadow truncated where it should be rounded
    p1 = adam_f32(inp, 4, hp, True, has_m=False)["p"]
    R.check_shadow("rounded", R.bf16_rne_bits(p1), p1, True)
    R.check_shadow("fp32", p1.view(np.uint32), p1, False)
    with pytest.raises(AssertionError, match="shadow differs"):
        R.check_shadow("truncated", (p1.view(np.uint32) >> 16).astype(np.uint16), p1, True)
    lines.append(f"{'shadow truncated':34s} caught by the bit comparison with the rounded master (today's test compares bits too)")
    # renormalisation without the 1e-9: only a row of small RMS shows it - the rows of RMS 1e-3, at k = 0 (no step)
    sched = sched_table()
    s = R.sphere_inputs(3, 257, 9)
    r = R.sphere_ref(s.latent, s.g, s.m, s.v, sched, 0, NUM_STEP, B1T, B2T, EPST)
    q = R.check_sphere("renorm", sphere_f32(s, sched, 0, "renormalisation without the 1e-9"), r, R.sphere_bounds(r), s.cls, fail=False)
    assert q["row"] > 1.0 and q["scale"] > 1.0 and q["v'"] <= 1.0 and any("row scale outside" in f for f in q["failures"])
    lines.append(f"{'renormalisation without the 1e-9':34s} caught by ['row', 'scale'] on the rows of RMS 1e-3; only whole inversions run it today")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert set(passed_today) >= {"eps dropped", "eps inside the square root", "eps before the bias correction"}, passed_today


def test_rho_is_what_the_docstring_says():
    hp = R.HP()
    assert 9e-5 < R.rho(1, hp, R.A_DEV, R.POW_ULPS) < 1e-4
    assert R.rho(1000, hp, R.A_DEV, R.POW_ULPS) < 7e-7 and R.rho(70, hp, R.A_DEV, R.POW_ULPS) < 2e-6
    assert R.rho(5, hp, R.A_HOST, 0) == 8 * 2.0 ** -24
    # the ABI's floats, not the decimal literals
    assert hp.b2 == float(np.float32(0.99)) != 0.99
