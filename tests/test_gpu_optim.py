"""Every Adam kernel, per element, against the float64 reference and the criteria of tests/optim_ref.py (derived there, proved on
the CPU by tests/test_optim_ref_cpu.py), through the C ABI: adam_ema_kernel (host step and device step), adam_fused_kernel (three
piece kinds), adam_proj_fused_kernel, the Adam epilogue of wgrad_mfma_kernel, sphere_adam_kernel, alpha_adam_kernel.

Inputs are the seven classes of optim_ref.Inputs on every lane of a float4 and in every piece kind; every input and intermediate is
a normal fp32 number or zero (the project promises nothing about denormals; R.assert_normal holds each case to it).  Each test
prints the largest |err| / bound it saw per kernel and step count (run with -s); a ratio above 1 fails.

Measured on an MI355X, largest |err| / bound over every case of this file (sphere_adam / alpha_adam: t = step index + 1; `row` the
renormalised latent, `scale` the row scale read back where the step size is zero; the fused kernels' stored gradient: 0.37 of
its bound at most):
    kernel                            t      v'      m'   delta      p'    ema'     row   scale
    adam_ema (device step)            1   0.324   0.545   0.144   0.997   0.546       -       -
    adam_ema (device step)            2   0.438   0.749   0.286   1.000   0.574       -       -
    adam_ema (device step)            3   0.334   0.658   0.206   0.986   0.552       -       -
    adam_ema (device step)            4   0.434   0.745   0.224   1.000   0.784       -       -
    adam_ema (device step)            5   0.237   0.635   0.026   0.953   0.526       -       -
    adam_ema (device step)            6   0.249   0.656   0.039   0.989   0.591       -       -
    adam_ema (device step)           70   0.327   0.717   0.309   0.974   0.549       -       -
    adam_ema (device step)         1000   0.330   0.642   0.305   0.986   0.572       -       -
    adam_ema (device step)      1000000   0.302   0.514   0.305   0.992   0.569       -       -
    adam_ema (host step)              1   0.304   0.545   0.331   0.998   0.546       -       -
    adam_ema (host step)              2   0.307   0.728   0.346   0.998   0.695       -       -
    adam_ema (host step)              4   0.329   0.655   0.313   0.992   0.628       -       -
    adam_ema (host step)            100   0.302   0.514   0.311   0.994   0.674       -       -
    adam_ema (host step)        1000000   0.302   0.514   0.311   0.992   0.570       -       -
    adam_fused                        1   0.410       -   0.002   0.995   0.619       -       -
    adam_fused                        4   0.414       -   0.021   0.998   0.593       -       -
    adam_fused                      100   0.404       -   0.162   0.999   0.586       -       -
    adam_proj_fused (VALU)            1   0.232       -   0.004   0.995   0.745       -       -
    adam_proj_fused (VALU)            4   0.232       -   0.019   0.997   0.728       -       -
    adam_proj_fused (VALU)          100   0.232       -   0.146   0.994   0.740       -       -
    alpha_adam                        1   0.289   0.391   0.000   0.000       -       -       -
    alpha_adam                        2   0.331   0.396   0.352   1.000       -       -       -
    alpha_adam                        6   0.313   0.394   0.339   0.998       -       -       -
    alpha_adam                       21   0.319   0.397   0.000   0.000       -       -       -
    alpha_adam                       24   0.327   0.400   0.000   0.000       -       -       -
    sphere_adam                       1   0.326   0.400       -       -       -   0.249   0.203
    sphere_adam                       2   0.326   0.400       -       -       -   0.290       -
    sphere_adam                       6   0.326   0.400       -       -       -   0.285       -
    sphere_adam                      21   0.326   0.400       -       -       -   0.249   0.203
    sphere_adam                      24   0.326   0.400       -       -       -   0.249   0.203
    wgrad_mfma Adam epilogue          1   0.232       -   0.044   0.997   0.727       -       -
    wgrad_mfma Adam epilogue          4   0.232       -   0.058   0.993   0.718       -       -
    wgrad_mfma Adam epilogue        100   0.344       -   0.152   1.000   0.740       -       -
p' and ema' come close to 1 by construction: where |delta| is below half an ulp of p the right answer is p itself, half an ulp
from the float64 value.  delta, the quantity that holds the formula, stays below 0.36 of its bound everywhere."""
import numpy as np
import pytest
import torch

from tests import optim_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = np.float32
GUARD = 64                                           # elements behind every buffer that no kernel may touch
SENT = 12288.0                                       # (a bf16 number)


@pytest.fixture(scope="module")
def L():
    from dusty_gan_amd import _lib
    _lib.lib()
    return _lib


def dev(a, guard=True):
    """a float32 array on the device with GUARD sentinel elements behind it"""
    a = np.ascontiguousarray(a, dtype=F).reshape(-1)
    t = torch.full((a.size + (GUARD if guard else 0),), SENT, dtype=torch.float32)
    t[:a.size] = torch.from_numpy(a)
    return t.to(DEV)


def host(t, n):
    """the first n elements as numpy, the guard behind them checked"""
    a = t.detach().cpu()
    if a.numel() > n:
        tail = a[n:].float()
        assert bool((tail == SENT).all()), "a kernel wrote behind its buffer"
    return a[:n].numpy()


def shadow_buf(n, kind):
    if kind is None:
        return None
    return torch.full((n + GUARD,), SENT, dtype=torch.bfloat16 if kind == "bf16" else torch.float32, device=DEV)


def shadow_bits(sh, n, kind):
    a = sh.detach().cpu()
    assert bool((a[n:].float() == SENT).all()), "a kernel wrote behind the shadow"
    return a[:n].view(torch.int16).numpy().view(np.uint16) if kind == "bf16" else a[:n].numpy().view(np.uint32)


def ptr(t):
    return None if t is None else t.data_ptr()


def counter(k):
    return torch.tensor([k], dtype=torch.int64, device=DEV)


# ---- adam_ema_kernel ----------------------------------------------------------------------------------------------------------------
def run_plain(L, inp, hp, t, on_dev, has_m, has_ema, sh_kind, state=None, step=None):
    """one launch of dg_adam_ema_step (host step t) or dg_adam_ema_step_dev (device counter t - 1) on the inputs (or on `state`,
    device buffers of an earlier launch); checks every criterion, returns the ratios and the device state"""
    lib, n = L.lib(), inp.n
    if state is None:
        state = dict(p=dev(inp.p), v=dev(inp.v), m=dev(inp.m) if has_m else None, ema=dev(inp.ema) if has_ema else None)
    before = {k: (None if b is None else host(b, n).copy()) for k, b in state.items()}
    gd, sh = dev(inp.g), shadow_buf(n, sh_kind)
    code = L.DG_BF16 if sh_kind == "bf16" else L.DG_F32
    if on_dev:
        step = counter(t - 1) if step is None else step
        L.check(lib.dg_adam_ema_step_dev(ptr(state["p"]), ptr(gd), ptr(state["m"]), ptr(state["v"]), ptr(state["ema"]), ptr(sh), code,
                                         n, hp.gscale, hp.lr, hp.b1, hp.b2, hp.eps, ptr(step), hp.d, None), "dg_adam_ema_step_dev")
        fac, A, P, name = {}, R.A_DEV, R.POW_ULPS, "adam_ema (device step)"
    else:
        L.check(lib.dg_adam_ema_step(ptr(state["p"]), ptr(gd), ptr(state["m"]), ptr(state["v"]), ptr(state["ema"]), ptr(sh), code, n,
                                     hp.gscale, hp.lr, hp.b1, hp.b2, hp.eps, t, hp.d, None), "dg_adam_ema_step")
        fac, A, P, name = dict(zip(("lr_bc1", "isb"), hp.host_factors(t))), R.A_HOST, 0, "adam_ema (host step)"
    torch.cuda.synchronize()
    if on_dev:
        assert int(step) == t - 1, "the kernel wrote the step counter"
    got = {k: (None if b is None else host(b, n)) for k, b in state.items()}
    assert np.array_equal(host(gd, n).view(np.uint32), inp.g.view(np.uint32)), "the gradient was written"
    r = R.adam_ref(before["p"], inp.g, before["m"], before["v"], before["ema"], t, hp, **fac)
    R.assert_normal(r)
    what = f"{name} n={n} t={t} b1={hp.b1:.2g} m={has_m} ema={has_ema} shadow={sh_kind}"
    q = R.check(what, got, r, R.bounds(r, A, P), inp.cls)
    now = R.Ref(cls=inp.cls, p=before["p"], m=before["m"], ema=before["ema"])
    R.check_class_facts(what, got, now, hp, has_ema)
    if sh is not None:
        R.check_shadow(what, shadow_bits(sh, n, sh_kind), got["p"], sh_kind == "bf16")
    R.note(name, t, q)
    return q, state


def plain_grid(b1s=(0.0, 0.5, 0.9)):
    """(b1, has_m, has_ema, shadow kind): m passed and NULL at beta1 = 0, ema present and absent, shadow bf16 / fp32 / absent"""
    out = []
    for b1 in b1s:
        for has_m in ((True, False) if b1 == 0 else (True,)):
            for has_ema in (True, False):
                for sk in ("bf16", "fp32", None):
                    out.append((b1, has_m, has_ema, sk))
    return out


BIG = 4 * (256 * 4096 + 37)   # the grid is capped at 4096 workgroups of 256 float4: the smallest n with a second, partial pass


@pytest.mark.parametrize("on_dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("n", [64, 1028])
def test_adam_ema_step_every_class_every_step(L, n, on_dev):
    steps = (1, 2, 3, 4, 70, 1000, 10 ** 6) if on_dev else (1, 2, 4, 100, 10 ** 6)
    for t in steps:
        for b1, has_m, has_ema, sk in plain_grid():
            hp = R.HP(b1=b1, d=1.0 if (t == 2 and sk is None) else 0.9)
            inp = R.Inputs(n, 1000 + t % 101 + n, hp, with_m=True)
            run_plain(L, inp, hp, t, on_dev, has_m, has_ema, sk)
    print("\n" + R.format_ratios("adam_ema (device step)" if on_dev else "adam_ema (host step)"))


@pytest.mark.parametrize("on_dev", [False, True], ids=["host", "dev"])
def test_adam_ema_step_grid_stride_second_pass(L, on_dev):
    """n = 4 (256 * 4096 + 37): every workgroup of the capped grid makes a first pass, 37 lanes a second one"""
    for t, b1, has_m, has_ema, sk in ((4, 0.0, False, True, "bf16"), (2, 0.9, True, False, "fp32")):
        hp = R.HP(b1=b1)
        run_plain(L, R.Inputs(BIG, 5 + t, hp, with_m=True), hp, t, on_dev, has_m, has_ema, sk)


def test_adam_ema_step_refuses_a_length_off_the_float4_grid(L):
    lib, hp = L.lib(), R.HP()
    inp = R.Inputs(1028, 3, hp)
    pd, gd, vd, st = dev(inp.p), dev(inp.g), dev(inp.v), counter(0)
    assert lib.dg_adam_ema_step(ptr(pd), ptr(gd), None, ptr(vd), None, None, L.DG_F32, 1027, hp.gscale, hp.lr, 0.0, hp.b2, hp.eps, 1,
                                hp.d, None) == L.DG_EINVAL
    assert lib.dg_adam_ema_step_dev(ptr(pd), ptr(gd), None, ptr(vd), None, None, L.DG_F32, 1027, hp.gscale, hp.lr, 0.0, hp.b2, hp.eps,
                                    ptr(st), hp.d, None) == L.DG_EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(host(pd, 1028), inp.p) and np.array_equal(host(vd, 1028), inp.v)


@pytest.mark.parametrize("b1", [0.0, 0.9])
def test_adam_ema_step_dev_sequence_of_six_steps(L, b1):
    """six launches on one state, the counter advanced by dg_counter_add between them, a fresh gradient every step; each step is
    checked against adam_ref started from the state the GPU left the step before: every t from 1 to 6 per element, no pile-up"""
    lib, hp, n = L.lib(), R.HP(b1=b1), 1028
    first = R.Inputs(n, 40, hp, with_m=b1 > 0)
    if b1 > 0:
        first.m = np.zeros(n, F)                     # a first step: no moments yet
    first.v = np.zeros(n, F)
    step, state = counter(0), None
    for t in range(1, 7):
        inp = R.Inputs(n, 40 + t, hp)
        inp.p, inp.v, inp.m, inp.ema = first.p, first.v, first.m, first.ema
        _, state = run_plain(L, inp, hp, t, True, b1 > 0, True, "bf16", state=state, step=step)
        L.check(lib.dg_counter_add(ptr(step), 1, None), "dg_counter_add")
        torch.cuda.synchronize()
        assert int(step) == t
        # p and ema go back to zero on their p = 0 half (the moments stay as the GPU left them): delta itself is read at every t
        zero = torch.from_numpy(first.p == 0).to(DEV)
        state["p"][:n][zero] = 0.0
        state["ema"][:n][zero] = 0.0
    print("\n" + R.format_ratios("adam_ema (device step)"))


# ---- adam_fused_kernel --------------------------------------------------------------------------------------------------------------
def seg(numel, splits=0, acc=0, ws_n=0, ws_bf16=0, ws_coef=True, kind=0, ci=0, co=0):
    return dict(numel=numel, splits=splits, acc=acc, ws_n=ws_n, ws_bf16=ws_bf16, ws_coef=ws_coef, kind=kind, ci=ci, co=co)


def to_bf16_values(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F)).bfloat16().float().numpy()


def run_fused(L, specs, hp, t, has_ema, sh_kind, seed, what):
    """one launch of dg_adam_fused over `specs`: the stored gradient against the float64 sum of the terms as stored, to
    (rows + 2) 2^-24 sum |terms|; Adam from the gradient the kernel stored (it is the value the kernel's update consumed, so the
    criteria are the plain kernel's); shadow and transposed shadow from the kernel's own master"""
    lib = L.lib()
    off = 0
    for s in specs:
        s["off"], off = off, off + s["numel"]
    n = off
    inp = R.Inputs(n, seed, hp)
    rng = np.random.default_rng(seed + 1)
    grad0 = np.full(n, 7.0, F)                       # (accumulate = 0: never read, overwritten)
    want_g, bound_g, seg_id = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64)
    keep, ws_scale = [], 0.25
    segs = (L.DgOptSeg * len(specs))()
    for i, s in enumerate(specs):
        sl = slice(s["off"], s["off"] + s["numel"])
        tgt = inp.g[sl].astype(np.float64)
        seg_id[sl] = i
        T = s["splits"] + s["acc"] + s["ws_n"]
        w = rng.uniform(0.5, 1.5, max(T, 1)) / max(T, 1)   # positive shares of the class value: the sum keeps the class
        parts = g0 = src = coef = None
        j = s["splits"]
        if s["splits"]:
            parts = (tgt[None] * w[:j, None]).astype(F)
        if s["acc"]:
            g0 = (tgt * w[j]).astype(F)
            grad0[sl] = g0
            j += 1
        if s["ws_n"]:
            coef = rng.uniform(0.5, 2.0, s["ws_n"]).astype(F) if s["ws_coef"] else None
            src = (tgt[None] * w[j:, None] / (ws_scale * (coef[:, None].astype(np.float64) if coef is not None else 1.0))).astype(F)
            if s["ws_bf16"]:
                src = to_bf16_values(src)
        if T:
            want_g[sl], bound_g[sl] = R.fused_grad_ref(parts, g0, src, coef, ws_scale)
        q = segs[i]
        q.off, q.numel, q.splits, q.accumulate, q.kind, q.ci, q.co = s["off"], s["numel"], s["splits"], s["acc"], s["kind"], s["ci"], s["co"]
        if parts is not None:
            pd = torch.from_numpy(parts).to(DEV)
            keep.append(pd)
            q.part = pd.data_ptr()
        if src is not None:
            stride = s["numel"] + 8                  # (rows apart by more than numel; what lies between is NaN: never read)
            buf = np.full((s["ws_n"], stride), np.nan, F)
            buf[:, :s["numel"]] = src
            sd = torch.from_numpy(buf).to(DEV)
            sd = sd.bfloat16() if s["ws_bf16"] else sd
            keep.append(sd)
            q.ws_src, q.ws_stride, q.ws_n, q.ws_bf16, q.ws_scale = sd.data_ptr(), stride, s["ws_n"], s["ws_bf16"], ws_scale
            if coef is not None:
                cd = torch.from_numpy(coef).to(DEV)
                keep.append(cd)
                q.ws_coef = cd.data_ptr()
        if s["kind"] == 1:
            s["st"] = shadow_buf(s["numel"], sh_kind)
            q.shadow_t = s["st"].data_ptr()
    pd_, gd, vd, ed = dev(inp.p), dev(grad0), dev(inp.v), dev(inp.ema) if has_ema else None
    sh, step = shadow_buf(n, sh_kind), counter(t - 1)
    L.check(lib.dg_adam_fused(ptr(pd_), ptr(gd), ptr(vd), ptr(ed), ptr(sh), L.DG_BF16 if sh_kind == "bf16" else L.DG_F32, segs,
                              len(specs), hp.gscale, hp.lr, hp.b2, hp.eps, ptr(step), hp.d, None), "dg_adam_fused")
    torch.cuda.synchronize()
    assert int(step) == t - 1
    got = dict(p=host(pd_, n), v=host(vd, n), ema=host(ed, n) if has_ema else None)
    g_gpu = host(gd, n)
    what = f"adam_fused {what} t={t} ema={has_ema} shadow={sh_kind}"
    bad, qg = R.ratio_of(g_gpu, want_g, bound_g)
    if bad.any():
        raise AssertionError(R.failure_report(f"{what}: stored gradient", bad, g_gpu, want_g, bound_g, inp.cls, seg_id))
    r = R.adam_ref(inp.p, g_gpu, None, inp.v, inp.ema if has_ema else None, t, hp)
    R.assert_normal(r)
    q = R.check(what, got, r, R.bounds(r, R.A_DEV, R.POW_ULPS), inp.cls, seg_id)
    R.check_class_facts(what, got, inp, hp, has_ema)
    R.check_shadow(what, shadow_bits(sh, n, sh_kind), got["p"], sh_kind == "bf16")
    for s in specs:
        if s["kind"] == 1:   # [16][co][ci]: the transposed rounded master
            pt = got["p"][s["off"]:s["off"] + s["numel"]].reshape(16, s["ci"], s["co"]).transpose(0, 2, 1)
            R.check_shadow(what + " transposed", shadow_bits(s["st"], s["numel"], sh_kind), np.ascontiguousarray(pt), sh_kind == "bf16")
    q["grad"] = qg
    R.note("adam_fused", t, {k: x for k, x in q.items() if k != "grad"})
    return q


FUSED_CASES = {
    # kind 0: the 8-wide unroll boundary of part_sum (7, 8, 9), its end (64), no rows at all, with and without the buffer's content
    "kind0-splits": lambda: [seg((1028, 96, 2052, 1024, 64, 260)[i % 6], sp, acc) for i, (sp, acc) in
                             enumerate((sp, acc) for sp in (0, 1, 7, 8, 9, 64) for acc in (0, 1))],
    # kind 0 with the batch term: bf16 and fp32 sources, 1 / 8 / 9 rows (the 8-wide groups), coefficients given and absent
    "kind0-ws": lambda: [seg((1028, 512, 96)[i % 3], (0, 3)[i % 2], (i // 2) % 2, ws_n, bf, cf) for i, (bf, ws_n, cf) in
                         enumerate((bf, ws_n, cf) for bf in (1, 0) for ws_n in (1, 8, 9) for cf in (True, False))],
    # kind 2 (more than 64 rows): 96 elements = one full workgroup of 16 float4 and a half-filled one
    "kind2": lambda: [seg(96, sp, acc) for sp in (65, 129) for acc in (0, 1)],
    # kind 1: the conv tile walk, co = 64 (16 x 64 tiles) and multiples of 128 (8 x 128 tiles)
    "kind1": lambda: [seg(16 * 16 * 64, 5, 1, kind=1, ci=16, co=64), seg(16 * 48 * 128, 0, 1, kind=1, ci=48, co=128),
                      seg(16 * 32 * 256, 9, 0, kind=1, ci=32, co=256)],
    # as many segments as a launch takes, the row counts in no order: the block-to-segment search sees every boundary
    "max-seg": lambda: [seg(16 * 16 * 64, 3, 0, kind=1, ci=16, co=64) if i in (4, 13) else
                        seg((4, 1028, 96, 2052, 64, 1024, 8)[i % 7], (9, 0, 129, 1, 64, 7, 65, 8, 2)[i % 9], i % 2,
                            ws_n=(0, 0, 9)[i % 3] if (9, 0, 129, 1, 64, 7, 65, 8, 2)[i % 9] <= 64 else 0, ws_bf16=i % 2)
                        for i in range(20)],
}


@pytest.mark.parametrize("case", list(FUSED_CASES))
def test_adam_fused_every_class_in_every_segment(L, case):
    assert L.OPT_MAX_SEG == 20
    worst = {}
    for t in (1, 4, 100):
        for has_ema, sk in ((True, "bf16"), (False, "fp32"), (True, "fp32"), (False, "bf16")):
            hp = R.HP(d=1.0 if (t == 4 and sk == "fp32") else 0.998)
            q = run_fused(L, FUSED_CASES[case](), hp, t, has_ema, sk, 300 + t, case)
            worst["grad"] = max(worst.get("grad", 0.0), q["grad"])
    print(f"\nadam_fused {case}: stored gradient, largest |err| / bound = {worst['grad']:.3f}\n" + R.format_ratios("adam_fused"))


# ---- dg_adam_proj_fused: the VALU kernel and the MFMA epilogue ----------------------------------------------------------------------
WSCALE = 0.125                                       # a power of two: acc * wscale * gscale is exact


def proj_case(nb, Np, K, mode, seed, hp):
    """Operands that put a class on every row of Proj.weight: dp0[:, row] = small integers times 2^s(row) (zero for padding and
    idle), z small integers - every product and every partial sum is then an integer times a power of two below 2^24 and the
    gradient is EXACT in any order (bound 0); the ordinary rows take random dp0 of the operand type's precision (fp32x3: 16
    mantissa bits, hi + lo; z's low half is zero, so no lo x lo product exists) and carry the dot product's bound."""
    rng = np.random.default_rng(seed)
    rows = np.arange(Np)
    c, j = rows % 7, rows // 7
    s = np.select([c == 2, c == 3, c == 4, c == 5, c == 6], [-30 + j % 10, -10 + j % 21, 0 * j, -10 + 0 * j, 17 + 0 * j], 0 * j)
    dp0 = rng.integers(-3, 4, (nb, Np)).astype(np.float64) * 2.0 ** s[None, :]
    dp0[:, c <= 1] = 0.0
    rnd = (rng.standard_normal((nb, Np)) * 0.125).astype(F)
    if mode == "bf16":
        rnd = to_bf16_values(rnd)
    elif mode == "x3":
        hi = to_bf16_values(rnd)
        rnd = hi + to_bf16_values(rnd - hi)
    dp0 = np.where((c == 4)[None, :], rnd.astype(np.float64), dp0).astype(F)
    z = rng.integers(-2, 3, (nb, K)).astype(F)
    cls = np.broadcast_to(c[:, None], (Np, K)).reshape(-1)
    zero_half = ((j[:, None] + np.arange(K)[None, :] // 4) % 2 == 0).reshape(-1)
    inp = R.Inputs(Np * K, seed + 1, hp, cls=cls, zero_half=zero_half)
    g, gerr = R.proj_grad_ref(dp0, z, WSCALE)
    gerr = np.where((c == 4)[:, None], gerr, 0.0)
    inp.g = g.reshape(-1)                            # (float64: exact where the class needs it)
    return inp, dp0, z, gerr.reshape(-1)


def run_proj(L, nb, Np, K, mode, name):
    lib = L.lib()
    for t in (1, 4, 100):
        for has_ema, sk in ((True, "bf16"), (False, "fp32"), (True, None)):
            hp = R.HP(d=1.0 if (t == 4 and sk is None) else 0.9)
            inp, dp0, z, gerr = proj_case(nb, Np, K, mode, 500 + t + nb, hp)
            n = Np * K
            pd, vd, ed, sh, step = dev(inp.p), dev(inp.v), dev(inp.ema) if has_ema else None, shadow_buf(n, sk), counter(t - 1)
            dt = torch.bfloat16 if mode == "bf16" else torch.float32
            dpd, zd = torch.from_numpy(dp0).to(DEV, dt).contiguous(), torch.from_numpy(z).to(DEV, dt).contiguous()
            op = L.DG_BF16 if mode == "bf16" else (L.DG_F32 | (L.DG_FORCE_FP32X3 if mode == "x3" else 0))
            L.check(lib.dg_adam_proj_fused(ptr(pd), ptr(vd), ptr(ed), ptr(sh), L.DG_BF16 if sk == "bf16" else L.DG_F32, ptr(dpd), ptr(zd),
                                           op, nb, Np, K, WSCALE, hp.gscale, hp.lr, hp.b2, hp.eps, ptr(step), hp.d, None),
                    "dg_adam_proj_fused")
            torch.cuda.synchronize()
            assert int(step) == t - 1
            got = dict(p=host(pd, n), v=host(vd, n), ema=host(ed, n) if has_ema else None)
            r = R.adam_ref(inp.p, inp.g, None, inp.v, inp.ema if has_ema else None, t, hp)
            R.assert_normal(r)
            what = f"{name} ({nb},{Np},{K}) {mode} t={t} ema={has_ema} shadow={sk}"
            q = R.check(what, got, r, R.bounds(r, R.A_DEV, R.POW_ULPS, gerr=gerr), inp.cls)
            R.check_class_facts(what, got, inp, hp, has_ema)
            if sh is not None:
                R.check_shadow(what, shadow_bits(sh, n, sk), got["p"], sk == "bf16")
            R.note(name, t, q)
    print("\n" + R.format_ratios(name))


@pytest.mark.parametrize("nb,Np,K", [(2, 70, 4), (4, 200, 8), (64, 130, 256), (32, 1000, 512)])
def test_adam_proj_fused_valu_kernel(L, nb, Np, K):
    """Np or K off the 128 grid: the LDS/VALU kernel - a row tail in the last workgroup, K / 4 from 1 to 128"""
    run_proj(L, nb, Np, K, "bf16", "adam_proj_fused (VALU)")


@pytest.mark.parametrize("mode", ["bf16", "fp32", "x3"])
@pytest.mark.parametrize("nb,Np,K", [(2, 128, 128), (3, 256, 128), (17, 384, 256), (100, 128, 256)])
def test_adam_proj_fused_mfma_epilogue(L, nb, Np, K, mode):
    """Np and K multiples of 128: the Adam epilogue of wgrad_mfma_kernel, bf16 / fp32 / fp32x3 operands"""
    run_proj(L, nb, Np, K, mode, "wgrad_mfma Adam epilogue")


# ---- sphere_adam_kernel, alpha_adam_kernel ------------------------------------------------------------------------------------------
NUM_STEP = 20
B1T, B2T, EPST = 0.9, 0.999, 1e-8
STEP_INDICES = (0, 1, 5, NUM_STEP, NUM_STEP + 3)


@pytest.fixture(scope="module")
def sched():
    from dusty_gan_amd.inversion import adam_table
    return adam_table(0.1, NUM_STEP, 0.05, 0.25)


@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("nz", [1, 100, 256, 257, 1024])
def test_sphere_adam(L, sched, nz, B):
    lib = L.lib()
    sc_np, sc_d = sched.numpy(), sched.to(DEV)
    s = R.sphere_inputs(B, nz, 900 + nz + B)
    noise = (np.random.default_rng(nz).standard_normal((B, nz)) * 0.05).astype(F)
    Bp = B + 3
    for i, k in enumerate(STEP_INDICES):
        engine_strides, perturb, z_bf16 = (i + nz) % 2 == 0, i % 2 == 1, (i // 2 + B) % 2 == 0
        if engine_strides:                           # [nz][Bp], Bp > B: grad(b, j) = grad[b + j Bp]
            gbuf = np.full((nz, Bp), np.nan, F)
            gbuf[:, :B] = s.g.T
            g_sb, g_sk = 1, Bp
        else:
            gbuf, g_sb, g_sk = s.g, nz, 1
        gd, ld, md, vd = dev(gbuf), dev(s.latent), dev(s.m), dev(s.v)
        nd = torch.from_numpy(noise).to(DEV) if perturb else None
        zT = shadow_buf(B * nz, "bf16" if z_bf16 else "fp32")
        step, ticket = counter(k), torch.zeros(1, dtype=torch.int32, device=DEV)
        args = (ptr(gd), g_sb, g_sk, ptr(ld), ptr(md), ptr(vd), ptr(step), ptr(ticket), ptr(nd), ptr(zT),
                L.DG_BF16 if z_bf16 else L.DG_F32, B, nz, ptr(sc_d), NUM_STEP, B1T, B2T, EPST, int(perturb), 1, 2)
        L.check(lib.dg_sphere_adam(*args, 0, None), "dg_sphere_adam")
        torch.cuda.synchronize()
        assert int(step) == k + 1 and int(ticket) == 0
        n = B * nz
        got = dict(latent=host(ld, n).reshape(B, nz), m=host(md, n).reshape(B, nz), v=host(vd, n).reshape(B, nz))
        r = R.sphere_ref(s.latent, s.g, s.m, s.v, sc_np, k, NUM_STEP, B1T, B2T, EPST)
        R.assert_normal(r)
        what = f"sphere_adam nz={nz} B={B} k={k} strides={'(1,Bp)' if engine_strides else '(nz,1)'}"
        q = R.check_sphere(what, got, r, R.sphere_bounds(r), s.cls)
        R.note("sphere_adam", k + 1, q)
        # zT: the stored latent plus the injected noise, rounded once (fp32), the RNE bf16 of that
        z32 = (got["latent"] + noise) if perturb else got["latent"]
        assert z32.dtype == np.float32
        R.check_shadow(what + " zT", shadow_bits(zT, n, "bf16" if z_bf16 else "fp32"), z32, z_bf16)
        # prime = 1: only zT is written
        before = [host(t_, n).copy() for t_ in (ld, md, vd)]
        zT2 = shadow_buf(n, "bf16" if z_bf16 else "fp32")
        args2 = args[:9] + (ptr(zT2),) + args[10:]
        L.check(lib.dg_sphere_adam(*args2, 1, None), "dg_sphere_adam prime")
        torch.cuda.synchronize()
        assert int(step) == k + 1 and int(ticket) == 0
        for a, t_ in zip(before, (ld, md, vd)):
            assert np.array_equal(a.view(np.uint32), host(t_, n).view(np.uint32)), "prime = 1 wrote the optimizer state"
        R.check_shadow(what + " zT (prime)", shadow_bits(zT2, n, "bf16" if z_bf16 else "fp32"), z32, z_bf16)
    print("\n" + R.format_ratios("sphere_adam"))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 7680])
def test_alpha_adam(L, sched, n):
    lib = L.lib()
    sc_np, sc_d = sched.numpy(), sched.to(DEV)
    hp = R.HP(0.0, B1T, B2T, EPST, 1.0, 1.0)
    for k in STEP_INDICES:
        inp = R.Inputs(n, 700 + n + k, hp, with_m=True)
        gd, xd, md, vd, step = dev(inp.g), dev(inp.p), dev(inp.m), dev(inp.v), counter(k)
        L.check(lib.dg_alpha_adam(ptr(gd), ptr(xd), ptr(md), ptr(vd), ptr(step), ptr(sc_d), NUM_STEP, B1T, B2T, EPST, n, None),
                "dg_alpha_adam")
        torch.cuda.synchronize()
        assert int(step) == k, "dg_alpha_adam only reads the step index"
        got = dict(p=host(xd, n), m=host(md, n), v=host(vd, n))
        r = R.alpha_ref(inp.p, inp.g, inp.m, inp.v, sc_np[min(k, NUM_STEP)], B1T, B2T, EPST)
        R.assert_normal(r)
        q = R.check(f"alpha_adam n={n} k={k}", got, r, R.bounds(r, R.A_TABLE, 0), inp.cls)
        R.note("alpha_adam", k + 1, q)
    print("\n" + R.format_ratios("alpha_adam"))
