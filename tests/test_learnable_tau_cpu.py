"""What the learnable-temperature tests lean on, shown without a GPU:
 (a) the float64 restatement of tests/learnable_tau_ref.py meets the gradients the REFERENCE recorded for its temperature weights
     (tests/golden/step_dusty{1,2}_ltau.npz, made by tests/golden/make_learnable_tau_golden.py) within the step test's 1e-3 A - and
     with a defect switched on it does not: a missing sigma(w), the image sigmoid used for the pixel sum, l taken without its noise;
 (b) the kernel's arithmetic carried out in float32, on the very inputs the GPU test uses, stays inside the criteria; the inputs keep
     their promise (no mask an fp32 sigmoid could decide either way) at every slope under test; wrong slopes fall outside;
 (c) the modules: `define_G` with tau: null builds, on the CPU, the reference's parameter names, order and shapes over one trailing
     store segment; with a numeric tau nothing moves; what stays refused says so."""
import numpy as np
import pytest
import torch

from oracle import dusty_oracle as O
from tests import learnable_tau_ref as T
from tests import net_end_ref as N
from tests.golden_util import load, step_rand, sub

F = np.float32
CASES = ["dusty1_ltau", "dusty2_ltau"]
TAU_KEYS = {"dusty1": ["gumbel.weight"], "dusty2": ["gumbel_pixel.weight", "gumbel_image.weight"]}
HEAD_B = ("backbone.4.heads.depth.1.module.bias", "backbone.4.heads.confidence.1.module.bias")


def fixture_step(g, it):
    """one recorded G phase as learnable_tau_ref's operands: the upstream d loss_G / d depth through the oracle's DiffAugment and
    the UPDATED discriminator in float64 (trainers/dcgan_amp.py:256-260), everything else as recorded; and the weights of the step"""
    arch = {"dusty1": 1, "dusty2": 2}[str(g["meta/arch"])]
    pre = f"s{it}"
    synth = sub(g, f"{pre}/synth")
    depth = synth["depth"].double().requires_grad_(True)
    D = {k: v.double() for k, v in sub(g, f"{pre}/after/D").items() if not k.endswith("kernel")}
    rp = {k: v.double() if v.is_floating_point() else v for k, v in step_rand(g, it)["aug"][3].items()}
    y = O.discriminator(D, O.diff_augment(depth, rp), bool(g["meta/ring"]))
    assert np.abs(y.detach().numpy() - g[f"{pre}/y_fake2"]).max() <= 1e-4 * max(1.0, np.abs(g[f"{pre}/y_fake2"]).max())
    (go,) = torch.autograd.grad(O.gan_loss(str(g["meta/gan_mode"]), None, y, "G"), depth)
    B = depth.shape[0]
    flat = lambda x: np.ascontiguousarray(x.reshape(B, -1).numpy())
    conf, mk = synth["confidence"], synth["mask"]
    zeros = np.zeros_like(flat(conf[:, 0]))
    inp = N.Ref(arch=arch, B=B, HW=zeros.shape[1], c=-1.0, t=flat(synth["depth_orig"]), go=flat(go), h1=flat(conf[:, 0]),
                h2=flat(conf[:, 1]) if arch == 2 else zeros, npx=flat(torch.from_numpy(g[f"{pre}/noise/pixel"])),
                nim=g[f"{pre}/noise/image"].reshape(B) if arch == 2 else np.zeros(B, dtype=F), mp=flat(mk[:, 0]),
                mi=flat(mk[:, 1]) if arch == 2 else np.ones_like(zeros))
    before = sub(g, "init/G") if it == 0 else sub(g, f"s{it - 1}/after/G")
    w = [float(before[k]) for k in TAU_KEYS[str(g["meta/arch"])]]
    return inp, w + [0.0] * (2 - len(w))


# ---- (a) the restatement meets the reference's recorded gradients; the defects do not ---------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_a_reference_gradients_and_defects(case):
    g = load("step_" + case)
    keys = TAU_KEYS[str(g["meta/arch"])]
    flagged = {"no_sigma": 0, "si_for_sp": 0, "clean_l": 0}
    for it in range(int(g["meta/steps"])):
        inp, (wp, wi) = fixture_step(g, it)
        assert it == 0 or wp != 0.0                                    # (the second step runs at trained weights)
        r = T.lt_bwd_ref(inp, wp, wi)
        # the head gradients sum to the recorded head-bias gradients: the operands are the reference's
        gb = [float(g[f"s{it}/grad_G/{HEAD_B[0]}"][0])] + [float(v) for v in g[f"s{it}/grad_G/{HEAD_B[1]}"]]
        for ch in range(1 + inp.arch):
            assert abs(r.d[ch].sum() - gb[ch]) <= 1e-3 * np.abs(r.d[ch]).sum(), (it, ch)
        for k, key in enumerate(keys):
            ref, A = float(g[f"s{it}/grad_G/{key}"]), float(g[f"s{it}/grad_G_mag/{key}"])
            w = (wp, wi)[k]
            val, _ = T.dtau_ref(r, k, w, 0, 0)
            sg, _ = T.sigma_parts(w)
            assert abs(sg * np.abs(r.g[k]).sum() - A) <= 1e-4 * A, (it, key)    # the recorded magnitude is this sum's
            assert abs(ref) >= 0.01 * A and abs(val - ref) <= 1e-3 * A, (it, key, val, ref, A)
            assert abs(2.0 * val - ref) > 1e-2 * A                               # (what the seed condition buys)
            bad = {"no_sigma": T.dtau_ref(r, k, w, 0, 0, defect="no_sigma")[0],
                   "clean_l": T.dtau_ref(T.lt_bwd_ref(inp, wp, wi, defect="clean_l"), k, w, 0, 0)[0]}
            if k == 0 and inp.arch == 2:
                bad["si_for_sp"] = T.dtau_ref(T.lt_bwd_ref(inp, wp, wi, defect="si_for_sp"), k, w, 0, 0)[0]
            for name, v in bad.items():
                assert abs(v - ref) > 1e-3 * A, (it, key, name, v, ref, A)
                flagged[name] += 1
    assert flagged["no_sigma"] and flagged["clean_l"] and (flagged["si_for_sp"] or str(g["meta/arch"]) == "dusty1")


# ---- (b) float32 stays inside, the inputs keep their promise, wrong slopes fall outside -------------------------------------------------
def test_b_slopes():
    for w in T.WEIGHTS + (-30.0, 20.0):
        inv, e = T.slope(w)
        assert abs(float(T.slope32(w)) - inv) <= e, w
        assert inv >= 1.0 and e < 1e-5 * inv
    # the bit-identity test's choice: softplus(-30) vanishes under half an ulp of 0.5, the slope IS 1 / tau_max
    # (9.4e-14, with any error the two functions may make, against 2^-25)
    assert T.slope32(-30.0, 0.5) == F(0.5) and 2.0 * float(T.softplus64(-30.0)) < 2.0 ** -26


@pytest.mark.parametrize("case", T.LT_BWD, ids=T.lt_case_id)
def test_b_inputs_keep_their_promise(case):
    inp = T.lt_case_inputs(case)
    assert T.excluded_pixels_lt(inp, case[4], case[5]) == 0
    N.assert_normal([inp.t, inp.go, inp.h1, inp.h2, inp.npx, inp.nim] + T.lt_intermediates(inp, case[4], case[5]), T.lt_case_id(case))


@pytest.mark.parametrize("case", [c for c in T.LT_BWD if c[3] <= 4096], ids=T.lt_case_id)
def test_b_float32_inside_and_defects_outside(case):
    tier, arch, B, HW, wp, wi = case
    inp = T.lt_case_inputs(case)
    r = T.lt_bwd_ref(inp, wp, wi)
    d32, g32 = T.lt_bwd32(inp, wp, wi)
    for ch in range(1 + arch):
        assert N.check(f"d{ch}", d32[ch], r.d[ch], r.b[ch]) <= 1.0
    adds, hb = N.head_bwd_adds(B, HW, HW % 4 == 0)
    for k in range(arch):
        assert N.check(f"g{k}", g32[k], r.g[k], r.gb[k]) <= 1.0
        w = (wp, wi)[k]
        val, bnd = T.dtau_ref(r, k, w, adds, 0)
        got = F(F(1.0) / (F(1.0) + np.exp(-F(w)))) * g32[k].astype(F).sum(dtype=F)          # (one order of summation among many)
        assert abs(float(got) - val) <= bnd, (k, float(got), val, bnd)
        # a reference without sigma(w) would be told apart by the bound
        assert abs(T.dtau_ref(r, k, w, adds, 0, defect="no_sigma")[0] - val) > bnd
    # wrong slopes: without 1 / tau_max, or (dusty2) the other sigmoid's, d1 leaves its bound
    for defect in ("no_min",) + (("d_uses_other",) if arch == 2 else ()):
        bad = T.lt_bwd_ref(inp, wp, wi, defect=defect)
        q, rep = N.check("d1", d32[1], bad.d[1], bad.b[1], fail=False)
        assert q > 1.0 and rep, (defect, q)


# ---- (c) modules -------------------------------------------------------------------------------------------------------------------------
def _cfg(g, tau):
    from dusty_gan_amd.utils.config import load_config
    arch = str(g["meta/arch"])
    H, W = (int(v) for v in g["meta/shape"])
    cfg = load_config([f"model={arch}_dcgan_eqlr", "dataset=synthetic", f"dataset.shape=[{H},{W}]", f"model.gen.in_ch={int(g['meta/in_ch'])}",
                       f"model.gen.ch_base={int(g['meta/ch_base'])}", f"model.gen.ch_max={int(g['meta/ch_max'])}", f"model.gen.tau={tau}"])
    cfg.model.gen.shape = cfg.dataset.shape
    return cfg


@pytest.mark.parametrize("case", CASES)
def test_c_define_G_with_a_learnable_tau_builds_the_references_parameters(case):
    from dusty_gan_amd import engine as E
    from dusty_gan_amd.models import define_G
    g = load("step_" + case)
    arch = str(g["meta/arch"])
    ref = sub(g, "init/G")
    G = define_G(_cfg(g, "null"))
    sd = G.state_dict()
    assert list(sd.keys()) == list(ref.keys())
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in ref.values()]
    names = [k for k, _ in G.named_parameters()]
    assert names == [k for k in ref if k != "drop_const"] and names[-len(TAU_KEYS[arch]):] == TAU_KEYS[arch]
    for k in TAU_KEYS[arch]:
        assert sd[k].shape == () and float(sd[k]) == 0.0 == float(ref[k])         # the reference's init
    st = G.store
    seg = list(st.seg.values())
    assert seg[-1].name == "tau_w" and seg[-1].kind == "scalar" and seg[-1].shape == (len(TAU_KEYS[arch]),)
    assert seg[-2].name == "head_b" and seg[-1].off >= seg[-2].off + seg[-2].numel and st.n == st.flat.numel() == E._align(seg[-1].off + 1)
    assert G.backbone.tau_learn and G.backbone.inv_tau_min == 1.0
    # the weights ARE the store's floats: loading writes through, in order pixel, image
    sd2 = {k: v.clone() for k, v in ref.items()}
    for i, k in enumerate(TAU_KEYS[arch]):
        sd2[k] = torch.tensor(0.25 * (i + 1))
    G.load_state_dict(sd2)
    assert st.view("tau_w").tolist() == [0.25 * (i + 1) for i in range(len(TAU_KEYS[arch]))]
    for k, v in G.state_dict().items():
        assert torch.equal(v, sd2[k]), k
    G.eval()
    G._sync()                                                      # the by-value tau of the inference paths, from the pixel weight
    assert abs(G.backbone.tau - 1.0 / (float(T.softplus64(0.25)) + 1.0)) < 1e-12
    # the other kind, both ways: torch's usual errors
    Gf = define_G(_cfg(g, 1))
    with pytest.raises(RuntimeError, match="Unexpected key"):
        Gf.load_state_dict(sd2)
    with pytest.raises(RuntimeError, match="Missing key"):
        G.load_state_dict(Gf.state_dict())


@pytest.mark.parametrize("arch", ["dusty1", "dusty2"])
def test_c_numeric_tau_is_what_it_was(arch):
    from dusty_gan_amd import engine as E
    from dusty_gan_amd.models import define_G
    g = load(f"step_{arch}_ring")                                   # the reference's state dict at tau: 1
    G = define_G(_cfg(g, 1))
    assert list(G.state_dict().keys()) == list(sub(g, "init/G").keys())
    bb = G.backbone
    plain = E.ParamStore(E.g_segments(bb.in_ch, bb.chs, bb.shape, 1 + E.ARCH_ID[arch]))
    assert G.store.n == plain.n and list(G.store.seg) == list(plain.seg) and "tau_w" not in G.store.seg
    assert [s.off for s in G.store.seg.values()] == [s.off for s in plain.seg.values()]
    assert not bb.tau_learn and not any("gumbel" in k for k, _ in G.named_parameters())
    G._sync()
    assert bb.tau == 1.0


def test_c_what_stays_refused_and_the_declared_entry_points():
    from dusty_gan_amd import _lib
    from dusty_gan_amd.models.dusty import GumbelSigmoid
    with pytest.raises(NotImplementedError, match="hard=False"):
        GumbelSigmoid(tau=None, hard=False)
    with pytest.raises(NotImplementedError, match="hard=False"):
        GumbelSigmoid(tau=1.0, hard=False)
    assert GumbelSigmoid(tau=None).weight.shape == () and not hasattr(GumbelSigmoid(tau=1.0), "weight")
    P = _lib.PROTOTYPES
    for lt, old, extra in (("dg_head_post_fwd_lt", "dg_head_post_fwd", 1), ("dg_head_post_fwd_sum_lt", "dg_head_post_fwd_sum", 1),
                           ("dg_head_post_bwd_lt", "dg_head_post_bwd", 2), ("dg_head_post_bwd_aug_lt", "dg_head_post_bwd_aug", 2)):
        assert len(P[lt]) == len(P[old]) + extra, lt
