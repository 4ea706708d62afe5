"""The kernels and the launch mode that `bench.py` times, under the checker.

`bench.py` runs BASELINE.json configs[1]: dcgan_eqlr baseline, 64x1024, 32 images per GPU, bf16, R1 + DiffAugment, the
step replayed from a hipGraph.  At that size every fat layer runs on the persistent large-tile conv with SEVERAL tiles
per workgroup (cross-tile LDS-DMA ring, counted-vmcnt epilogue overlap, LDS bias-gradient carry), the weight gradients
on the LDS-DMA wgrad kernel and Proj.weight on the fused gradient-GEMM + Adam kernel - none of which the small golden
cases reach.  Every test here asserts through `dg_conv_plan` / `dg_wgrad_kernel_variant` (engine.TRACE) that those
kernels are what actually ran.  Oracle = oracle/dusty_oracle.py (CPU fp32, pinned to the reference by tests/golden).
"""
import math

import pytest
import torch

from dusty_gan_amd._lib import (DG_CONV_FAMILY_LOCKSTEP, DG_CONV_FAMILY_PINGPONG, DG_FORCE_LOCKSTEP, DG_FORCE_PINGPONG,
                                DG_WGRAD_VARIANT_DMA)
from tests import test_gpu_ops as OPS
from tests.golden_util import rel_l2
from tests.test_gpu_step import _cos, make_trainer, run_both

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture
def trace():
    from dusty_gan_amd import engine as E
    E.TRACE = []
    yield E.TRACE
    E.TRACE = None


def _persist(trace):
    return [t for t in trace if t[0] == "conv" and t[1] in (DG_CONV_FAMILY_LOCKSTEP, DG_CONV_FAMILY_PINGPONG)]


# (Ci, Co, H, W, B, dtype, wg_cap, force): the large-tile kernel with `wg_cap` workgroups, i.e. >= 4 tiles per workgroup, on
# all three tile shapes (256 x 128, 256 x 64, 128 x 128), both modes, adj 0 / 1, bias-gradient sums with per-sample
# weights, uneven chunk lengths (tile count not a multiple of the workgroup count)
MULTI = [
    (128, 256, 4, 128, 8, torch.bfloat16, 5, DG_FORCE_PINGPONG),    # 256 x 128 tiles from 2 samples' row segments
    (256, 128, 4, 128, 8, torch.bfloat16, 3, DG_FORCE_PINGPONG),
    (128, 128, 4, 512, 4, torch.bfloat16, 7, DG_FORCE_PINGPONG),    # two x tiles per row
    (128, 256, 4, 64, 16, torch.bfloat16, 4, DG_FORCE_PINGPONG),    # 4 samples' row segments per tile
    (64, 128, 4, 256, 4, torch.bfloat16, 5, DG_FORCE_PINGPONG),     # 64-channel side: 256 x 64 tiles in the backward-data passes
    (128, 256, 4, 128, 8, torch.bfloat16, 5, DG_FORCE_LOCKSTEP),    # the lock-step kernel on the same geometries
    (128, 256, 4, 64, 14, torch.bfloat16, 6, DG_FORCE_LOCKSTEP),    # 14 % 4 != 0: 128 x 128 tiles from 2 samples' row segments
    (64, 128, 4, 256, 4, torch.bfloat16, 5, DG_FORCE_LOCKSTEP),
    (128, 256, 4, 64, 16, torch.float32, 3, DG_FORCE_LOCKSTEP),     # fp32 instance (64-byte stages x 4)
    (128, 128, 4, 256, 8, torch.float32, 5, DG_FORCE_LOCKSTEP),
]


@pytest.mark.parametrize("Ci,Co,H,W,B,dtype,cap,force", MULTI)
@pytest.mark.parametrize("which", ["down", "up"])
def test_persistent_conv_several_tiles_per_workgroup(monkeypatch, trace, which, Ci, Co, H, W, B, dtype, cap, force):
    from dusty_gan_amd.engine import Ops
    monkeypatch.setattr(Ops, "default_wg_cap", cap)
    from dusty_gan_amd import _lib as L
    fn = OPS.test_down_fwd_bwd_wgrad if which == "down" else OPS.test_up_fwd_bwd_wgrad
    fn(L, Ci, Co, H, W, B, True, dtype, force)
    family = {DG_FORCE_LOCKSTEP: DG_CONV_FAMILY_LOCKSTEP, DG_FORCE_PINGPONG: DG_CONV_FAMILY_PINGPONG}[force]
    pc = [t for t in trace if t[0] == "conv" and t[1] == family]
    # forward + backward-data both on the persistent kernel (bf16: run_conv repeats the backward-data launch without the
    # saved mask bits to compare the two forms)
    assert len(pc) == (2 if dtype != torch.bfloat16 else 3), trace
    for t in pc:
        assert t[5] <= cap and t[6] >= 4, t         # workgroups <= cap, >= 4 tiles per workgroup


def _check_step(res, tr, state, amp, loss_tol=None, x3=False):
    G, D, G_ema = state
    sc_ref, ex, synth, gD, gG, scal = res
    keys = ["loss/D/output/real", "loss/D/output/fake", "loss/D/adversarial", "loss/D/gradient_penalty",
            "loss/G/adversarial"]
    out_tol = 2e-2 if amp else 1e-3
    loss_tol = loss_tol or (1e-2 if amp else 1e-3)
    for k, v in zip(keys, scal):
        assert abs(v - sc_ref[k]) <= loss_tol * max(1.0, abs(sc_ref[k])), (k, v, sc_ref[k])
    for k in synth:
        if k == "mask":
            assert (synth[k] != ex["synth"][k]).float().mean() < (1e-2 if amp else 1e-4)
        else:
            assert rel_l2(synth[k], ex["synth"][k]) < out_tol, (k, rel_l2(synth[k], ex["synth"][k]))
    # Gradients: the same linear maps given the same leaky-relu masks; units within rounding of zero take the other slope
    # (DESIGN.md "Precision contract").  D's gradients see that only: fp32 cosine >= 0.9999 / rel-L2 <= 2e-2, bf16
    # cosine >= 0.97 / rel-L2 <= 0.25.  G's gradients are taken through the UPDATED discriminator (reference :238 before
    # :260), and the first Adam step at beta1 = 0 is lr * sign(g): every D weight whose gradient is rounding noise lands
    # 2 lr apart in the two implementations, so the two G phases differentiate slightly different discriminators - fp32
    # measured cosine 0.9991 at B = 32 (0.99995 at B = 2); held to 0.998 / 8e-2.
    lim = {("grad_D", False): (0.9999, 2e-2), ("grad_G", False): (0.998, 8e-2),
           ("grad_D", True): (0.97, 2.5e-1), ("grad_G", True): (0.97, 2.5e-1)}
    for name, got, ref in (("grad_D", gD, ex["grad_D"]), ("grad_G", gG, ex["grad_G"])):
        cmin, rmax = lim[(name, amp)]
        for k, v in ref.items():
            if v.abs().max() > 0:
                if x3 and v.numel() <= 4:
                    # (fp32x3: a head bias gradient is ONE number per head, the sum of 10^5-10^6 signed per-pixel gradients that cancel
                    #  to ~1e-3 of their absolute sum; the split products' 1e-4 per-pixel error shows there first: 9e-2 measured at
                    #  128x2048, 3.7e-2 at 64x1024 - tests/test_gpu_configs.py)
                    assert rel_l2(got[k], v) < 2e-1, (name, k, rel_l2(got[k], v))
                    continue
                assert _cos(got[k], v) > cmin, (name, k, _cos(got[k], v))
                assert rel_l2(got[k], v) < rmax, (name, k, rel_l2(got[k], v))
    # Post-Adam parameters and the EMA.  First step, beta1 = 0: the update is lr * g / (|g| + eps) ~ lr * sign(g), so
    # every element must be within 2 lr of the oracle's, N(0,1)-initialised tensors within 1e-3 rel-L2, and the step must
    # have the oracle's sign on the bulk of a tensor (all of it up to gradient elements that are rounding noise)
    lr = 0.002
    for tag, net, ref in (("G", tr.G, G), ("D", tr.D, D), ("G_ema", tr.G_ema, G_ema)):
        sd = net.state_dict()
        for k, v in ref.items():
            if k == "drop_const" or k.endswith("kernel"):
                continue
            got = sd[k].cpu()
            assert float((got - v).abs().max()) <= 2.001 * lr, (tag, k)
            if float(v.abs().mean()) > 0.1:
                assert rel_l2(got, v) < 1e-3, (tag, k)
            if tag != "G_ema" and v.numel() >= 64:
                agree = ((got - v).abs() < 0.5 * lr).float().mean()   # same sign of the step
                # (G's step direction inherits the updated-discriminator effect above: fp32 measured 0.985 on Proj.weight)
                assert agree > (0.85 if amp else (0.97 if tag == "G" else 0.99)), (tag, k, float(agree))


@pytest.mark.parametrize("amp", [True, False], ids=["bf16", "fp32"])
def test_bench_configuration_step_vs_oracle(trace, amp):
    """BASELINE configs[1] exactly as bench.py runs it (arch none, 64x1024, B = 32, default kernel selection), one step
    with injected randomness against the CPU oracle; bf16 = the timed mode, fp32 = the parity mode (<= 1e-3)."""
    tr, state, res = run_both("none", (64, 1024), 512, 64, 512, 32, amp=amp)
    pc = _persist(trace)
    assert len(pc) >= 10 and max(t[6] for t in pc) > 1, pc          # persistent conv with tcount > 1 ran ...
    assert any(t[2:4] == (256, 128) for t in pc)
    if amp:
        assert any(t[0] == "wgrad" and t[1] == DG_WGRAD_VARIANT_DMA for t in trace)    # ... and the LDS-DMA weight-gradient kernel
        assert tr.optim_G.regen_grad is not None                    # Proj.weight went through dg_adam_proj_fused
        assert tr.proj_route.name == "FUSED"
    _check_step(res[0], tr, state, amp)


def test_graph_replay_matches_eager_at_bench_size(monkeypatch):
    """hipGraph replay (what bench.py times) against eager launches at 64x1024, B = 32, bf16: same seeds -> same
    parameters after 2 eager + 3 replayed steps, bit for bit (round 5, deterministic sums; with DUSTY_GAN_DETERMINISTIC=0
    atomics reorder the last bits, Adam at beta1 = 0 turns a sign change of a near-zero gradient into a 2 lr difference:
    bounded per element; over G - 96 % of it Proj.weight, whose gradients are bf16-noise-sized for most elements - repeated
    runs measured 0.9e-3 ... 1.05e-3 rel-L2, hence the 2.5e-3 bound of that mode)"""
    def run(graph):
        monkeypatch.setenv("DUSTY_GAN_GRAPH", "1" if graph else "0")
        torch.manual_seed(99)
        tr = make_trainer("none", True, (64, 1024), 512, 64, 512, 32, amp=True)
        sc = [dict(tr.step(i).items()) for i in range(5)]
        assert (tr._graph is not None) == graph
        return tr, sc
    from dusty_gan_amd import engine as E
    E.WGRAD_WS._by_stream.clear()
    a, sa = run(True)
    # the split-K workspace of the capture stream started at the size the eager warm-up steps had grown theirs to: a
    # workspace that grows DURING capture bakes its extra reduce launches into every replay (round 4: 59 launches, not 58)
    wss = list(E.WGRAD_WS._by_stream.values())
    assert len(wss) >= 2 and all(w.buf is not None for w in wss), [(w.grows, w.buf is not None) for w in wss]
    assert wss[0].grows >= 1 and all(w.grows == 1 and w.early_flushes == 0 for w in wss[1:]), [w.grows for w in wss]
    b, sb = run(False)
    for net in ("G", "D", "G_ema"):
        fa, fb = getattr(a, net).store.flat.cpu(), getattr(b, net).store.flat.cpu()
        if E.DETERMINISTIC:   # round 5: no order-dependent sum is left on this path - the two launch forms agree bit for bit
            assert torch.equal(fa, fb), (net, rel_l2(fa, fb))
            continue
        assert rel_l2(fa, fb) < 2.5e-3, (net, rel_l2(fa, fb))
        assert float((fa - fb).abs().max()) <= 0.05, net  # (Adam can move an element ~sqrt(k) lr at step k)
    for x, y in zip(sa, sb):
        for k in x:
            # deterministic sums: the two launch forms execute the same additions - the logged scalars agree like the parameters
            # (1e-6 for the one float-rounding a different launch form may add); with atomics the mean raw logits had run-to-run
            # noise of their own (tests/test_gpu_step.py)
            tol = 1e-6 if E.DETERMINISTIC else (4e-2 if "/output/" in k else 2e-2)
            assert abs(x[k] - y[k]) <= tol * max(1.0, abs(y[k])), (k, x[k], y[k])


def test_replayed_step_makes_at_most_48_launches(monkeypatch):
    """The launch count of the step bench.py times (config 2: 64x1024, B = 32, bf16, R1 + DiffAugment on), counted as kernel
    nodes of the captured hipGraph: 48 (round 5: 54; round 4: 58) - the depth head applies its tanh and sums itself (DgConv.tanh_sum_parts), fetch_reals rides on the step's first launch
    (dg_step_prologue_fetch), R1's turn-around at the image is one launch (dg_blur_r1_tangent), each network's optimizer is one
    launch that sums its own partial tiles (dg_adam_fused) plus the small shadow / counter launch behind it.  A workspace that
    grows during capture, a fallback to an unfused form, a stray zero-fill - each shows up here as a number."""
    monkeypatch.setenv("DUSTY_GAN_GRAPH", "1")
    monkeypatch.setenv("DUSTY_GAN_KEEP_GRAPH", "1")
    torch.manual_seed(7)
    tr = make_trainer("none", True, (64, 1024), 512, 64, 512, 32, amp=True)
    for i in range(4):
        tr.step(i)
    assert tr._graph is not None
    n = tr.graph_kernel_nodes()
    assert n is not None, "hipGraphGetNodes did not answer"
    assert 40 <= n <= 48, n


@pytest.mark.parametrize("arch,amp", [("none", True), ("dusty2", True), ("dusty2", False)], ids=["none", "dusty2", "dusty2-fp32x3"])
def test_two_runs_from_one_seed_are_bit_identical(monkeypatch, arch, amp):
    """SURVEY section 5 "determinism check by double-run", at the timed configuration (64x1024, bf16, B = 32; `none` =
    BASELINE config 2, `dusty2` = config 4's per-GPU share): two trainers built from one seed end five steps with IDENTICAL
    bits in G, D and G_ema - replayed from the hipGraph and launched eagerly, and the two forms agree with each other too.
    Rounds 1-4 ended such runs 1e-3 apart: bias-gradient sums and per-sample image sums / logits went through float atomics
    in arrival order, and Adam at beta1 = 0 turns a sign flip of a rounding-noise gradient into a +-lr step.  Round 5:
    per-workgroup partial rows summed in a fixed order (DgConv.dbias_part, dg_final_gan_bwd's dbias_part) and fixed-point
    integer accumulation for the accumulator arena (dg_det_arena).  fp32x3: the parity-class mode with split-bf16 storage (B = 8)
    - its fat layers run the same kernels in their DG_BF16X2 forms, the two-channel ends the fp32 VALU kernels, whose bias-gradient
    sums (thin_smallk: fixed-point staging) and weight gradients (partial tiles through the split-K workspace) are
    order-independent too."""
    from dusty_gan_amd import engine as E
    assert E.DETERMINISTIC
    monkeypatch.setenv("DUSTY_GAN_FP32_SPLIT", "0" if amp else "1")

    def run(graph):
        monkeypatch.setenv("DUSTY_GAN_GRAPH", "1" if graph else "0")
        torch.manual_seed(4242)
        tr = make_trainer(arch, True, (64, 1024), 512, 64, 512, 32 if amp else 8, amp=amp)
        assert amp or (tr.fp32_pairs and tr.D.engine().x2)
        sc = [dict(tr.step(i).items()) for i in range(5)]
        assert (tr._graph is not None) == graph
        torch.cuda.synchronize()
        return {k: getattr(tr, k).store.flat.clone() for k in ("G", "D", "G_ema")}, sc
    g1, s1 = run(True)
    g2, s2 = run(True)
    e1, s3 = run(False)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), ("two graph runs", k, rel_l2(g1[k].cpu(), g2[k].cpu()))
        assert torch.equal(g1[k], e1[k]), ("graph against eager", k, rel_l2(g1[k].cpu(), e1[k].cpu()))
    for x, y in zip(s1, s2):     # (the logged scalars are means formed with float atomics: equal to rounding, not to the bit)
        for k in x:
            assert abs(x[k] - y[k]) <= 1e-5 * max(1.0, abs(y[k])), (k, x[k], y[k])


@pytest.mark.parametrize("amp,B,x3", [(False, 2, False), (True, 4, False), (False, 2, True)], ids=["fp32-B2", "bf16-B4", "fp32x3-B2"])
def test_config5_shapes_whole_step(monkeypatch, trace, amp, B, x3):
    """BASELINE configs[4] shapes: dusty2, 128x2048 (Proj / final kernels (8,128), fat layers at 2x the spatial size,
    524 288-long final dots), one whole step against the oracle.  fp32x3: the split-bf16 storage form (DG_BF16X2) at this size,
    held to the fp32 mode's bounds."""
    monkeypatch.setenv("DUSTY_GAN_FP32_SPLIT", "1" if x3 else "0")
    tr, state, res = run_both("dusty2", (128, 2048), 512, 64, 512, B, amp=amp)
    assert tr.fp32_pairs == x3 and tr.D.engine().x2 == x3
    assert len(_persist(trace)) >= 1
    # (the final conv is a 524 288-long dot of bf16 activations: logits / losses held to 2e-2 here)
    _check_step(res[0], tr, state, amp, loss_tol=2e-2 if amp else None, x3=x3)
