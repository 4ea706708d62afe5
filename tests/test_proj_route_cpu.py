"""The route of Proj.weight's gradient in the G phase (trainers/dcgan_amp.py `ProjRoute`, `proj_route`) as a pure decision:
checked on every combination of its inputs against the three boolean expressions `Trainer.optimize_G` held before the
route had a name.  No GPU, no library load."""
import itertools
import math

import pytest
import torch

from dusty_gan_amd.trainers.dcgan_amp import ProjRoute, proj_route

R = ProjRoute
BF16, FP32, FP16 = torch.bfloat16, torch.float32, torch.float16


def oracle(world, force_seg, n_acc, dtype, first_seg, proj_off, fuse_proj_ok, fuse_proj_fp32, beta1, profile):
    """the former expressions, verbatim up to `self.` / `Gst.` / `E.PROFILE` becoming plain values"""
    gather_proj = (world > 1 or force_seg) and n_acc == 1 and first_seg == "proj_w"
    fuse_proj = (not gather_proj and world == 1 and n_acc == 1 and dtype in (torch.bfloat16, torch.float32)
                 and (dtype == torch.bfloat16 or fuse_proj_fp32)
                 and first_seg == "proj_w" and proj_off == 0 and fuse_proj_ok
                 and beta1 == 0.0 and profile is None)
    fuse_gathered = (gather_proj and dtype == torch.bfloat16 and proj_off == 0
                     and fuse_proj_ok and beta1 == 0.0 and profile is None)
    if fuse_gathered:
        return R.GATHER_FUSED
    if gather_proj:
        return R.GATHER
    if fuse_proj:
        return R.FUSED
    return R.MATERIALISED


def test_route_agrees_with_the_former_expressions_on_every_input():
    n = 0
    for world, force_seg, n_acc, dtype, proj_first, fuse_ok, fuse_fp32, profiling, beta1 in itertools.product(
            (1, 2), (False, True), (1, 2), (BF16, FP32, FP16), (True, False), (True, False), (True, False), (True, False),
            (0.0, 0.5)):
        # (proj_w is the first segment -> its offset is 0: ParamStore lays the segments out from 0; elsewhere any other)
        first_seg, off = ("proj_w", 0) if proj_first else ("up1_w", 256)
        want = oracle(world, force_seg, n_acc, dtype, first_seg, off, fuse_ok, fuse_fp32, beta1, [] if profiling else None)
        got = proj_route(multi_rank_schedule=world > 1 or force_seg, n_acc=n_acc, dtype=dtype, proj_first=proj_first,
                         fuse_ok=fuse_ok, fuse_fp32=fuse_fp32, beta1=beta1, profiling=profiling)
        assert got is want, (world, force_seg, n_acc, dtype, proj_first, fuse_ok, fuse_fp32, profiling, beta1, got, want)
        n += 1
    assert n == 2 * 2 * 2 * 3 * 2 * 2 * 2 * 2 * 2


def test_the_first_segment_starts_at_offset_zero():
    """what lets `Gst.seg["proj_w"].off == 0` drop out of the rule"""
    from dusty_gan_amd.engine import NetCfg, ParamStore, g_segments
    st = ParamStore(g_segments(8, (4, 8, 16, 16), (32, 64), 2))
    assert next(iter(st.seg)) == "proj_w" and st.seg["proj_w"].off == 0
    c = NetCfg((32, 64), 8, (4, 8, 16, 16))
    assert c.proj_rows * c.nz == st.seg["proj_w"].numel and c.proj_scale == 1.0 / math.sqrt(c.proj_rows)


@pytest.mark.parametrize("route,skips,gathers,in_opt", [
    (R.MATERIALISED, False, False, False), (R.FUSED, True, False, True), (R.GATHER, True, True, False),
    (R.GATHER_FUSED, True, True, True)])
def test_derived_properties(route, skips, gathers, in_opt):
    assert (route.skips_backward, route.gathers, route.in_optimizer) == (skips, gathers, in_opt)
    assert len(R) == 4


# every input not named in a row: one rank, no force_seg, one micro-batch, bf16, proj_w first, fuse_ok, fuse_fp32, beta1 0,
# not profiling
FAVOURABLE = dict(multi_rank_schedule=False, n_acc=1, dtype=BF16, proj_first=True, fuse_ok=True, fuse_fp32=True, beta1=0.0,
                  profiling=False)
MULTI = dict(multi_rank_schedule=True)
ROWS = [
    ("single rank, bf16, fusable", {}, R.FUSED),
    ("single rank, fp32, fuse_fp32", dict(dtype=FP32), R.FUSED),
    ("single rank, fp32, fuse_fp32 off", dict(dtype=FP32, fuse_fp32=False), R.MATERIALISED),
    ("single rank, bf16, fuse_ok off", dict(fuse_ok=False), R.MATERIALISED),
    ("single rank, bf16, beta1 = 0.5", dict(beta1=0.5), R.MATERIALISED),
    ("single rank, bf16, profiling", dict(profiling=True), R.MATERIALISED),
    ("multi-rank, bf16, fusable", MULTI, R.GATHER_FUSED),
    ("multi-rank, fp32, fusable", dict(MULTI, dtype=FP32), R.GATHER),
    ("multi-rank, bf16, fuse_ok off", dict(MULTI, fuse_ok=False), R.GATHER),
    ("single rank, n_acc = 2", dict(n_acc=2), R.MATERIALISED),
    ("multi-rank, n_acc = 2", dict(MULTI, n_acc=2), R.MATERIALISED),
    ("single rank, proj_first false", dict(proj_first=False), R.MATERIALISED),
    ("multi-rank, proj_first false", dict(MULTI, proj_first=False), R.MATERIALISED),
    ("single rank, fp16", dict(dtype=FP16), R.MATERIALISED),
]


@pytest.mark.parametrize("name,changed,want", ROWS, ids=[r[0] for r in ROWS])
def test_named_rows(name, changed, want):
    assert proj_route(**dict(FAVOURABLE, **changed)) is want
