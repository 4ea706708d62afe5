"""The form of R1 at the image in the D phase (trainers/dcgan_amp.py `R1Form`, `r1_form`) as a pure decision: the issue's
table of shapes, and on a sweep of shapes against the ladder of conditions `Trainer.optimize_D` and the two engine methods
held before the form had a name.  No GPU, no library load."""
import pytest
import torch

from dusty_gan_amd.engine import DEngine, NetCfg
from dusty_gan_amd.trainers.dcgan_amp import R1Form, r1_form

F = R1Form
ROWS = [
    ("the turn-around takes the shape", (32, 256, True), F.TURNAROUND),
    ("6*W*4 > 60 KiB refuses the turn-around, H*W % 1024 == 0", (16, 3072, True), F.FUSED_ADJOINT),
    ("turn-around refused and H*W % 1024 != 0", (16, 2576, True), F.THREE_PASS),
    ("no arena slice, turn-around shape", (32, 256, False), F.THREE_PASS),
    ("no arena slice, fused-adjoint shape", (16, 3072, False), F.THREE_PASS),
    ("no arena slice, three-pass shape", (16, 2576, False), F.THREE_PASS),
]


@pytest.mark.parametrize("name,args,want", ROWS, ids=[r[0] for r in ROWS])
def test_named_rows(name, args, want):
    H, W, have_ssq = args
    assert r1_form(H=H, W=W, have_ssq=have_ssq) is want
    assert len(F) == 3


def former_ladder(H, W, have_ssq):
    """the former conditions, verbatim up to `c.` becoming plain values: `ssq is None or not deng.r1_turnaround(...)` with
    its refusal `c.W % 4 or c.H % 4 or 6 * c.W * 4 > 60 * 1024`, then `ssq is None or not deng.backward_input(..., r1=)`
    with its refusal `not (c.W % 4 == 0 and (c.H * c.W) % 1024 == 0)`"""
    if not (not have_ssq or (W % 4 or H % 4 or 6 * W * 4 > 60 * 1024)):
        return F.TURNAROUND
    if not (not have_ssq or not (W % 4 == 0 and (H * W) % 1024 == 0)):
        return F.FUSED_ADJOINT
    return F.THREE_PASS


def test_form_and_engine_predicates_agree_on_a_sweep_of_shapes():
    seen = set()
    for H in (16, 32, 64):
        for W in range(64, 4097, 64):
            # (the predicates take plain H, W: NetCfg itself refuses H = 16, SURVEY.md §0.2, so a discriminator engine
            #  exists on the CPU for the two taller shapes only - there the values come out of its configuration)
            if H >= 32 and W % 16 == 0:
                deng = DEngine(NetCfg((H, W), 8, (4, 8, 16, 16)), torch.float32)
                turn, fused = deng.r1_turnaround_ok(deng.cfg.H, deng.cfg.W), deng.r1_fused_ok(deng.cfg.H, deng.cfg.W)
            else:
                turn, fused = DEngine.r1_turnaround_ok(H, W), DEngine.r1_fused_ok(H, W)
            want = F.TURNAROUND if turn else F.FUSED_ADJOINT if fused else F.THREE_PASS
            got = r1_form(H=H, W=W, have_ssq=True)
            assert got is want and got is former_ladder(H, W, True), (H, W, got, want)
            assert r1_form(H=H, W=W, have_ssq=False) is F.THREE_PASS is former_ladder(H, W, False), (H, W)
            seen.add(got)
    # (every W of the sweep is a multiple of 64, so H * W is one of 1024: with an arena slice the third form is the table's
    #  16 x 2576 alone)
    assert seen == {F.TURNAROUND, F.FUSED_ADJOINT}
