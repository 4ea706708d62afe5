"""tests/image_exact_util.py on the CPU: every case of the table satisfies the exactness condition, the float64 references are the
oracle's maps (equal to their float32 evaluation, adjoints exact transposes), the index-by-index restatements equal them - and the
written proof of the gap: each of the thirteen mutants is reported by a named case of the per-element comparators, while the
whole-tensor bounds of tests/test_gpu_fused_small.py (bf16: rel_l2 < 1e-2 against the oracle, 2e-3 / 1e-3 fused against unfused)
let most of them through at that file's own shape."""
import pytest
import torch

from oracle import dusty_oracle as O
from tests import image_exact_util as U
from tests.golden_util import rel_l2


def _f32_eval(fn, *args):
    """fn on float32 copies of the float64 arguments"""
    return fn(*[a.float() if torch.is_tensor(a) and a.is_floating_point() else a for a in args]).double()


def _rp32(rp):
    return {k: (v.float() if v.is_floating_point() else v) for k, v in rp.items()}


# ---- every case: the premise, the tie to the oracle, the adjoint identity ------------------------------------------------------
@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_case_is_exact_and_is_the_oracles(case):
    U.assert_exact_inputs(case)
    family, H, W, draws = case
    if family == "sum":
        return
    if family == "blur":
        k = U.blur(H, W, U.blur_batch(H, W))
        for ring in (True, False):
            assert torch.equal(k.fwd(ring), _f32_eval(U.blur64, k.x, ring))
            assert torch.equal(k.fwd(ring), U.blur_fwd_r(k.x, ring)) and torch.equal(k.adj(ring), U.blur_adj_r(k.d, ring))
            # <BlurVH x, d> == <x, BlurVH^T d>, exactly
            assert float((k.fwd(ring) * k.d).sum()) == float((k.x * k.adj(ring)).sum())
            assert torch.equal(k.tangent(ring), U.blur_fwd_r(U.OSCALE * U.blur_adj_r(k.d, ring), ring))
        return
    sets = [U.aug(H, W, draws)] + ([U.aug(H, W, draws, 1)] if (H, W, draws) in U.FUSED else [])
    for a in sets:
        for policy in U.policies_for(H, W):
            y = a.y(policy)
            assert torch.equal(y, O.diff_augment(a.x.float(), _rp32(a.rp), U.POLICIES[policy]).double())
            assert torch.equal(y, U.aug_fwd_r(a.x, a.rp, policy))
            gx, gsum = a.gx(policy), a.gsum(policy)
            assert torch.equal(gx, U.aug_adj_r(a.e, a.rp, policy)) and torch.equal(gsum, U.window_sum_r(a.e, a.rp, policy))
            # <A(x) - A(0), e> == <x, A^T e> per sample, exactly (brightness makes A affine)
            y0 = U.aug64(torch.zeros_like(a.x), a.rp, policy)
            assert torch.equal(((y - y0) * a.e).sum(dim=[1, 2, 3]), (a.x * gx).sum(dim=[1, 2, 3]))
            # the window sum, written from the reference's definition, is the derivative along a uniform shift of the image:
            # A(x + c) = A(x) + c on exactly the window's pixels, so the adjoint's total is the window's sum
            assert torch.equal(gx.sum(dim=[1, 2, 3]), gsum)
    if (H, W, draws) in U.FUSED:
        assert not torch.equal(sets[0].rp["t_w"], sets[1].rp["t_w"]) and not torch.equal(sets[0].x, sets[1].x)


def test_exhaustive_draws_are_what_the_oracle_draws():
    d = U.all_draws(8, 16)
    assert d["t_h"].shape[0] == 3 * 3 * 9 * 17 == 1377
    assert int(U.all_draws(4, 32)["t_h"].abs().max()) == 0
    g = torch.Generator().manual_seed(3)
    rp = O.draw_augment_params(4096, 8, 16, g)
    have = set(zip(*[d[k].tolist() for k in ("t_h", "t_w", "o_x", "o_y")]))
    seen = set(zip(*[rp[k].tolist() for k in ("t_h", "t_w", "o_x", "o_y")]))
    assert seen <= have and len(seen) > 1200
    e = U.extra_draws(8, 16)
    assert sorted(e["t_w"][:4].tolist()) == [-19, -15, 15, 16] and sorted(e["t_h"][4:].tolist()) == [-11, -8, 8, 11]


def test_bf16_exactness_is_as_the_criteria_assume():
    """BlurVH's outputs and the R1 tangent at OSCALE are bf16 numbers (assert_exact serves both types); BlurVH(A(x)) under contrast
    mostly is not: that is why its bf16 criterion is the RNE of the reference"""
    for H, W in U.TANGENT:
        k = U.blur(H, W)
        for ring in (True, False):
            assert torch.equal(k.tangent(ring).bfloat16().double(), k.tangent(ring))
    f = U.aug(16, 64, "some").fused("default", True)
    share = float((f.bfloat16().double() == f).double().mean())
    print("BlurVH(A(x)) 16 x 64, default policy: %.0f %% of the elements are bf16 numbers" % (100 * share))
    assert 0.05 < share < 0.95


def test_head_bias_gradient_launches_cover_contrast():
    """the head's bias gradient is compared over the leading samples whose total is exact in ANY order: all 25 pairs of factors
    without contrast, and under contrast at 8 x 16; at 16 x 64 the pivot term's unit (2^-13) leaves room for fewer"""
    for H, W, d in U.HEAD:
        a = U.aug(H, W, d)
        assert U.dbias_samples(a, "translation") == U.dbias_samples(a, "none") == U.DBIAS_SAMPLES
        print("head %d x %d: bias gradient over %d samples under the default policy" % (H, W, U.dbias_samples(a, "default")))
    assert U.dbias_samples(U.aug(8, 16, "all"), "default") == U.DBIAS_SAMPLES
    assert U.dbias_samples(U.aug(16, 64, "some"), "default") >= 1


# ---- the mutants ---------------------------------------------------------------------------------------------------------------
def _reported(fn, *args):
    with pytest.raises(AssertionError) as ei:
        fn(*args)
    msg = str(ei.value)
    assert "elements wrong" in msg and "by x % 4" in msg, msg
    return msg


def _old_shape(seed=11, B=3, H=64, W=1024):
    """the operands of the existing bf16 tests at their flagship shape: normal data, drawn parameters with the extreme ones"""
    g = torch.Generator().manual_seed(seed)
    rp = O.draw_augment_params(B, H, W, g)
    sh, sw = O.translation_shift(H, W)
    rp["t_h"][0], rp["t_w"][0], rp["o_x"][0], rp["o_y"][0] = -sh, sw, 0, 0
    rp["t_h"][1], rp["t_w"][1], rp["o_x"][1], rp["o_y"][1] = sh, -sw, H - 1, W - 1
    rp = {k: (v.double() if v.is_floating_point() else v) for k, v in rp.items()}
    x = torch.randn(B, 1, H, W, generator=g, dtype=torch.float64)
    d = torch.randn(B, H, W, 2, generator=g, dtype=torch.float64)
    return x, d, rp


# Each mutant: the named case the per-element comparator is given, and - mutants 1-7, 10, 11 - the rel_l2 the same defect leaves at
# 64 x 1024 on normal data against the bound of the existing bf16 test of that kernel, wrong wherever the defect applies and wrong
# at one pixel.  (`cut_h / 2` rounded up has no figure there: at 64 x 1024 the box height is even and the defect does nothing,
# which is why 6 x 12 is in the table.  Mutants 8, 9, 12, 13 are whole-image errors the old tests see as well; they are here
# because the exact data must tell them apart too.)
def _blur_fwd_case(H, W, ring, defect):
    k = U.blur(H, W)
    return lambda: U.assert_exact(U.blur_fwd_r(k.x, ring, defect).float(), k.fwd(ring), defect)


def _blur_adj_case(H, W, ring, defect):
    k = U.blur(H, W)
    return lambda: U.assert_exact(U.blur_adj_r(k.d, ring, defect).float(), k.adj(ring), defect)


def _aug_fwd_case(H, W, draws, policy, defect):
    a = U.aug(H, W, draws)
    return lambda: U.assert_exact(U.aug_fwd_r(a.x, a.rp, policy, defect).float(), a.y(policy), defect)


def _aug_adj_case(H, W, draws, policy, defect):
    a = U.aug(H, W, draws)
    return lambda: U.assert_exact(U.aug_adj_r(a.e, a.rp, policy, defect).float(), a.gx(policy), defect)


def _gsum_case(H, W, draws, policy, defect):
    a = U.aug(H, W, draws)
    return lambda: U.assert_exact(U.window_sum_r(a.e, a.rp, policy, defect).float(), a.gsum(policy), defect)


def _both(mut, ref):
    """(rel_l2 of the defect as restated: at every pixel it applies to, in every sample; rel_l2 of the same defect at ONE pixel -
    the first it touches: a single corner, quad edge or lane gone wrong)"""
    mut, ref = U.as4(mut), U.as4(ref)
    b, _, y, x = (mut != ref).nonzero()[0].tolist()
    loc = ref.clone()
    loc[b, :, y, x] = mut[b, :, y, x]
    return float(rel_l2(mut, ref)), float(rel_l2(loc, ref))


def _old_blur_fwd(defect):
    x, d, rp = _old_shape()
    return _both(U.blur_fwd_r(x, True, defect), U.blur_fwd_r(x, True))


def _old_blur_adj(defect, ring=True):
    x, d, rp = _old_shape()
    return _both(U.blur_adj_r(d, ring, defect), U.blur_adj_r(d, ring))


def _old_fused(defect, policy="default"):
    x, d, rp = _old_shape()
    return _both(U.blur_fwd_r(U.aug_fwd_r(x, rp, policy, defect), True), U.blur_fwd_r(U.aug_fwd_r(x, rp, policy), True))


def _old_adj(defect, policy="default"):
    x, d, rp = _old_shape()
    e = U.blur_adj_r(d, True)
    return _both(U.aug_adj_r(e, rp, policy, defect), U.aug_adj_r(e, rp, policy))


def _old_trunc():
    x, d, rp = _old_shape()
    f = U.blur_fwd_r(U.aug_fwd_r(x, rp, "default"), True).float().double()
    return _both(U.bf16_truncated(f).double(), f.float().bfloat16().double())


# Measured here (printed by the test below).  Wrong at every pixel it applies to, only mutants 10 and 11 stay under the old bound;
# wrong at ONE pixel, every mutant does - except mutant 5, whose single pixel (the source column that output columns 0 and W - 1
# share, missing one of its two gradients) leaves 1.6e-3 against the 1e-3 of the head's bf16 copy: that bound would see it, but
# it compares the fused launch with the unfused one, and both take the gather from csrc/diffaug.h.
OVER_AT_ONE_PIXEL = {"shared_col"}
OLD_R1, OLD_FUSED, OLD_PM = 1e-2, 2e-3, 1e-3   # test_r1_turnaround_in_one_launch (oracle), test_diffaug_blurvh_one_pass, the head's copy
MUTANTS = [
    # (number, name, the named case, its two rel_l2 at the old shape, the old bound, under it even where wrong everywhere)
    (1, "replicate", _blur_fwd_case(3, 12, True, "replicate"), lambda: _old_blur_fwd("replicate"), OLD_R1, False),
    (2, "no_double_row", _blur_adj_case(8, 16, True, "no_double_row"), lambda: _old_blur_adj("no_double_row"), OLD_R1, False),
    (2, "no_double_col", _blur_adj_case(6, 10, False, "no_double_col"), lambda: _old_blur_adj("no_double_col", False), OLD_R1, False),
    (3, "ring_clamp forward", _blur_fwd_case(2, 8, True, "ring_clamp"), lambda: _old_blur_fwd("ring_clamp"), OLD_R1, False),
    (3, "ring_clamp adjoint", _blur_adj_case(2, 8, True, "ring_clamp"), lambda: _old_blur_adj("ring_clamp"), OLD_R1, False),
    (4, "mod_W", _aug_fwd_case(8, 16, "all", "default", "mod_W"), lambda: _old_fused("mod_W"), OLD_FUSED, False),
    (5, "shared_col", _aug_adj_case(8, 16, "all", "translation", "shared_col"), lambda: _old_adj("shared_col"), OLD_PM, False),
    (6, "cut_row", _aug_fwd_case(8, 16, "all", "default", "cut_row"), lambda: _old_fused("cut_row"), OLD_FUSED, False),
    (6, "cut_col", _aug_fwd_case(8, 16, "all", "default", "cut_col"), lambda: _old_fused("cut_col"), OLD_FUSED, False),
    (6, "cut_half_up", _aug_fwd_case(6, 12, "some", "no-contrast", "cut_half_up"), None, OLD_FUSED, False),
    (7, "row_clamp", _aug_fwd_case(8, 16, "all", "default", "row_clamp"), lambda: _old_fused("row_clamp"), OLD_FUSED, False),
    (8, "pivot_no_br", _aug_fwd_case(8, 16, "all", "no-translation", "pivot_no_br"), None, OLD_FUSED, False),
    (9, "factor_u", _aug_fwd_case(8, 16, "all", "default", "factor_u"), None, OLD_FUSED, False),
    (10, "bf16 truncated", None, _old_trunc, OLD_R1, True),
    (11, "window_incl_cut", _gsum_case(8, 16, "all", "default", "window_incl_cut"), lambda: _old_adj("window_incl_cut"), OLD_PM, True),
    (11, "window_band_twice", _gsum_case(8, 16, "all", "default", "window_band_twice"), lambda: _old_adj("window_band_twice"), OLD_PM, True),
    (12, "second_trip", _blur_fwd_case(4, 1028, True, "second_trip"), None, OLD_R1, False),
]


@pytest.mark.parametrize("number,name,case,old,bound,under", MUTANTS, ids=[f"{m[0]}-{m[1].replace(' ', '-')}" for m in MUTANTS])
def test_mutant_is_reported_by_a_named_case(number, name, case, old, bound, under):
    if case is not None:
        _reported(case)
    if old is not None:
        r, r1 = old()
        say = lambda v: "under" if v < bound else "OVER"
        print("[image-exact] mutant %d %s at 64 x 1024: rel_l2 %.1e everywhere (%s the old bound %.0e), %.1e at one pixel (%s)" %
              (number, name, r, say(r), bound, r1, say(r1)))
        assert r >= r1 > 0
        if name not in OVER_AT_ONE_PIXEL:
            assert r1 < bound, (name, r1, bound)     # one pixel gone wrong: the old criterion cannot see it
        if under:
            assert r < bound, (name, r, bound)       # ... and these not even where the defect is everywhere


def test_mutant_10_truncating_store_is_reported():
    """BlurVH(A(x)) under contrast has elements between two bf16 numbers: a store that truncates misses the RNE on those it should
    have rounded away from zero"""
    a = U.aug(8, 16, "all")
    ref = a.fused("default", True)
    assert U.assert_rne(ref.float().bfloat16(), ref) == ref.numel()
    _reported(U.assert_rne, U.bf16_truncated(ref), ref, "truncated")


def test_mutant_13_second_set_with_the_first_sets_parameters_is_reported():
    a0, a1 = U.aug(8, 16, "all"), U.aug(8, 16, "all", 1)
    wrong = U.blur64(U.aug64(a1.x, a0.rp, "default"), True)
    _reported(U.assert_exact, wrong.float(), a1.fused("default", True), "second set")
    # ... and on the smallest fused case too
    b0, b1 = U.aug(4, 8, "some"), U.aug(4, 8, "some", 1)
    _reported(U.assert_exact, U.blur64(U.aug64(b1.x, b0.rp, "default"), True).float(), b1.fused("default", True), "second set")


def test_every_listed_mutant_has_a_case():
    assert sorted({m[0] for m in MUTANTS} | {13}) == list(range(1, 14))
    assert all(m[2] is not None or m[0] == 10 for m in MUTANTS)


def test_comparators_pass_the_reference_and_see_one_element():
    k = U.blur(3, 12)
    ref = k.fwd(True)
    assert U.assert_exact(ref.float(), ref) == ref.numel() and U.assert_exact(ref.bfloat16(), ref) == ref.numel()
    one = ref.float().clone()
    one[2, 1, 7, 1] += 0.25
    msg = _reported(U.assert_exact, one, ref, "one tap")
    assert "1 of %d elements wrong" % ref.numel() in msg and "(b=2, c=1, y=1, x=7" in msg
    nan = ref.float().clone()
    nan[0, 0, 0, 0] = float("nan")
    _reported(U.assert_exact, nan, ref, "nan")
    s = k.ssq(True)
    _reported(U.assert_exact, (s + torch.tensor([0.0, 0.0625, 0.0], dtype=torch.float64)).float(), s, "ssq")
