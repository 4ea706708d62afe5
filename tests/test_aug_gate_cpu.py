"""The float64 restatement of DiffAugment(policy, p < 1) (tests/aug_gate_ref.py) held to what the reference's own module computed
(tests/golden/aug_gate_*.npz, written by tests/golden/make_aug_gate_golden.py): forward and autograd input gradient for
p in {0, 0.3, 0.7, 1}, the full policy and `translation,cutout` alone, 8x16 and 32x64, B = 64.  <= 1e-6 absolute (the fixture is the
module's fp32 arithmetic on images in [-1, 1], results below 4: a few roundings of at most 1.2e-7 each), exact where the reference
only moves values.  No GPU."""
import numpy as np
import pytest
import torch

from tests import aug_gate_ref as R
from tests.golden_util import load

PS = (0.0, 0.3, 0.7, 1.0)
TAGS = ("full", "tc")
SHAPES = ((8, 16), (32, 64))
TOL = 1e-6


def case(H, W, tag, i):
    """(x, gy, y, gx float64, rp, policy, p) of one recorded case"""
    if (H, W) == (8, 16):
        g, pre = load("aug_gate_8x16"), f"{tag}/p{i}/"
    else:
        g, pre = load(f"aug_gate_{H}x{W}_{tag}_p{i}"), ""
    t = lambda k: torch.from_numpy(np.array(g[pre + k]))
    rp = {k[len(pre) + 3:]: torch.from_numpy(np.array(g[k])) for k in g.files if k.startswith(pre + "rp/")}
    rp = {k: (v.double() if k.startswith("u_") else v.long()) for k, v in rp.items()}
    return t("x").double(), t("gy").double(), t("y").double(), t("gx").double(), rp, tuple(str(g[pre + "policy"]).split(",")), float(g[pre + "p"])


CASES = [(H, W, tag, i) for H, W in SHAPES for tag in TAGS for i in range(len(PS))]


@pytest.mark.parametrize("H,W,tag,i", CASES, ids=[f"{H}x{W}-{tag}-p{PS[i]}" for H, W, tag, i in CASES])
def test_restatement_meets_the_reference(H, W, tag, i):
    x, gy, y, gx, rp, policy, p = case(H, W, tag, i)
    assert p == PS[i] and x.shape == (64, 1, H, W)
    st = torch.bincount(R.gate_state(rp), minlength=4).tolist()
    if p in (0.3, 0.7):
        assert min(st) >= 2, st                 # the generator's condition: every gate state at least twice
    elif p == 0.0:
        assert st == [64, 0, 0, 0]
    else:
        assert st == [0, 0, 0, 64]
    for name, got, want in (("fwd", R.fwd(x, rp, policy), y), ("fwd oracle", R.fwd_oracle(x, rp, policy), y),
                            ("adj", R.adj(gy, rp, policy), gx), ("adj oracle", R.adj_oracle(gy, rp, policy), gx)):
        err = float((got - want).abs().max())
        print(f"[aug-gate] {H}x{W} {tag} p={p} {name}: max |err| = {err:.3g}, states {st}")
        if tag == "tc":
            assert torch.equal(got, want), (name, err)
        else:
            assert err <= TOL, (name, err)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_each_defect_is_rejected_by_the_fixture(defect):
    """forward and adjoint, at p = 0.3 and 0.7 on 8x16, miss the fixture by far more than the bound under each defect"""
    for i in (1, 2):
        x, gy, y, gx, rp, policy, p = case(8, 16, "full", i)
        ef = float((R.fwd(x, rp, policy, defect) - y).abs().max())
        ea = float((R.adj(gy, rp, policy, defect) - gx).abs().max())
        print(f"[aug-gate] defect {defect} p={p}: forward {ef:.3g}, adjoint {ea:.3g}")
        assert ef > 1e-3 and ea > 1e-3, (defect, p, ef, ea)


def test_the_colour_stages_do_not_depend_on_p():
    """the reference's brightness / contrast factors are u * u at every p - p = 0 included, where translation and cutout are off for
    every sample: A(x) is then the colour stages alone, with the factor of the recorded uniform draw"""
    for H, W in SHAPES:
        for i, p in enumerate(PS):
            x, gy, y, gx, rp, policy, _ = case(H, W, "full", i)
            on = R.gate_state(rp) == 0            # neither stage: what is left is colour
            if not bool(on.any()):
                continue
            ub, uc = rp["u_b"][on].view(-1, 1, 1, 1), rp["u_c"][on].view(-1, 1, 1, 1)
            v = x[on] + 0.5 * ub * ub
            m = v.mean(dim=[1, 2, 3], keepdim=True)
            want = m + (1 + 0.5 * uc * uc) * (v - m)
            assert float((y[on] - want).abs().max()) <= TOL
            assert float((want - x[on]).abs().max()) > 1e-3      # ... and they are not the identity
    # p = 0 with the colour stages out of the policy: the exact identity, forward and adjoint
    x, gy, y, gx, rp, policy, p = case(8, 16, "tc", 0)
    assert torch.equal(y, x) and torch.equal(gx, gy)


def test_window_sum_follows_the_gates():
    """the contrast pivot's gradient: sum of the upstream over the pixels that come from the source - the whole image where both
    stages are off; the adjoint of the restatement uses it (checked against the fixture above)"""
    x, gy, y, gx, rp, policy, p = case(8, 16, "full", 1)
    ws = R.window_sum(gy, rp, policy)
    off = R.gate_state(rp) == 0
    assert torch.equal(ws[off], gy[off].sum(dim=[1, 2, 3]))
    both = R.gate_state(rp) == 3
    assert not torch.equal(ws[both], gy[both].sum(dim=[1, 2, 3]))


def test_interleaved_batch_mixes_the_states():
    from tests import image_exact_util as U
    rp = R.interleaved(U.with_factors(U.all_draws(8, 16)))
    st = R.gate_state(rp)
    assert st.shape[0] == 4 * 1377 and torch.bincount(st).tolist() == [1377] * 4
    assert bool((st[1:] != st[:-1]).all())
