"""The target corruptions on the CPU: the test-side restatement (tests/corruption_util.py) reproduces
tests/golden/corruption.npz (made from the reference's own functions by tests/golden/make_corruption_golden.py) exactly; the
fixture's closing cases tell Jacobi sweeps from an in-place update; the command's --corruption argument."""
import pytest
import torch

from tests import corruption_util as U
from tests.test_inversion_cpu import REF_COLUMNS


@pytest.mark.parametrize("name", U.CASES)
def test_restatement_equals_reference_fixture(name):
    c = U.case(name)
    depth, mask = c["depth"], c["mask"]
    B, _, H, W = depth.shape
    for corr in U.NAMED:
        d, m = U.apply_corruption(depth, mask, corr, u=c["u"], noise=c["noise"])
        key = corr.replace(" ", "_")
        assert torch.equal(d, c[f"{key}/depth"]), (name, corr)
        assert torch.equal(m, c[f"{key}/mask"]), (name, corr)
    assert torch.equal(U.median_blur3(depth), c["median"])
    filled, sweeps, left = U.closing(depth)
    assert torch.equal(sweeps, c["sweeps"]) and int(left.sum()) == 0 and int(sweeps.min()) >= 3
    assert torch.equal(U.mask_corrupt(mask, u=c["fn/dropout_u"], rate=0.5), c["fn/dropout"])
    assert torch.equal(U.mask_corrupt(mask, row_keep=U.every(H, 1 / 2)), c["fn/hlines"])
    assert torch.equal(U.mask_corrupt(mask, col_keep=U.every(W, 1 / 4)), c["fn/vlines"])
    assert torch.equal(U.mask_corrupt(mask, row_keep=U.rows_keep(H, c["fn/rows"])), c["fn/random_lines"])
    assert torch.equal(U.mask_corrupt(mask, col_keep=U.half_keep(W)), c["fn/half"])
    assert torch.equal(U.mask_corrupt(mask, col_keep=U.quarter_keep(W)), c["fn/quarter"])


def test_fixture_tells_jacobi_from_in_place_sweeps():
    """an in-place raster update of the same holes (every pixel reading what the sweep has already written) gives another
    image than the fixture's at many pixels: the cases can fail a kernel that does not sweep in Jacobi order"""
    differ = 0
    for name in U.CASES:
        c = U.case(name)
        x = c["median"].clone()
        B, _, H, W = x.shape
        for b in range(B):
            img = x[b, 0]
            for _ in range(max(H, W)):
                if not bool((img <= U.THRESH).any()):
                    break
                for h in range(H):
                    for w in range(W):
                        if img[h, w] <= U.THRESH:
                            img[h, w] = img[max(h - 1, 0):h + 2, max(w - 1, 0):w + 2].max()
        differ += int((x != c["closing/depth"]).sum())
    assert differ >= 100, differ


def test_hole_fill_ends_on_a_scan_without_a_valid_pixel():
    """where the reference's loop never ends: no sweep counted, every pixel left, the image unchanged"""
    x = torch.zeros(2, 1, 4, 9)
    x[1, 0, 2, 3] = 0.5
    out, sweeps, left = U.hole_fill(x)
    assert sweeps.tolist() == [0, 5] and left.tolist() == [36, 0]   # (2, 3) is 5 columns from the right border
    assert torch.equal(out[0], x[0]) and bool((out[1] == 0.5).all())


def test_command_accepts_the_corruption_names():
    from dusty_gan_amd import evaluate_reconstruction as E
    from dusty_gan_amd.corruption import CORRUPTIONS
    base = ["--model-path", "m.pth", "--config-path", "c.yaml"]
    assert CORRUPTIONS == ("additive noise", "low resolution", "dropout", "closing")
    args = E.parse_args(base)
    assert args.corruption is None and args.corruption_seed == 0
    for name in CORRUPTIONS:
        assert E.parse_args(base + ["--corruption", name]).corruption == name
    assert E.parse_args(base + ["--corruption", "additive_noise"]).corruption == "additive noise"
    assert E.parse_args(base + ["--corruption", "low_resolution", "--corruption-seed", "3"]).corruption_seed == 3
    for bad in ("blur", "Dropout", ""):
        with pytest.raises(SystemExit):
            E.parse_args(base + ["--corruption", bad])
    assert E.COLUMNS == REF_COLUMNS


def test_corruptions_refuse_the_cpu():
    from dusty_gan_amd import corruption as K
    x = torch.zeros(1, 1, 4, 8)
    for fn in (K.dropout_noise, K.sparse_hlines, K.sparse_vlines, K.corrupt_half, K.corrupt_quarter, K.additive_noise,
               K.median_blur3, K.closing, lambda t: K.random_lines(t, 0.5, rows=[0])):
        with pytest.raises(RuntimeError):
            fn(x)
    assert K.apply_corruption(x, x, None) == (x, x)
    with pytest.raises(ValueError):
        K.apply_corruption(x, x, "blur")
