"""The target corruptions on the MI355X (csrc/corrupt.hip: dg_corrupt_mask, dg_additive_noise, dg_median3x3, dg_hole_fill;
dusty_gan_amd/corruption.py) against tests/golden/corruption.npz - the reference's own functions, demo.py:71-137 - and, where
a golden would be too large, against the restatement tests/test_corruption_cpu.py holds to it.  Every operation is a
selection, a maximum, a product with 0 / 1 or two correctly rounded fp32 operations: torch.equal, no tolerance.  The only
bounds are the two statistical ones on the device's own draws."""
import csv
import math

import numpy as np
import pytest
import torch

from tests import corruption_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _abi_mask(mask, row_keep=None, col_keep=None, u=None, rate=1.0, in_place=False):
    from dusty_gan_amd import _lib as L
    m = mask.to(DEV).contiguous()
    B, _, H, W = m.shape
    rk, ck, ud = (None if t is None else t.to(DEV).float().contiguous() for t in (row_keep, col_keep, u))
    out = m if in_place else torch.empty_like(m)
    L.check(L.lib().dg_corrupt_mask(L.ptr(m), L.ptr(rk), L.ptr(ck), L.ptr(ud), rate, B, H, W, L.ptr(out), L.stream_ptr()),
            "dg_corrupt_mask")
    return out.cpu()


def _abi_noise(x, noise, strength, in_place=False):
    from dusty_gan_amd import _lib as L
    xd, nd = x.to(DEV).contiguous(), noise.to(DEV).contiguous()
    out = xd if in_place else torch.empty_like(xd)
    L.check(L.lib().dg_additive_noise(L.ptr(xd), L.ptr(nd), strength, xd.numel(), L.ptr(out), L.stream_ptr()), "dg_additive_noise")
    return out.cpu()


def _abi_median(x):
    from dusty_gan_amd import _lib as L
    xd = x.to(DEV).contiguous()
    B, _, H, W = xd.shape
    out = torch.empty_like(xd)
    L.check(L.lib().dg_median3x3(L.ptr(xd), B, H, W, L.ptr(out), L.stream_ptr()), "dg_median3x3")
    return out.cpu()


def _abi_fill(x, thresh=U.THRESH):
    from dusty_gan_amd import _lib as L
    xd = x.to(DEV).contiguous().clone()
    B, _, H, W = xd.shape
    tmp = torch.empty_like(xd)
    sweeps = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    left = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    L.check(L.lib().dg_hole_fill(L.ptr(xd), L.ptr(tmp), B, H, W, thresh, L.ptr(sweeps), L.ptr(left), L.stream_ptr()), "dg_hole_fill")
    return xd.cpu(), sweeps.cpu(), left.cpu()


@pytest.mark.parametrize("name", U.CASES)
def test_c_abi_equals_reference_fixture(name):
    c = U.case(name)
    depth, mask = c["depth"], c["mask"]
    B, _, H, W = depth.shape
    assert torch.equal(_abi_noise(depth, c["noise"], 0.01), c["additive_noise/depth"])
    assert torch.equal(_abi_mask(mask, row_keep=U.every(H, 1 / 8)), c["low_resolution/mask"])
    assert torch.equal(_abi_mask(mask, u=c["u"], rate=0.1), c["dropout/mask"])
    med = _abi_median(depth)
    assert torch.equal(med, c["median"])
    filled, sweeps, left = _abi_fill(med)
    assert torch.equal(filled, c["closing/depth"])
    assert torch.equal(sweeps, c["sweeps"]) and left.tolist() == [0] * B
    assert torch.equal(_abi_mask(mask, u=c["fn/dropout_u"], rate=0.5), c["fn/dropout"])
    assert torch.equal(_abi_mask(mask, row_keep=U.every(H, 1 / 2)), c["fn/hlines"])
    assert torch.equal(_abi_mask(mask, col_keep=U.every(W, 1 / 4)), c["fn/vlines"])
    assert torch.equal(_abi_mask(mask, row_keep=U.rows_keep(H, c["fn/rows"])), c["fn/random_lines"])
    assert torch.equal(_abi_mask(mask, col_keep=U.half_keep(W)), c["fn/half"])
    assert torch.equal(_abi_mask(mask, col_keep=U.quarter_keep(W)), c["fn/quarter"])
    # all three factors in one launch
    both = _abi_mask(mask, row_keep=U.every(H, 1 / 2), col_keep=U.every(W, 1 / 4), u=c["u"], rate=0.5)
    assert torch.equal(both, U.mask_corrupt(mask, U.every(H, 1 / 2), U.every(W, 1 / 4), c["u"], 0.5))
    # in place equals out of place
    assert torch.equal(_abi_mask(mask, u=c["u"], rate=0.1, in_place=True), c["dropout/mask"])
    assert torch.equal(_abi_noise(depth, c["noise"], 0.01, in_place=True), c["additive_noise/depth"])


@pytest.mark.parametrize("name", U.CASES)
def test_python_api_equals_reference_fixture(name):
    from dusty_gan_amd import corruption as K
    c = U.case(name)
    depth, mask = c["depth"].to(DEV), c["mask"].to(DEV)
    d0, m0 = depth.clone(), mask.clone()
    for corr in K.CORRUPTIONS:
        d, m = K.apply_corruption(depth, mask, corr, u=c["u"], noise=c["noise"])
        key = corr.replace(" ", "_")
        assert torch.equal(d.cpu(), c[f"{key}/depth"]), (name, corr)
        assert torch.equal(m.cpu(), c[f"{key}/mask"]), (name, corr)
        assert torch.equal(depth, d0) and torch.equal(mask, m0), (name, corr, "an input was modified")
    d, m = K.apply_corruption(depth, mask, None)
    assert d is depth and m is mask
    assert torch.equal(K.apply_corruption(depth, mask, "additive_noise", noise=c["noise"])[0].cpu(), c["additive_noise/depth"])
    assert torch.equal(K.median_blur3(depth).cpu(), c["median"])
    filled, info = K.closing(depth, return_info=True)
    assert torch.equal(filled.cpu(), c["closing/depth"]) and torch.equal(info["sweeps"].cpu(), c["sweeps"])
    assert int(info["left"].sum()) == 0
    assert torch.equal(K.dropout_noise(mask, 0.5, u=c["fn/dropout_u"]).cpu(), c["fn/dropout"])
    assert torch.equal(K.sparse_hlines(mask, 1 / 2).cpu(), c["fn/hlines"])
    assert torch.equal(K.sparse_vlines(mask, 1 / 4).cpu(), c["fn/vlines"])
    assert torch.equal(K.random_lines(mask, 0.5, rows=c["fn/rows"]).cpu(), c["fn/random_lines"])
    assert torch.equal(K.corrupt_half(mask).cpu(), c["fn/half"])
    assert torch.equal(K.corrupt_quarter(mask).cpu(), c["fn/quarter"])
    assert torch.equal(depth, d0) and torch.equal(mask, m0)
    # random_lines' own rows: int(H (1 - rate)) distinct rows, the same for a seed, zeroed in every sample
    H = mask.shape[2]
    rows = K.random_rows(H, 0.5, seed=3)
    assert len(set(rows.tolist())) == int(H * 0.5) == len(rows) and torch.equal(rows, K.random_rows(H, 0.5, seed=3))
    assert torch.equal(K.random_lines(mask, 0.5, seed=3), K.random_lines(mask, 0.5, rows=rows))


def test_closing_full_width_equals_restatement():
    """[2,64,1024]: 64 pixels per thread at the full workgroup width; validity 0.85 and a 44 x 160 hole at the top border, which
    fills from below only: 44 sweeps that change something (the reference's loop makes a 45th, which changes nothing)"""
    from dusty_gan_amd import corruption as K
    depth, _ = U.scan_like(2, 64, 1024, 0.85, (44, 160), seed=7, at=(0, 300))
    want, sweeps, left = U.closing(depth)
    got, info = K.closing(depth.to(DEV), return_info=True)
    print("full-width closing sweeps:", info["sweeps"].tolist(), "restatement:", sweeps.tolist())
    assert left.tolist() == [0, 0] and sweeps.tolist() == [44, 44]
    assert torch.equal(info["sweeps"].cpu(), sweeps) and info["left"].tolist() == [0, 0]
    assert torch.equal(got.cpu(), want)


def test_hole_fill_batch_with_a_scan_without_a_valid_pixel():
    """the first sample equals its B = 1 result; the all-zero one - where the reference's loop never ends - comes back
    unchanged with left = H W"""
    c = U.case("c1")
    H, W = c["median"].shape[2:]
    x = torch.cat([c["median"], torch.zeros(1, 1, H, W)])
    got, sweeps, left = _abi_fill(x)
    one, s1, l1 = _abi_fill(c["median"])
    assert torch.equal(got[:1], one) and torch.equal(one, c["closing/depth"])
    assert sweeps.tolist() == [int(s1), 0] and left.tolist() == [0, H * W]
    assert torch.equal(got[1], x[1])
    # an odd and an even number of kept sweeps both end in x: one valid pixel, 1 and 2 columns from the farthest
    for W2, n in ((2, 1), (3, 2)):
        y = torch.zeros(1, 1, 1, W2)
        y[..., 0] = 0.25
        got, sweeps, left = _abi_fill(y)
        assert bool((got == 0.25).all()) and sweeps.tolist() == [n] and left.tolist() == [0]
    got, sweeps, left = _abi_fill(torch.zeros(1, 1, 1, 1))
    assert got.item() == 0.0 and sweeps.tolist() == [0] and left.tolist() == [1]


def test_hole_fill_refuses_more_than_2_18_pixels():
    from dusty_gan_amd import _lib as L
    x = torch.zeros(1, 1, 513, 512, device=DEV)
    tmp = torch.empty_like(x)
    cnt = torch.zeros(2, dtype=torch.int32, device=DEV)
    rc = L.lib().dg_hole_fill(L.ptr(x), L.ptr(tmp), 1, 513, 512, 1e-8, L.ptr(cnt[:1]), L.ptr(cnt[1:]), L.stream_ptr())
    assert rc == L.DG_EUNSUPPORTED
    from dusty_gan_amd import corruption as K
    with pytest.raises(ValueError):
        K.closing(x)


@pytest.mark.parametrize("shape", [(3, 5, 37), (3, 16, 160)])
def test_draws_are_keyed_by_the_scan_index(shape):
    """a batch of three with first_index 5 equals three single scans with first_index 5, 6, 7; another seed differs"""
    from dusty_gan_amd import corruption as K
    B, H, W = shape
    depth, mask = U.scan_like(B, H, W, 0.8, (3, 5), seed=11)
    depth, mask = depth.to(DEV), torch.ones_like(mask).to(DEV)
    for corr, pick in (("dropout", 1), ("additive noise", 0)):
        whole = K.apply_corruption(depth, mask, corr, seed=2, first_index=5)[pick]
        for b in range(B):
            single = K.apply_corruption(depth[b:b + 1], mask[b:b + 1], corr, seed=2, first_index=5 + b)[pick]
            assert torch.equal(whole[b:b + 1], single), (corr, b)
        assert not torch.equal(whole[0], whole[1])
        other = K.apply_corruption(depth, mask, corr, seed=3, first_index=5)[pick]
        assert not torch.equal(whole, other), corr


def test_device_draws_have_the_right_statistics():
    """64 x 1024.  Dropout keeps a share of the valid pixels within 5 binomial standard deviations of 0.1; (out - in) / 0.01 of
    the additive noise has mean within 5 / sqrt(n) of 0 and standard deviation within 5 / sqrt(2 n) of 1"""
    from dusty_gan_amd import corruption as K
    depth, mask = U.scan_like(1, 64, 1024, 0.85, (8, 32), seed=5)
    d, m = depth.to(DEV), mask.to(DEV)
    _, kept = K.apply_corruption(d, m, "dropout")
    assert bool(((kept == 0) | (kept == 1)).all()) and bool((kept <= m).all())
    nv = float(mask.sum())
    share = float(kept.sum()) / nv
    print("dropout keeps", share, "of", nv)
    assert abs(share - 0.1) <= 5 * math.sqrt(0.1 * 0.9 / nv)
    noisy, same = K.apply_corruption(d, m, "additive noise")
    assert same is m
    z = (noisy.double() - d.double()).flatten().cpu() / 0.01
    n = z.numel()
    print("additive noise mean", float(z.mean()), "std", float(z.std()))
    assert abs(float(z.mean())) <= 5 / math.sqrt(n) and abs(float(z.std()) - 1) <= 5 / math.sqrt(2 * n)


@pytest.fixture(scope="module")
def evaluation(tmp_path_factory):
    """the recipe of tests/test_gpu_inversion.py::test_evaluate_reconstruction_end_to_end - a synthetic full-width dusty2 bf16
    checkpoint, three .npy test scans, batch 2, 20 steps - and its rows without a corruption"""
    from dusty_gan_amd import evaluate_reconstruction as E
    from dusty_gan_amd.models import define_G
    from dusty_gan_amd.utils.config import dump_config, load_config
    from tests.test_gpu_data import write_kitti_tree
    tmp = tmp_path_factory.mktemp("corruption_eval")
    root = str(tmp / "kitti")
    write_kitti_tree(root, 64, 2048, {11: 3})
    cfg = load_config(["model=dusty2_dcgan_eqlr", "dataset=kitti_odometry", f"dataset.root={root}",
                       "dataset.shape=[64,1024]", "enable_amp=true"])
    cfg_path, ckpt = str(tmp / "config.yaml"), str(tmp / "model.pth")
    dump_config(cfg, cfg_path)
    torch.manual_seed(0)
    cfg.model.gen.shape = cfg.dataset.shape
    torch.save({"step": 0, "G_ema": define_G(cfg).state_dict()}, ckpt)

    def run(*extra):
        path = E.main(["--model-path", ckpt, "--config-path", cfg_path, "--save-dir-path", str(tmp / "out"), "--batch-size", "2",
                       "--num-step", "20", *extra])
        return list(csv.reader(open(path)))
    return run, run()


@pytest.mark.parametrize("name", ["closing", "dropout"])
def test_evaluate_reconstruction_with_a_corruption(evaluation, name):
    """finite rows in the reference's columns; drop_ref - a property of the FULL scan's mask - equals the uncorrupted run's
    row for row, while the inversion, run against the corrupted target, gives other depth errors"""
    from dusty_gan_amd import evaluate_reconstruction as E
    run, plain = evaluation
    rows = run("--corruption", name)
    assert rows[0] == [""] + E.COLUMNS == plain[0] and len(rows) == 4 == len(plain)
    vals = np.array([[float(v) for v in r[1:]] for r in rows[1:]])
    assert np.isfinite(vals).all(), vals
    at = 1 + E.COLUMNS.index("drop_ref")
    assert [r[at] for r in rows[1:]] == [r[at] for r in plain[1:]]
    assert 0.0 < float(rows[1][at]) < 1.0
    rmse = 1 + E.COLUMNS.index("rmse")
    assert [r[rmse] for r in rows[1:]] != [r[rmse] for r in plain[1:]]
