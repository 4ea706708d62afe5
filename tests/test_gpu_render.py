"""The picture log on the GPU (csrc/render.hip, dusty_gan_amd/utils/render.py, dusty_gan_amd/train.py).

Against the reference (tests/golden/render.npz, written by tests/golden/make_render_golden.py from its utils/render.py):
per element |out - fp64| <= 2 e_ref + 1e-6, e_ref = the reference's own max |fp32 - fp64| read from the fixture (the 2x is
the rule of test_gpu_raw_scan).  Edge shapes against the float64 restatements of tests/render_util.py, which
tests/test_render_cpu.py pins to the same fixture.  Their tolerance, from the formats: the kernel evaluates the same formulae
in double on the same float32 inputs, so what separates it from the restatement is (a) the 24.40 fixed point, at most 2^-41
per term, and (b) one rounding to float32, 2^-24 relative.
  raw splat:   |d| <= 2^-23 |v| + 4 N 2^-41                                   (4 N = every term a pixel can receive)
  normalised:  a term of the weight channel is >= 1e-3 (the corner cut) x exp(-3 x 1.2) = 2.7e-5 for the clouds here (depth
               <= 1.2 after the shift), so a pixel of T terms has a denominator >= 2.7e-5 T against an error <= 2^-41 T in
               numerator and denominator: 2 x 2^-41 / 2.7e-5 = 3.4e-8 on a ratio <= 1, plus 6e-8 of float32: 9.4e-8 -> 2e-7.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import render_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_RATIO = 2e-7


def _report(name, out, ref, bound):
    err = (out.double().cpu() - ref).abs()
    print(f"{name}: max err {float(err.max()):.3e}, bound {float(torch.as_tensor(bound).max()):.3e}")
    return err


@pytest.mark.parametrize("C", [1, 3])
def test_rasterizer_matches_the_reference(C):
    from dusty_gan_amd.utils.render import bilinear_rasterizer
    g = U.golden()
    ref = torch.from_numpy(g[f"rast/c{C}/f64"])
    out = bilinear_rasterizer(torch.from_numpy(g["rast/coords"]).to(DEV), torch.from_numpy(g[f"rast/c{C}/values"]).to(DEV),
                              ref.shape[2:])
    assert out.shape == ref.shape and out.dtype == torch.float32
    bound = 2 * float(g[f"rast/c{C}/e_ref"]) + 1e-6
    assert bool((_report(f"rasterizer C={C}", out, ref, bound) <= bound).all())


@pytest.mark.parametrize("view", ["train", "demo"])
def test_views_match_the_reference(view):
    from dusty_gan_amd.utils.render import render_point_clouds
    g = U.golden()
    xyz, normals = torch.from_numpy(g["cloud/xyz"]).to(DEV), torch.from_numpy(g["cloud/normals"]).to(DEV)
    keep = xyz.clone()
    R = torch.from_numpy(g[f"view/{view}/R"]).to(DEV) if f"view/{view}/R" in g else None
    out = render_point_clouds(xyz, normals, L=int(g["meta/L"]), R=R, t=torch.from_numpy(g[f"view/{view}/t"]).to(DEV))
    ref = torch.from_numpy(g[f"view/{view}/f64"])
    assert out.shape == ref.shape and torch.equal(xyz, keep)        # the inputs are not modified
    bound = 2 * float(g[f"view/{view}/e_ref"]) + 1e-6
    assert bool((_report(f"view {view}", out, ref, bound) <= bound).all())


def _cloud(N, seed, B=2):
    gen = torch.Generator().manual_seed(seed)
    xyz = (torch.rand(B, N, 3, generator=gen) - 0.5) * 0.8
    xyz[:, ::7] = 0.0                                                # dropped points
    return xyz, torch.rand(B, N, 3, generator=gen)


T_TRAIN = torch.tensor([0.0, 0.0, 0.5])


def test_order_freedom():
    from dusty_gan_amd.utils.render import render_point_clouds
    xyz, normals = (t.to(DEV) for t in _cloud(2049, 1))
    t = T_TRAIN.to(DEV)
    a = render_point_clouds(xyz, normals, L=37, t=t)
    b = render_point_clouds(xyz, normals, L=37, t=t)
    perm = torch.randperm(2049, generator=torch.Generator().manual_seed(2)).to(DEV)
    c = render_point_clouds(xyz[:, perm], normals[:, perm], L=37, t=t)
    assert float(a.abs().max()) > 0.1 and torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("N", [1, 63, 2049])
def test_edge_sizes_against_the_restatement(N):
    from dusty_gan_amd.utils.render import render_point_clouds
    xyz, normals = _cloud(N, 10 + N)
    if N == 1:
        xyz[:, 0] = torch.tensor([0.11, -0.07, 0.2])
    out = render_point_clouds(xyz.to(DEV), normals.to(DEV), L=37, t=T_TRAIN.to(DEV))
    ref = U.render(xyz, normals, 37, t=T_TRAIN)
    assert out.shape == (2, 3, 37, 37) and float(ref.abs().max()) > 0.01
    assert bool((_report(f"N={N}", out, ref, TOL_RATIO) <= TOL_RATIO).all())


def test_all_dropped_cloud_and_nan_point():
    from dusty_gan_amd.utils.render import render_point_clouds
    zeros, normals = torch.zeros(2, 63, 3), torch.rand(2, 63, 3, generator=torch.Generator().manual_seed(3))
    # without a shift z' = 0: the projection is 0 / 0 and the depth 0 - nothing is drawn
    assert not render_point_clouds(zeros.to(DEV), normals.to(DEV), L=37).any()
    # with the training view every point lands on the centre: L / 2, an exact integer coordinate for even L (one cell per
    # sample), the middle of four cells for odd L
    for size, cells in ((64, 1), (37, 4)):
        out = render_point_clouds(zeros.to(DEV), normals.to(DEV), L=size, t=T_TRAIN.to(DEV))
        ref = U.render(zeros, normals, size, t=T_TRAIN)
        assert int((ref.abs().sum(1) > 0).sum()) == 2 * cells and bool(((out.double().cpu() - ref).abs() <= TOL_RATIO).all())
    # one NaN point is skipped and the rest is unchanged, bit for bit
    xyz, normals = _cloud(63, 4)
    t = T_TRAIN.to(DEV)
    clean = render_point_clouds(torch.cat([xyz[:, :5], xyz[:, 6:]], 1).to(DEV), torch.cat([normals[:, :5], normals[:, 6:]], 1).to(DEV),
                                L=37, t=t)
    xyz[:, 5, 1] = float("nan")
    assert torch.equal(render_point_clouds(xyz.to(DEV), normals.to(DEV), L=37, t=t), clean) and float(clean.abs().max()) > 0.01


def test_integer_and_outside_coordinates():
    from dusty_gan_amd.utils.render import bilinear_rasterizer
    H, W = 9, 13
    coords = torch.tensor([[[5.0, 7.0],            # on a cell: the far corners carry zero weight
                            [-0.5, 3.25],          # above the image: only the clamped row 0 takes weight
                            [H - 1 + 0.4, 2.5],    # below the last row: only row H-1
                            [2.5, -0.75],          # left of the image: only column 0
                            [3.5, W - 1 + 0.5],    # right of the last column
                            [-2.0, 4.0], [4.0, W + 1.5], [1e30, 1.0],   # out of reach: nothing
                            [float("inf"), 2.0], [3.0, float("nan")]]])  # non-finite: skipped
    values = torch.arange(1, 11, dtype=torch.float32).view(1, 10, 1) / 8
    out = bilinear_rasterizer(coords.to(DEV), values.to(DEV), (H, W)).double().cpu()
    ref = U.splat(coords, values, H, W)
    assert bool(((out - ref).abs() <= 2.0 ** -23 * ref.abs() + 40 * 2.0 ** -41).all())
    assert float(out[0, 0, 5, 7]) == 0.125 and not out[0, 0, 6, 7] and not out[0, 0, 5, 8] and not out[0, 0, 6, 8]
    lit = {(int(r), int(c)) for r, c in torch.nonzero(out[0, 0])}
    assert lit == {(5, 7), (0, 3), (0, 4), (H - 1, 2), (H - 1, 3), (2, 0), (3, 0), (3, W - 1), (4, W - 1)}
    with pytest.raises(RuntimeError):
        bilinear_rasterizer(coords, values, (H, W))                  # CPU tensors raise


@pytest.mark.parametrize("case", ["colour", "plain1", "plain3", "colour3"])
def test_image_grid_bytes(case):
    from dusty_gan_amd.utils.render import grid_shape, image_grid, turbo_lut
    lut = turbo_lut().numpy()
    rng = np.random.default_rng(7)
    C = 3 if case.endswith("3") else 1
    x = rng.uniform(-0.3, 1.3, (5, C, 6, 7)).astype(np.float32)
    x[0, 0, 0, :4] = [np.nan, -1.0, 0.4, 7.0]
    x[1, 0, 1, :3] = [1.0 / 2.5, 255.0 / 256 / 2.5, 0.0]             # the table's last index and its edge at scale 2.5
    color, scale = case.startswith("colour"), 2.5 if case == "colour" else 1.0
    out = image_grid(torch.from_numpy(x).to(DEV), color=color, scale=scale)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2 * 8 + 2, 4 * 9 + 2, 3) == grid_shape(5, 6, 7) + (3,)
    want = U.grid_bytes(x, color, scale, lut)
    assert np.array_equal(out.cpu().numpy(), want)
    pad = [int(v) for v in out[0, 0]]
    assert pad == ([int(np.float32(v) * np.float32(255)) for v in lut[0]] if color else [0, 0, 0])
    if case == "plain1":   # a channel slice of a wider tensor is read in place
        wide = torch.from_numpy(np.concatenate([x, x + 1], 1)).to(DEV)
        assert torch.equal(image_grid(wide[:, 0:1], color=False), out)
        assert tuple(image_grid(wide[:3, 0:1], color=False).shape) == (1 * 8 + 2, 3 * 9 + 2, 3)


def test_colorize_against_the_table():
    from dusty_gan_amd.utils.render import colorize, turbo_lut
    lut = turbo_lut().numpy()                                        # (tests/test_render_cpu.py holds it against matplotlib)
    rng = np.random.default_rng(11)
    x = rng.uniform(-0.2, 1.2, (3, 1, 5, 9)).astype(np.float32)
    x[0, 0, 0, :4] = [0.0, 1.0, 0.5 / 255, 254.5 / 255]             # the ends and round's half-way cases
    t = torch.from_numpy(x).to(DEV)
    keep = t.clone()
    want = lut[np.round(np.clip(x[:, 0], 0, 1) * np.float32(255)).astype(np.int64)].transpose(0, 3, 1, 2)   # utils.colorize
    for arg in (t, t[:, 0]):                                         # [B,1,H,W] and [B,H,W]
        out = colorize(arg)
        assert out.shape == (3, 3, 5, 9) and out.dtype == torch.float32 and np.array_equal(out.cpu().numpy(), want)
    assert torch.equal(t, keep) and torch.equal(colorize(t), colorize(t))   # (the second call reads the cached device table)
    with pytest.raises(RuntimeError):
        colorize(torch.from_numpy(x))


def test_value_window_streams_and_a_clean_workspace_after_errors():
    from dusty_gan_amd._lib import DgError
    from dusty_gan_amd.utils.render import bilinear_rasterizer, render_point_clouds
    xyz, normals = (t.to(DEV) for t in _cloud(63, 5))
    t = T_TRAIN.to(DEV)
    first = render_point_clouds(xyz, normals, L=37, t=t)
    coords = torch.tensor([[[2.5, 3.5], [4.25, 1.5]]], device=DEV)
    ok = bilinear_rasterizer(coords, torch.tensor([[[8.0], [-8.0]]], device=DEV), (9, 13))
    assert float(ok[0, 0, 2, 3]) == 2.0 and float(ok[0, 0, 4, 1]) == -3.0     # the window's edge is inside
    for bad in (8.5, -1e30, float("inf")):                           # beyond it: refused, not wrapped or dropped
        with pytest.raises(ValueError):
            bilinear_rasterizer(coords, torch.tensor([[[1.0], [bad]]], device=DEV), (9, 13))
    with pytest.raises(ValueError):
        render_point_clouds(xyz, normals * 100, L=37, t=t)
    with pytest.raises(DgError):                                     # more points than the range analysis allows
        render_point_clouds(torch.zeros(1, (1 << 18) + 1, 3, device=DEV), torch.zeros(1, (1 << 18) + 1, 3, device=DEV), L=37, t=t)
    assert torch.equal(render_point_clouds(xyz, normals, L=37, t=t), first)   # the words were left zero
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                    # a stream has words of its own
        other = render_point_clouds(xyz, normals, L=37, t=t)
    side.synchronize()
    assert torch.equal(other, first)


ARGS = ["model=dusty2_dcgan_eqlr", "dataset=synthetic", "dataset.shape=[32,64]", "model.gen.in_ch=16", "model.gen.ch_base=8",
        "model.gen.ch_max=32", "model.dis.ch_base=8", "model.dis.ch_max=32", "solver.batch_size=4", "enable_amp=false",
        "dataset.pool=2", "solver.checkpoint.save_stats=1", "solver.checkpoint.save_image=2", "solver.checkpoint.test=3",
        "solver.checkpoint.save_model=4", "solver.validation.num_points=256"]
LOSS_KEYS = {"loss/D/output/real", "loss/D/output/fake", "loss/D/adversarial", "loss/D/gradient_penalty", "loss/G/adversarial"}


def test_train_command_in_process(tmp_path):
    from PIL import Image

    from dusty_gan_amd import train as T
    from dusty_gan_amd import utils
    run = T.main(ARGS + ["solver.total_kimg=0.024", "--out-dir", str(tmp_path / "run")])
    out = str(tmp_path / "run")
    assert run["out_dir"] == out and run["start_iteration"] == 1 and run["total_iteration"] == 6
    lines = [json.loads(ln) for ln in open(os.path.join(out, "scalars.jsonl"))]
    assert [ln["iteration"] for ln in lines] == [1, 2, 3, 4, 5, 6] and [ln["step"] for ln in lines] == [4, 8, 12, 16, 20, 24]
    for ln in lines:
        assert LOSS_KEYS <= set(ln) and all(np.isfinite(ln[k]) for k in LOSS_KEYS)
        scores = {k for k in ln if k.startswith("score/")}
        assert bool(scores) == (ln["iteration"] % 3 == 0)
        if scores:
            assert {"score/jsd", "score/mmd-cd", "score/cov-cd", "score/1-nn-accuracy-cd"} <= scores
            assert any(k.startswith("score/swd") for k in scores)
    synth = ["synth/inv", "synth/normal", "synth/bev", "synth/inv/orig", "synth/confidence/pix", "synth/confidence/img",
             "synth/mask/pix", "synth/mask/img", "synth/mask"]
    for tag, steps in [(t, [1]) for t in T.REAL_TAGS] + [(t, [8, 16, 24]) for t in synth]:
        d = os.path.join(out, "images", tag)
        assert sorted(f for f in os.listdir(d) if f.endswith(".png")) == ["{:010d}.png".format(s) for s in steps], tag
        with Image.open(os.path.join(d, "{:010d}.png".format(steps[0]))) as im:
            want = (4 * 514 + 2, 514 + 2) if tag.endswith("bev") else (4 * 66 + 2, 34 + 2)
            assert im.size == want and im.mode == "RGB", (tag, im.size)
    with Image.open(os.path.join(out, "images", "synth/bev", "0000000024.png")) as im:
        assert np.asarray(im).max() > 0                              # something was drawn
    ckpts = sorted(os.listdir(os.path.join(out, "models")))
    assert ckpts == ["checkpoint_0000000016.pth", "checkpoint_0000000024.pth"] and run["checkpoint"].endswith(ckpts[-1])
    # the run directory feeds the evaluation command's loader
    cfg, G, lidar, device = utils.setup(run["checkpoint"], os.path.join(out, ".hydra", "config.yaml"))
    assert list(cfg.dataset.shape) == [32, 64] and cfg.solver.batch_size == 4 and lidar.angle is not None
    # a later invocation with resume= continues behind the last finished iteration
    run2 = T.main(ARGS + ["solver.total_kimg=0.032", "resume=" + run["checkpoint"], "--out-dir", str(tmp_path / "run2")])
    assert run2["start_iteration"] == 7 and run2["total_iteration"] == 8
    lines2 = [json.loads(ln) for ln in open(os.path.join(str(tmp_path / "run2"), "scalars.jsonl"))]
    assert [ln["iteration"] for ln in lines2] == [7, 8]
    assert os.path.exists(os.path.join(str(tmp_path / "run2"), "models", "checkpoint_0000000032.pth"))
