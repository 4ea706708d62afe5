"""CPU-side checks of the picture log (no GPU): the turbo table compiled into the library, the float64 restatements of
tests/render_util.py against the reference's own outputs (tests/golden/render.npz), and the training command's argument
parsing and run-directory layout."""
import os

import numpy as np
import pytest
import torch

from tests import render_util as U


def test_turbo_table_is_matplotlibs():
    cm = pytest.importorskip("matplotlib.cm")
    from dusty_gan_amd import _lib
    from dusty_gan_amd.utils.render import turbo_lut
    _lib.build()
    lut = turbo_lut().numpy()
    want = cm.turbo(np.linspace(0, 1, 256))[:, :3]
    assert lut.shape == (256, 3) and np.abs(lut.astype(np.float64) - want).max() <= 1e-7
    # the image-log rules of render_util.grid_bytes ARE the reference's chain: make_grid's padded layout, then
    # matplotlib's Normalize + ScalarMappable on channel 0, then TensorBoard's (x * 255).clip(0, 255).astype(uint8)
    import matplotlib
    rng = np.random.default_rng(5)
    x = rng.uniform(-0.2, 1.2, (5, 1, 6, 7)).astype(np.float32)
    x[1, 0, 2, 3] = np.nan
    got = U.grid_bytes(x, True, 2.5, lut)
    grid = np.zeros((2 * 8 + 2, 4 * 9 + 2), dtype=np.float32)
    for k in range(5):
        grid[(k // 4) * 8 + 2:(k // 4) * 8 + 8, (k % 4) * 9 + 2:(k % 4) * 9 + 9] = x[k, 0] * np.float32(2.5)
    mapper = cm.ScalarMappable(norm=matplotlib.colors.Normalize(vmin=0.0, vmax=1.0), cmap="turbo")
    rgb = mapper.to_rgba(grid)[..., :3]
    assert np.array_equal(got, (rgb * 255).clip(0, 255).astype(np.uint8))


@pytest.mark.parametrize("view", ["train", "demo"])
def test_render_restatement_matches_the_reference(view):
    g = U.golden()
    R = torch.from_numpy(g[f"view/{view}/R"]) if f"view/{view}/R" in g else None
    out = U.render(torch.from_numpy(g["cloud/xyz"]), torch.from_numpy(g["cloud/normals"]), int(g["meta/L"]), R=R,
                   t=torch.from_numpy(g[f"view/{view}/t"]))
    ref = torch.from_numpy(g[f"view/{view}/f64"])
    assert out.shape == ref.shape and float(ref.abs().max()) > 0.1
    assert float((out - ref).abs().max()) <= 1e-12       # float64 against float64: summation order only


@pytest.mark.parametrize("C", [1, 3])
def test_splat_restatement_matches_the_reference(C):
    g = U.golden()
    ref = torch.from_numpy(g[f"rast/c{C}/f64"])
    out = U.splat(torch.from_numpy(g["rast/coords"]), torch.from_numpy(g[f"rast/c{C}/values"]), ref.shape[2], ref.shape[3])
    assert out.shape == ref.shape and float((out - ref).abs().max()) <= 1e-12


def test_fixture_records_the_references_own_error():
    g = U.golden()
    for k in ("view/train/e_ref", "view/demo/e_ref", "rast/c1/e_ref", "rast/c3/e_ref"):
        assert 0.0 < float(g[k]) < 1e-3, k
    assert os.path.getsize(U.GOLDEN) < 1 << 20


def test_train_command_arguments_and_layout(tmp_path, monkeypatch):
    import datetime

    from dusty_gan_amd import train as T
    from dusty_gan_amd.utils.config import load_config_file
    args = T.parse_args(["dataset=synthetic", "model=dusty2_dcgan_eqlr", "solver.batch_size=8", "--out-dir", str(tmp_path / "run")])
    assert args.overrides == ["dataset=synthetic", "model=dusty2_dcgan_eqlr", "solver.batch_size=8"]
    assert args.out_dir == str(tmp_path / "run")
    assert T.parse_args([]).out_dir is None and T.parse_args([]).overrides == []
    with pytest.raises(SystemExit):
        T.parse_args(["solver.batch_size"])
    assert T.default_out_dir(datetime.datetime(2026, 1, 2, 3, 4, 5)) == os.path.join("outputs", "2026-01-02", "03-04-05")
    # relative paths are the invoking directory's (train.py:179-182); absolute ones and a null resume stay
    monkeypatch.chdir(tmp_path)
    cfg = T.compose(["dataset=kitti_odometry", "dataset.root=data/kitti", "resume=models/checkpoint_0000000024.pth"])
    assert cfg.dataset.root == os.path.join(str(tmp_path), "data/kitti")
    assert cfg.resume == os.path.join(str(tmp_path), "models/checkpoint_0000000024.pth")
    cfg = T.compose(["dataset=synthetic", "dataset.root=/abs/x", "solver.batch_size=8", "solver.num_accumulation=2"])
    assert cfg.dataset.root == "/abs/x" and cfg.resume is None
    assert T.local_config(cfg, 1, 2) == {"gpu": 1, "ngpus": 2, "batch_size": 2, "num_workers": 4}
    out = T.prepare_out_dir(cfg, "run2")
    assert out == str(tmp_path / "run2") and sorted(os.listdir(out)) == [".hydra", "images", "models"]
    back = load_config_file(os.path.join(out, ".hydra", "config.yaml"))
    assert back.solver.batch_size == 8 and back.dataset.name == "synthetic" and list(back.model.gen.out_ch) == list(cfg.model.gen.out_ch)
    # the reference's tags for a dusty2 result (train.py:125-151)
    fake = {"depth": torch.zeros(1, 1, 2, 2), "depth_orig": 0, "confidence": torch.zeros(1, 2, 2, 2), "mask": torch.zeros(1, 2, 2, 2)}
    assert [t[0] for t in T.image_tags(fake)] == ["synth/inv", "synth/normal", "synth/bev", "synth/inv/orig", "synth/confidence/pix",
                                                  "synth/confidence/img", "synth/mask/pix", "synth/mask/img", "synth/mask"]
    assert [t[0] for t in T.image_tags({"depth": 0, "mask": torch.zeros(1, 1, 2, 2)})] == ["synth/inv", "synth/normal", "synth/bev",
                                                                                            "synth/mask"]
