"""The synthesis command without a GPU (dusty_gan_amd/synthesis.py, dusty_gan_amd/synthesize.py): the float64
restatements of tests/synthesis_util.py against hand-computed cases and against what the reference's own utils/interp.py
and utils/geometry.py produced (tests/golden/synthesis.npz), view(), argument parsing, file naming, the .bin writer and
the header's declarations."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import synthesis_util as SU
from tests.golden_util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_on_hand_computed_cases():
    assert np.array_equal(SU.linspace01(1), [0.0]) and np.array_equal(SU.linspace01(2), [0.0, 1.0])
    assert np.array_equal(SU.linspace01(5), [0.0, 0.25, 0.5, 0.75, 1.0])
    for n in (1, 2, 3, 6, 7, 8, 9, 10, 11, 63, 64, 65, 1000, 1001, 4096, 65536):
        assert np.array_equal(SU.linspace01(n), torch.linspace(0, 1, n).numpy()), n
    assert np.array_equal(SU.lerp(0.25, [0.0, 4.0], [8.0, 0.0]), [2.0, 3.0])
    # orthogonal endpoints: omega = pi / 2, sin(omega) = 1; the un-normalised endpoints are blended
    got = SU.slerp(1.0 / 3.0, [2.0, 0.0], [0.0, 3.0])
    assert np.allclose(got, [2.0 * math.sin(math.pi / 3), 3.0 * math.sin(math.pi / 6)], rtol=0, atol=1e-15)
    got = SU.slerp(0.5, [1.0, 0.0, 0.0], [0.0, 0.0, 1.0])
    assert np.allclose(got, [math.sqrt(0.5), 0.0, math.sqrt(0.5)], rtol=0, atol=1e-15)
    # 60 degrees apart, half way: both coefficients sin(30) / sin(60) = 1 / sqrt(3)
    got = SU.slerp(0.5, [1.0, 0.0], [0.5, math.sqrt(0.75)])
    assert np.allclose(got, np.array([1.5, math.sqrt(0.75)]) / math.sqrt(3.0), rtol=0, atol=1e-15)
    rows = SU.walk([0.0, 4.0], [8.0, 0.0], 5, "lerp")
    assert rows.shape == (5, 2) and np.array_equal(rows[:, 0], [0.0, 2.0, 4.0, 6.0, 8.0])
    # the demo's default view: Rz(45 deg) Ry(60 deg), t = (0.05, 0, 0.5)
    R, t = SU.view()
    c, s60 = math.sqrt(0.5), math.sqrt(0.75)
    want = [[c * 0.5, -c, c * s60], [c * 0.5, c, c * s60], [-s60, 0.0, 0.5]]
    assert np.allclose(R, want, rtol=0, atol=1e-15) and np.allclose(t, [0.05, 0.0, 0.5], rtol=0, atol=1e-15)
    assert np.allclose(SU.view(120, 0, 0)[0], np.eye(3), rtol=0, atol=0) and np.array_equal(SU.view(120, 0, 0)[1], [0.1, 0.0, 1.0])
    # compaction: row-major order, a zero fourth column
    pts = np.arange(2 * 3 * 2 * 3, dtype=np.float32).reshape(2, 3, 2, 3)
    valid = np.array([[[1, 0, 0], [0, 1, 1]], [[0, 0, 0], [0, 0, 0]]], bool)
    records, counts = SU.compact(pts, valid)
    assert counts.tolist() == [3, 0] and records[1].shape == (0, 4)
    assert np.array_equal(records[0], [[0, 6, 12, 0], [4, 10, 16, 0], [5, 11, 17, 0]])


def test_restatement_reproduces_the_reference():
    """the reference's float32 rows lie within float32 rounding of the float64 restatement: a few ulp of the largest term
    (|z| < 5 here: 16 ulp(4) = 7.6e-6), and where one is not finite (nz = 1 under slerp) neither is the other"""
    g = load("synthesis")
    worst = 0.0
    for nz in SU.WALK_NZ:
        z0, z1 = g[f"walk/nz{nz}/z0"], g[f"walk/nz{nz}/z1"]
        assert z0.shape == z1.shape == (nz,) and z0.dtype == np.float32 and float(np.abs([z0, z1]).max()) < 5.0
        for n in SU.WALK_N:
            for mode in ("lerp", "slerp"):
                ref, mine = g[f"walk/nz{nz}/n{n}/{mode}"], SU.walk(z0, z1, n, mode)
                assert ref.shape == mine.shape == (n, nz)
                if nz == 1 and mode == "slerp":
                    assert not np.isfinite(ref).any()
                    continue
                assert np.isfinite(ref).all() and np.isfinite(mine).all()
                worst = max(worst, float(np.abs(ref - mine).max()))
        if nz > 1:
            assert 1.2 < float(g[f"walk/nz{nz}/angle"]) < 1.9
    assert 0.0 < worst < 7.6e-6, worst


def test_view_equals_the_reference_rotation():
    from dusty_gan_amd.synthesis import view
    g = load("synthesis")
    assert [tuple(v) for v in g["view/angles"].tolist()] == [tuple(float(x) for x in v) for v in SU.VIEWS]
    assert tuple(g["view/angles"][0]) == (60.0, -45.0, 60.0)
    for (zoom, yaw, pitch), R_ref in zip(SU.VIEWS, g["view/R"]):
        R, t = view(zoom, yaw, pitch)
        assert R.dtype == t.dtype == torch.float32 and R.shape == (3, 3) and t.shape == (3,) and not R.is_cuda
        assert float(np.abs(R.numpy().astype(np.float64) - R_ref.astype(np.float64)).max()) <= 1e-6, (zoom, yaw, pitch)
        R64, t64 = SU.view(zoom, yaw, pitch)
        assert np.array_equal(R.numpy(), R64.astype(np.float32)) and np.array_equal(t.numpy(), t64.astype(np.float32))
    R, t = view()
    assert np.array_equal(t.numpy(), np.array([0.05, 0.0, 0.5], np.float32))
    assert np.array_equal(R.numpy(), SU.view(60, -45, 60)[0].astype(np.float32))


def test_arguments_and_file_names():
    from dusty_gan_amd import synthesis as S
    from dusty_gan_amd import synthesize as C
    base = ["--model-path", "m.pth", "--config-path", "c.yaml"]
    a = C.parse_args(base)
    assert (a.num_samples, a.latent, a.seed, a.tol, a.zoom, a.yaw, a.pitch) == (4, "random", 0, 0, 60, -45, 60)
    assert a.save_dir_path == "." and not a.no_images and not a.no_bins
    a = C.parse_args(base + ["--num-samples", "1024", "--latent", "slerp", "--seed", "7", "--tol", "0.01", "--zoom", "30",
                             "--yaw", "10", "--pitch", "5", "--save-dir-path", "out", "--no-images", "--no-bins"])
    assert (a.num_samples, a.latent, a.seed, a.tol, a.zoom, a.yaw, a.pitch) == (1024, "slerp", 7, 0.01, 30, 10, 5)
    assert a.save_dir_path == "out" and a.no_images and a.no_bins
    for bad in (["--latent", "cubic"], ["--num-samples", "0"]):
        with pytest.raises(SystemExit):
            C.parse_args(base + bad)
    with pytest.raises(SystemExit):
        C.parse_args(["--model-path", "m.pth"])
    assert C.picture_name("synth/inv") == "inv.png" and C.picture_name("synth/inv/orig") == "inv_orig.png"
    assert C.picture_name("synth/confidence/pix") == "confidence_pix.png" and C.picture_name("synth/mask") == "mask.png"
    assert S.bin_path("d", 0) == os.path.join("d", "000000.bin") and S.bin_path("d", 123456) == os.path.join("d", "123456.bin")
    assert C.COLOR_SCALE == 2.5 and C.BEV_SIZE == 512
    # the library refuses CPU tensors and unknown modes before it touches the GPU
    with pytest.raises(RuntimeError):
        S.latent_walk(torch.zeros(4), torch.ones(4), 3, "lerp")
    with pytest.raises(ValueError):
        S.latent_walk(torch.zeros(4), torch.ones(4), 3, "cubic")


def test_write_bins_round_trip(tmp_path):
    from dusty_gan_amd.synthesis import write_bins
    HW = 12
    records = torch.arange(3 * HW * 4, dtype=torch.float32).view(3, HW, 4) + 0.5
    counts = torch.tensor([0, 1, HW], dtype=torch.int32)
    paths = write_bins(records, counts, str(tmp_path / "points"), first_index=41)
    assert paths == [str(tmp_path / "points" / f"{i:06d}.bin") for i in (41, 42, 43)]
    for b, path in enumerate(paths):
        assert os.path.getsize(path) == int(counts[b]) * 16
        back = np.fromfile(path, np.float32).reshape(-1, 4)
        assert np.array_equal(back, records[b, :int(counts[b])].numpy())
        assert open(path, "rb").read() == records[b, :int(counts[b])].numpy().astype("<f4").tobytes()


def test_header_declares_the_synthesis_symbols():
    from dusty_gan_amd import _lib
    h = open(os.path.join(ROOT, "include", "dusty_gan_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(dg_\w+)\s*\(", h, flags=re.M))
    assert {"dg_latent_walk", "dg_export_points"} <= declared
    assert {"dg_latent_walk", "dg_export_points"} <= set(_lib.PROTOTYPES)
    assert int(re.search(r"^#define\s+DG_EXPORT_CHUNK\s+(\d+)", h, flags=re.M).group(1)) == _lib.EXPORT_CHUNK
    src = open(os.path.join(ROOT, "dusty_gan_amd", "csrc", "Makefile")).read()
    assert "synthesis.hip" in src
