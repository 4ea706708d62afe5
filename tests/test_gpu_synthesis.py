"""The synthesis command on the MI355X (dusty_gan_amd/synthesis.py, dusty_gan_amd/synthesize.py, csrc/synthesis.hip):
dg_latent_walk against the float64 restatement of the reference's lerp / slerp, dg_export_points against
LiDAR.inv_to_xyz plus a host compaction (bit for bit), and the command end to end on a fresh generator."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import synthesis_util as SU
from tests.golden_util import load

pytestmark = pytest.mark.gpu
DEV = "cuda"
MIN_DEPTH, MAX_DEPTH = 1.45, 80.0
NAN_BITS = 0x7FC00ABC   # a quiet NaN with a payload: the sentinel of records that must not be written


# ---------------------------------------------------------------------------------------------- dg_latent_walk
def raw_walk(z0, z1, n, mode, nz=None):
    """dg_latent_walk itself (no finiteness check) -> (return code, [n, nz] tensor)"""
    from dusty_gan_amd import _lib as L
    nz = z0.numel() if nz is None else nz
    out = torch.full((max(n, 1), max(nz, 1)), float("nan"), device=DEV)
    rc = L.lib().dg_latent_walk(L.ptr(z0), L.ptr(z1), n, nz, mode, L.ptr(out), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


@pytest.fixture(scope="module")
def walk_bounds():
    """4 x the largest error of the reference's own float32 rows (the golden file) against float64, per mode: the margin is
    for the device's sin / acos differing from the host's.  The reference's error: lerp 2.4e-7, slerp 2.9e-7 (bounds 9.5e-7
    and 1.15e-6); the kernel measured 1.2e-7 in both modes on an MI355X."""
    g = load("synthesis")
    e_ref = {"lerp": 0.0, "slerp": 0.0}
    for nz in SU.WALK_NZ:
        for n in SU.WALK_N:
            for mode in e_ref:
                ref = g[f"walk/nz{nz}/n{n}/{mode}"]
                if np.isfinite(ref).all():
                    e_ref[mode] = max(e_ref[mode], float(np.abs(ref - SU.walk(g[f"walk/nz{nz}/z0"], g[f"walk/nz{nz}/z1"], n, mode)).max()))
    assert all(1e-8 < e < 1e-6 for e in e_ref.values()), e_ref
    return {mode: 4.0 * e for mode, e in e_ref.items()}


def test_latent_walk_against_float64(walk_bounds):
    from dusty_gan_amd import _lib as L
    from dusty_gan_amd.synthesis import MODES, latent_walk
    g = load("synthesis")
    worst = {"lerp": 0.0, "slerp": 0.0}
    for nz in SU.WALK_NZ:
        z0n, z1n = g[f"walk/nz{nz}/z0"], g[f"walk/nz{nz}/z1"]
        z0, z1 = torch.from_numpy(z0n).to(DEV), torch.from_numpy(z1n).to(DEV)
        for n in SU.WALK_N + (5, 64):
            for mode in ("lerp", "slerp"):
                rc, out = raw_walk(z0, z1, n, MODES[mode])
                assert rc == L.DG_OK and out.shape == (n, nz)
                if nz == 1 and mode == "slerp":   # two numbers are always on one line: no arc (the reference: NaN)
                    assert not bool(torch.isfinite(out).any())
                    with pytest.raises(ValueError):
                        latent_walk(z0, z1, n, mode)
                    continue
                got = out.cpu().numpy()
                assert np.isfinite(got).all()
                assert torch.equal(latent_walk(z0, z1, n, mode), out)
                assert torch.equal(latent_walk(z0[None], z1[None], n, mode), out)   # [1, nz] rows, as the demo holds them
                worst[mode] = max(worst[mode], float(np.abs(got - SU.walk(z0n, z1n, n, mode)).max()))
                # the ends: n = 1 is z0; lerp's first and last rows are the endpoints themselves
                assert np.array_equal(got[0], z0n), (nz, n, mode)
                if mode == "lerp" and n > 1:
                    assert np.array_equal(got[-1], z1n), (nz, n)
    print("dg_latent_walk max |error| vs float64:", worst, "bounds:", walk_bounds)
    for mode in worst:
        assert worst[mode] <= walk_bounds[mode], (mode, worst[mode], walk_bounds[mode])


def test_latent_walk_degenerate_endpoints_and_bad_arguments():
    from dusty_gan_amd import _lib as L
    from dusty_gan_amd.synthesis import latent_walk
    z = torch.randn(100, generator=torch.Generator().manual_seed(3)).to(DEV)
    for other in (z.clone(), 2.0 * z, -z, -0.5 * z):   # identical, parallel, antipodal
        with pytest.raises(ValueError):
            latent_walk(z, other, 4, "slerp")
        assert bool(torch.isfinite(latent_walk(z, other, 4, "lerp")).all())
    with pytest.raises(ValueError):
        latent_walk(z, z[:50], 4, "lerp")
    with pytest.raises(ValueError):
        latent_walk(z, z, 0, "lerp")
    with pytest.raises(RuntimeError):
        latent_walk(z.cpu(), z.cpu(), 4, "lerp")
    assert raw_walk(z, z, 0, 0)[0] == L.DG_EINVAL
    assert raw_walk(z, z, -1, 0)[0] == L.DG_EINVAL
    assert raw_walk(z, z, 4, 0, nz=0)[0] == L.DG_EINVAL
    assert raw_walk(z, z, 4, 2)[0] == L.DG_EINVAL and raw_walk(z, z, 4, -1)[0] == L.DG_EINVAL
    out = torch.empty(4, 100, device=DEV)
    assert L.lib().dg_latent_walk(None, L.ptr(z), 4, 100, 0, L.ptr(out), L.stream_ptr()) == L.DG_EINVAL
    assert L.lib().dg_latent_walk(L.ptr(z), L.ptr(z), 4, 100, 0, None, L.stream_ptr()) == L.DG_EINVAL


def test_sample_latents_draws_the_engines_stream():
    from types import SimpleNamespace as NS

    from dusty_gan_amd.synthesis import latent_walk, sample_latents
    from dusty_gan_amd.utils.rng import Philox
    cfg = NS(model=NS(gen=NS(in_ch=100)))
    for seed in (0, 7):
        want = Philox(seed, DEV).normal(5 * 100).view(5, 100)
        assert torch.equal(sample_latents(cfg, DEV, 5, "random", seed), want)
        ends = Philox(seed, DEV).normal(2 * 100).view(2, 100)
        assert torch.equal(ends, want[:2])
        for mode in ("lerp", "slerp"):
            got = sample_latents(cfg, DEV, 5, mode, seed)
            assert got.shape == (5, 100) and torch.equal(got, latent_walk(ends[0], ends[1], 5, mode))
            assert torch.equal(got[0], ends[0])
    assert not torch.equal(sample_latents(cfg, DEV, 5, "random", 0), sample_latents(cfg, DEV, 5, "random", 7))
    with pytest.raises(ValueError):
        sample_latents(cfg, DEV, 5, "cubic", 0)


# -------------------------------------------------------------------------------------------- dg_export_points
SHAPES = [(1, 1, 64),        # one wave
          (1, 2, 100),       # a partial chunk, not a multiple of 64
          (3, 5, 1000),      # several chunks, the last one partial
          (2, 64, 1024)]     # the real scan
PATTERNS = ("none", "all", "bernoulli", "first", "last", "chunk", "mixed")


def make_lidar(H, W, angles):
    from dusty_gan_amd.utils.lidar import LiDAR
    lidar = LiDAR(H, W, MIN_DEPTH, MAX_DEPTH).use_nominal_angles()
    if angles == "random":
        g = torch.Generator().manual_seed(H * 10007 + W)
        pitch = torch.rand(H, W, generator=g) * 0.5 - 0.45
        yaw = torch.rand(H, W, generator=g) * 2 * np.pi - np.pi
        lidar.angle = torch.stack([pitch, yaw])[None].contiguous()
    return lidar.to(DEV)


def keep_of(pattern, B, HW, g, b0=0):
    """[B, HW] bool: the pixels a drop pattern keeps"""
    from dusty_gan_amd._lib import EXPORT_CHUNK
    keep = torch.ones(B, HW, dtype=torch.bool)
    if pattern == "all":
        keep[:] = False
    elif pattern == "bernoulli":
        keep = torch.rand(B, HW, generator=g) < 0.5
    elif pattern == "first":
        keep[:] = False
        keep[:, 0] = True
    elif pattern == "last":
        keep[:] = False
        keep[:, -1] = True
    elif pattern == "chunk":   # one whole interior chunk of the kernel; a scan of fewer than three chunks: its middle third
        lo, hi = (EXPORT_CHUNK, 2 * EXPORT_CHUNK) if HW >= 3 * EXPORT_CHUNK else (HW // 3, 2 * HW // 3)
        keep[:, lo:hi] = False
    elif pattern == "mixed":   # a different pattern per scan
        order = ("bernoulli", "last", "chunk", "all", "first", "none")
        for b in range(B):
            keep[b] = keep_of(order[(b + b0) % len(order)], 1, HW, g)[0]
    return keep


def make_inv(keep, B, H, W, from_tanh, g):
    """inverse depth [B,1,H,W] with the drop constant (0 of [0,1]) at the dropped pixels; of the kept pixels one in eight
    lies at 0.005 and one in eight at 0.02 of [0,1], either side of tol = 1e-2, the rest in 0.05 .. 0.95"""
    inv01 = torch.rand(B, H * W, generator=g) * 0.9 + 0.05
    pick = torch.randint(0, 8, (B, H * W), generator=g)
    inv01 = torch.where(pick == 0, torch.full_like(inv01, 0.005), inv01)
    inv01 = torch.where(pick == 1, torch.full_like(inv01, 0.02), inv01)
    inv01 = torch.where(keep, inv01, torch.zeros_like(inv01)).view(B, 1, H, W)
    return (inv01 * 2 - 1 if from_tanh else inv01).to(DEV)


def raw_export(inv, lidar, tol, from_tanh, out=None):
    """dg_export_points itself -> (records with the sentinel wherever nothing was stored, counts)"""
    from dusty_gan_amd import _lib as L
    B, _, H, W = inv.shape
    if out is None:
        out = torch.full((B, H * W, 4), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    counts = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    chunks = torch.full((B * (-(-H * W // L.EXPORT_CHUNK)),), -7, dtype=torch.int32, device=DEV)
    L.check(L.lib().dg_export_points(L.ptr(inv), L.ptr(lidar.angle), B, H, W, int(from_tanh), lidar.min_depth, lidar.max_depth,
                                     lidar.drop_const, float(tol), L.ptr(chunks), L.ptr(out), L.ptr(counts), L.stream_ptr()),
            "dg_export_points")
    return out, counts


def reference_records(inv, lidar, tol, from_tanh):
    """LiDAR.inv_to_xyz(...) * max_depth gathered at the valid pixels in row-major order on the host -> (list of [k,4]
    float32 arrays, counts); valid by the kernel's own predicate on the [0,1] inverse depth it returns"""
    pts, d01 = lidar.inv_to_xyz(inv, tol, from_tanh=from_tanh, return_depth=True)
    metres = (pts * lidar.max_depth).cpu().numpy()
    valid = np.abs(d01.cpu().numpy()[:, 0] - np.float32(lidar.drop_const)) > np.float32(tol)
    return SU.compact(metres, valid)


def check_export(inv, lidar, tol, from_tanh, what):
    B, _, H, W = inv.shape
    want, want_counts = reference_records(inv, lidar, tol, from_tanh)
    out, counts = raw_export(inv, lidar, tol, from_tanh)
    assert counts.cpu().tolist() == want_counts.tolist(), what
    bits = out.view(torch.int32).cpu().numpy()
    for b in range(B):
        k = int(want_counts[b])
        assert np.array_equal(bits[b, :k], want[b].astype(np.float32).view(np.int32)), (what, b)   # bit-equal
        assert (bits[b, :k, 3] == 0).all(), (what, b)
        assert (bits[b, k:] == NAN_BITS).all(), (what, b)   # nothing written at or beyond counts[b]
    return out, counts, want_counts


@pytest.mark.parametrize("angles", ["nominal", "random"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_export_points_equals_inv_to_xyz_compacted(shape, angles):
    from dusty_gan_amd.synthesis import export_points
    B, H, W = shape
    lidar = make_lidar(H, W, angles)
    g = torch.Generator().manual_seed(B * 1000 + H + W)
    seen = set()
    for pi, pattern in enumerate(PATTERNS):
        if pattern == "mixed" and B == 1:
            continue
        keep = keep_of(pattern, B, H * W, g)
        for from_tanh in (True, False):
            inv = make_inv(keep, B, H, W, from_tanh, g)
            for tol in (0.0, 1e-2):
                what = (shape, angles, pattern, from_tanh, tol)
                out, counts, want_counts = check_export(inv, lidar, tol, from_tanh, what)
                seen.add((pattern, tuple(want_counts.tolist())))
                if tol == 0.0:   # the pattern is what the kernel saw: the kept pixels, all of them
                    assert want_counts.tolist() == keep.sum(dim=1).tolist(), what
                elif int(keep.sum()) >= 64:   # the pixels at 0.005 fall under the tolerance, those at 0.02 do not
                    assert 0 < int(want_counts.sum()) < int(keep.sum()), what
            if pattern == "bernoulli":   # two calls, identical bytes; the library call is the same launch
                again, counts2 = raw_export(inv, lidar, 1e-2, from_tanh)
                assert torch.equal(again.view(torch.int32), out.view(torch.int32)) and torch.equal(counts2, counts)
                rec, cnt = export_points(inv, lidar, tol=1e-2, from_tanh=from_tanh)
                assert rec.shape == (B, H * W, 4) and cnt.dtype == torch.int32 and torch.equal(cnt, counts)
                for b in range(B):
                    k = int(cnt[b])
                    assert torch.equal(rec[b, :k].view(torch.int32), out[b, :k].view(torch.int32))
    assert len(seen) >= (6 if B == 1 else 7)


def test_export_points_bad_arguments():
    from dusty_gan_amd import _lib as L
    from dusty_gan_amd.synthesis import export_points
    B, H, W = 1, 2, 100
    lidar = make_lidar(H, W, "nominal")
    inv = torch.zeros(B, 1, H, W, device=DEV)
    out = torch.empty(B * H * W * 4 + 4, device=DEV)
    counts = torch.empty(B, dtype=torch.int32, device=DEV)
    chunks = torch.empty(4, dtype=torch.int32, device=DEV)

    def call(inv_p=L.ptr(inv), angle_p=L.ptr(lidar.angle), B=B, H=H, W=W, chunks_p=L.ptr(chunks), out_p=L.ptr(out),
             counts_p=L.ptr(counts)):
        return L.lib().dg_export_points(inv_p, angle_p, B, H, W, 1, MIN_DEPTH, MAX_DEPTH, 0.0, 0.0, chunks_p, out_p, counts_p,
                                        L.stream_ptr())
    assert call() == L.DG_OK
    for kw in ({"inv_p": None}, {"angle_p": None}, {"chunks_p": None}, {"out_p": None}, {"counts_p": None}, {"B": 0},
               {"H": 0}, {"W": -1}, {"out_p": L.ptr(out) + 4},          # records are stored 16 bytes at a time
               {"H": 1 << 16, "W": 1 << 15}):                           # H W = 2^31: past the int32 counts
        assert call(**kw) == L.DG_EINVAL, kw
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        export_points(inv.cpu(), lidar)


def test_export_points_indexes_past_2_31():
    """B H W 4 > 2^31 floats: the last scan's records land where a 64-bit index puts them"""
    B, H, W = 8200, 64, 1024
    assert B * H * W * 4 > 2**31
    lidar = make_lidar(H, W, "nominal")
    g = torch.Generator().manual_seed(1)
    keep = torch.rand(1, H * W, generator=g) < 1.0 / 16
    one = make_inv(keep, 1, H, W, True, g)
    want, want_counts = reference_records(one, lidar, 0.0, True)
    inv = one.expand(B, 1, H, W).contiguous()
    out = torch.empty(B, H * W, 4, device=DEV)
    out[-1].view(torch.int32).fill_(NAN_BITS)
    out, counts = raw_export(inv, lidar, 0.0, True, out=out)
    k = int(want_counts[0])
    assert 0 < k < H * W and bool((counts == k).all())
    for b in (0, B // 2, B - 1):
        assert np.array_equal(out[b, :k].cpu().numpy().view(np.int32), want[0].astype(np.float32).view(np.int32)), b
    assert bool((out[-1, k:].view(torch.int32) == NAN_BITS).all())


# ------------------------------------------------------------------------------------------------- the command
def make_world(tmp, model, name):
    from dusty_gan_amd.models import define_G
    from dusty_gan_amd.utils.config import dump_config, load_config
    cfg = load_config([f"model={model}", "dataset=synthetic", "dataset.shape=[64,1024]", "solver.batch_size=4",
                       "enable_amp=true"])
    cfg_path, ckpt = str(tmp / f"{name}.yaml"), str(tmp / f"{name}.pth")
    dump_config(cfg, cfg_path)
    torch.manual_seed(0)
    cfg.model.gen.shape = cfg.dataset.shape
    sd = define_G(cfg).state_dict()
    # (tests/test_gpu_evaluate_synthesis.py) a fresh generator's inverse depths stay within 0.5 +- 0.2: the depth head is
    # scaled and shifted so that the depths spread from a few metres to the far end
    prefix = "backbone." if model != "dcgan_eqlr" else ""
    sd[prefix + "4.heads.depth.1.module.weight"] *= 10.0
    sd[prefix + "4.heads.depth.1.module.bias"] -= 1.5
    torch.save({"step": 0, "G_ema": sd}, ckpt)
    return ["--model-path", ckpt, "--config-path", cfg_path]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """config and checkpoint of a seeded full-width dusty2 generator at 64x1024, batches of 4 -> argv and the loaded setup"""
    from dusty_gan_amd import utils
    tmp = tmp_path_factory.mktemp("synthesize")
    argv = make_world(tmp, "dusty2_dcgan_eqlr", "dusty2")
    cfg, G, lidar, device = utils.setup(argv[1], argv[3], ema=True, fix_noise=True)
    return {"tmp": tmp, "argv": argv, "cfg": cfg, "G": G, "lidar": lidar, "device": device}


def read_bins(dir, n):
    assert sorted(os.listdir(dir)) == [f"{i:06d}.bin" for i in range(n)]
    return [np.fromfile(os.path.join(dir, f"{i:06d}.bin"), np.float32).reshape(-1, 4) for i in range(n)]


def test_command_writes_bins_pictures_and_the_view(world):
    from PIL import Image

    from dusty_gan_amd import synthesis as S
    from dusty_gan_amd import synthesize as cmd
    from dusty_gan_amd.train import image_tags
    from dusty_gan_amd.utils.render import flatten, grid_shape, image_grid, render_point_clouds
    cfg, G, lidar, device = world["cfg"], world["G"], world["lidar"], world["device"]
    save = str(world["tmp"] / "a")
    out_dir = cmd.main(world["argv"] + ["--num-samples", "6", "--latent", "slerp", "--save-dir-path", save])
    assert out_dir == os.path.join(save, "synthesis")
    latents = np.load(os.path.join(out_dir, "latents.npy"))
    assert latents.shape == (6, int(cfg.model.gen.in_ch)) and latents.dtype == np.float32
    assert np.array_equal(latents, S.sample_latents(cfg, device, 6, "slerp", 0).cpu().numpy())
    # six bins = export_points of synthesize()'s depth for the saved latents (6 = a full batch of 4 and a padded one of 2)
    out = S.synthesize(cfg, G, lidar, torch.from_numpy(latents).to(device))
    assert out["depth"].shape == (6, 1, 64, 1024) and len({float(out["depth"][i].sum()) for i in range(6)}) == 6
    records, counts = S.export_points(out["depth"], lidar, tol=0.0, from_tanh=False)
    bins = read_bins(os.path.join(out_dir, "points"), 6)
    mask_points = out["mask"].prod(dim=1).sum(dim=(1, 2))
    for i in range(6):
        k = int(counts[i])
        assert 0 < k < 64 * 1024 and bins[i].shape == (k, 4)   # some pixels drop
        assert np.array_equal(bins[i].view(np.int32), records[i, :k].cpu().numpy().view(np.int32)), i
        assert k == int(mask_points[i]), (i, k, int(mask_points[i]))
        assert float(np.abs(bins[i][:, :3]).max()) <= lidar.max_depth * 1.001 and (bins[i][:, 3] == 0).all()
    # every picture image_tags names, as a make_grid of the six samples
    full = dict(out)
    R, t = (v.to(device) for v in S.view())
    full["bev"] = render_point_clouds(flatten(out["points"]), flatten(out["normals"]), L=512, R=R, t=t)
    full["mask_prod"] = out["mask"].prod(dim=1, keepdim=True)
    tags = image_tags(full)
    names = {cmd.picture_name(tag) for tag, *_ in tags}
    assert names == {"inv.png", "normal.png", "bev.png", "inv_orig.png", "confidence_pix.png", "confidence_img.png",
                     "mask_pix.png", "mask_img.png", "mask.png"}
    assert set(os.listdir(out_dir)) == names | {"bev_rgba.png", "latents.npy", "points"}
    for tag, key, channel, color in tags:
        x = full[key] if channel is None else full[key][:, channel:channel + 1]
        Hg, Wg = grid_shape(6, *x.shape[2:])
        img = np.asarray(Image.open(os.path.join(out_dir, cmd.picture_name(tag))))
        assert img.shape == (Hg, Wg, 3) and img.dtype == np.uint8, tag
        scale = cmd.COLOR_SCALE if key in ("depth", "depth_orig") else 1.0
        assert np.array_equal(img, image_grid(x, color=color, scale=scale).cpu().numpy()), tag
    # the RGBA bird's-eye view: alpha 0 exactly where the rendered RGB has a zero channel (and on the grid's padding)
    rgba = np.asarray(Image.open(os.path.join(out_dir, "bev_rgba.png")))
    Hg, Wg = grid_shape(6, 512, 512)
    assert rgba.shape == (Hg, Wg, 4)
    assert np.array_equal(rgba[..., :3], np.asarray(Image.open(os.path.join(out_dir, "bev.png"))))
    lit = torch.all(full["bev"] != 0.0, dim=1, keepdim=True).float()
    want_alpha = image_grid(lit, color=False).cpu().numpy()[..., 0]
    assert set(np.unique(want_alpha).tolist()) == {0, 255}
    assert np.array_equal(rgba[..., 3], want_alpha)
    for i in range(6):   # sample i's cell of the grid, pixel for pixel
        r, c = divmod(i, 4)
        cell = rgba[2 + r * 514:2 + r * 514 + 512, 2 + c * 514:2 + c * 514 + 512, 3]
        assert np.array_equal(cell == 0, (full["bev"][i] == 0.0).any(dim=0).cpu().numpy()), i


def test_command_no_images_and_seeded_repeats(world, monkeypatch):
    from dusty_gan_amd import synthesize as cmd
    from dusty_gan_amd.utils import lidar as U
    runs = []
    for name in ("r1", "r2", "r3"):
        save = str(world["tmp"] / name)
        seed = "5" if name != "r3" else "6"
        out_dir = cmd.main(world["argv"] + ["--num-samples", "5", "--latent", "random", "--seed", seed, "--save-dir-path", save])
        runs.append({f: open(os.path.join(root, f), "rb").read() for root, _, files in os.walk(out_dir) for f in files})
    assert set(runs[0]) == set(runs[1]) and len(runs[0]) == 1 + 5 + 10
    assert runs[0] == runs[1]   # --seed s twice: identical files
    assert runs[0]["latents.npy"] != runs[2]["latents.npy"] and runs[0]["000000.bin"] != runs[2]["000000.bin"]

    def no_normals(*a, **k):
        raise AssertionError("--no-images computed normals")
    monkeypatch.setattr(U, "xyz_to_normal", no_normals)
    save = str(world["tmp"] / "lean")
    out_dir = cmd.main(world["argv"] + ["--num-samples", "5", "--seed", "5", "--save-dir-path", save, "--no-images"])
    assert sorted(os.listdir(out_dir)) == ["latents.npy", "points"]
    for i, b in enumerate(read_bins(os.path.join(out_dir, "points"), 5)):
        assert b.tobytes() == runs[0][f"{i:06d}.bin"]
    out_dir = cmd.main(world["argv"] + ["--num-samples", "2", "--save-dir-path", str(world["tmp"] / "bare"), "--no-images",
                                        "--no-bins"])
    assert os.listdir(out_dir) == ["latents.npy"]


def test_command_on_a_baseline_checkpoint(tmp_path):
    """dcgan_eqlr has no confidence head: no mask, no dropped pixel, no mask pictures"""
    from dusty_gan_amd import synthesize as cmd
    argv = make_world(tmp_path, "dcgan_eqlr", "baseline")
    out_dir = cmd.main(argv + ["--num-samples", "3", "--latent", "lerp", "--save-dir-path", str(tmp_path)])
    assert set(os.listdir(out_dir)) == {"inv.png", "normal.png", "bev.png", "bev_rgba.png", "latents.npy", "points"}
    bins = read_bins(os.path.join(out_dir, "points"), 3)
    assert all(0 < len(b) <= 64 * 1024 and np.isfinite(b).all() for b in bins)
    assert np.load(os.path.join(out_dir, "latents.npy")).shape[0] == 3
