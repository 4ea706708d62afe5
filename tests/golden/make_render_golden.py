"""Generate tests/golden/render.npz from the REFERENCE's own utils/render.py.

Runs only where the reference's sources are at hand (DUSTY_REFERENCE, default /root/reference):
    python tests/golden/make_render_golden.py
utils/render.py is loaded by path and `render_point_clouds` / `bilinear_rasterizer` are called unmodified, in float32 and in
float64.  Its imports that are not installed here are stand-ins: numba (unused by the two functions), matplotlib (only
`colorize` uses it) and kornia.  `kornia.geometry.project_points` is restated here as the plain pinhole formula
xy / z * (fx, fy) + (cx, cy) in the dtype of the points: THIS ONE STEP IS THEREFORE PINNED TO THE FORMULA, NOT TO KORNIA
(whose version guards the division with an epsilon that no point of the fixture comes near).  The demo view's rotation is
the reference's utils/geometry.py euler_angles_to_rotation_matrix (demo.py:225-226), built in float32 and handed to both
precisions.

Clouds: B = 2 on a 16 x 64 nominal angle grid (the synthetic dataset's), depths 0.02 .. 0.52 of unit space, 15 % of the
points dropped to the origin, random normals in [0,1], L = 64.  Views: `train` R = None, t = (0, 0, 0.5) (train.py:92);
`demo` pitch 60 deg, yaw 45 deg, t = (0.05, 0, 0.5) (demo.py's slider defaults).  The bare rasterizer: B = 2, N = 700 random
coordinates over and around a 24 x 40 image, C = 1 and C = 3.

Decisions, not arithmetic, separate float32 from float64 where a coordinate lies on an integer (floor), on 0 or L-1 (the
in-image mask, the clamp) or a corner weight on the 1e-3 cut.  Every point that in float64 has a coordinate within 1e-3 of
an integer, or a corner weight within 1e-5 of 1e-3, in any view is re-drawn until none is left (asserted), so the tests
exclude no pixel.  The dropped points are exempt and checked separately: they project to t alone, the numerators 0 / z are
exactly zero in every precision, so their exact-integer coordinates take the same side of every decision everywhere.

What e_ref is made of.  The reference's float32 error is not uniform: its median over the lit elements is 3e-8 .. 4e-8 and
its 99.9th percentile 1e-5 in both views; the maximum is one pixel each.  A pixel's value is a ratio of sums of
(corner weight x point weight) terms, and a corner weight is a product of two coordinate differences whose ABSOLUTE
float32 error is that of a coordinate near L (a few 1e-6 after the projection); on a term that barely passes the 1e-3 cut
that is a relative error of 1e-3 and more.  The train view's maximum, 2.0e-5, is pixel (sample 0, row 53, column 30): two
terms, corner weights 1.6e-2 and 3.9e-3.  The demo view's, 1.5e-4, is pixel (sample 1, row 62, column 34): its ONLY two
terms have corner weights 1.13e-3 and 1.09e-3, both just above the cut, from points 503 and 695, each with one coordinate
within 1e-2 of the next integer, so the ratio takes the full relative error of each; three elements of that view exceed
2e-5.  An unresampled draw of the same set-up happened to hold no such pixel (2.0e-5 there).  The bound 2 e_ref + 1e-6 is
per view, so the demo view's is the wider one; the arithmetic itself is pinned far below either by the float64
edge-shape tests of tests/test_gpu_render.py (2e-7 on a ratio).

Contents (float64 results; e_ref = max |float32 result - float64 result| of the reference itself):
    meta/L, meta/torch
    cloud/xyz, cloud/normals [2,1024,3] f32
    view/<name>/R [3,3] f32 (demo only), view/<name>/t [3] f32, view/<name>/f64 [2,3,64,64], view/<name>/e_ref
    rast/coords [2,700,2] f32, rast/c<C>/values [2,700,C] f32, rast/c<C>/f64 [2,C,24,40], rast/c<C>/e_ref
"""
import importlib.util
import math
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("DUSTY_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
L_IMG, GRID_H, GRID_W, RH, RW, RN = 64, 16, 64, 24, 40, 700


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    for name in ("numba", "kornia", "kornia.geometry", "matplotlib", "matplotlib.cm"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["matplotlib"].cm = sys.modules["matplotlib.cm"]
    sys.modules["kornia"].geometry = sys.modules["kornia.geometry"]

    def project_points(point_3d, camera_matrix):
        K = camera_matrix.to(point_3d.dtype)
        xy = point_3d[..., :2] / point_3d[..., 2:3]
        return xy * torch.stack([K[..., 0, 0], K[..., 1, 1]], -1) + torch.stack([K[..., 0, 2], K[..., 1, 2]], -1)

    sys.modules["kornia.geometry"].project_points = project_points
    return _load(os.path.join(REF, "utils", "render.py"), "ref_render"), _load(os.path.join(REF, "utils", "geometry.py"), "ref_geometry")


def near_decision(coords, size):
    """[...,2] float64 splat coordinates -> bool [...]: within 1e-3 of an integer, or a corner weight within 1e-5 of 1e-3"""
    frac = coords - torch.floor(coords)
    near = ((frac < 1e-3) | (frac > 1 - 1e-3)).any(-1)
    fh, fw = frac[..., 0], frac[..., 1]
    for a in (fh, 1 - fh):
        for b in (fw, 1 - fw):
            near |= (a * b - 1e-3).abs() < 1e-5
    return near


def view_coords(xyz, R, t):
    """render_point_clouds' splat coordinates L - uv in float64"""
    p = xyz.double().clone()
    p[..., 2] *= -1
    if R is not None:
        p = p @ R.double()
    p = p + t.double()
    return L_IMG - (p[..., :2] / p[..., 2:3] + 0.5) * L_IMG


def make_cloud(rng, views):
    pitch = torch.linspace(math.radians(2.0), math.radians(-24.8), GRID_H)[:, None].expand(GRID_H, GRID_W).reshape(-1)
    yaw = (-(torch.arange(GRID_W).float() + 0.5) / GRID_W * 2 * math.pi + math.pi)[None].expand(GRID_H, GRID_W).reshape(-1)
    unit = torch.stack([pitch.cos() * yaw.cos(), pitch.cos() * yaw.sin(), pitch.sin()], -1)   # [N,3]
    N = unit.shape[0]
    dropped = torch.from_numpy(rng.random((2, N)) < 0.15)
    depth = torch.from_numpy(rng.uniform(0.02, 0.52, (2, N))).float()
    for _ in range(100):
        xyz = (unit[None] * depth[..., None]) * (~dropped)[..., None]
        bad = torch.zeros(2, N, dtype=torch.bool)
        for R, t in views:
            bad |= near_decision(view_coords(xyz, R, t), L_IMG)
        bad &= ~dropped
        if not bad.any():
            break
        depth[bad] = torch.from_numpy(rng.uniform(0.02, 0.52, int(bad.sum()))).float()
    assert not bad.any()
    normals = torch.from_numpy(rng.random((2, N, 3))).float()
    return xyz.contiguous(), normals, dropped


def main():
    ref, geo = load_reference()
    rng = np.random.default_rng(20261017)
    d = {"meta/L": np.array(L_IMG), "meta/torch": np.array(torch.__version__)}
    R_demo = geo.euler_angles_to_rotation_matrix(torch.tensor([0.0, math.radians(60.0), math.radians(45.0)])).float()
    views = {"train": (None, torch.tensor([0.0, 0.0, 0.5])), "demo": (R_demo, torch.tensor([0.05, 0.0, 0.5]))}
    xyz, normals, dropped = make_cloud(rng, list(views.values()))
    d["cloud/xyz"], d["cloud/normals"] = xyz.numpy(), normals.numpy()
    for name, (R, t) in views.items():
        # the dropped points: the same coordinates, bit for bit, in both precisions wherever they sit on an integer
        c64 = view_coords(xyz, R, t)[dropped]
        p32 = xyz.clone()
        p32[..., 2] *= -1
        p32 = (p32 @ R if R is not None else p32) + t
        c32 = (L_IMG - (p32[..., :2] / p32[..., 2:3] + 0.5) * L_IMG)[dropped].double()
        on_int = c64 == torch.floor(c64)
        assert torch.equal(c32[on_int], c64[on_int]) and not near_decision(torch.where(on_int, c64 + 0.5, c64), L_IMG).any()
        out = {}
        for dt in (torch.float32, torch.float64):
            torch.set_default_dtype(dt)      # (the reference allocates its image and its camera matrix in the default dtype)
            out[dt] = ref.render_point_clouds(xyz.to(dt).clone(), normals.to(dt), L=L_IMG, R=None if R is None else R.to(dt),
                                              t=t.to(dt)).double()
        torch.set_default_dtype(torch.float32)
        e_ref = float((out[torch.float32] - out[torch.float64]).abs().max())
        print(f"view {name}: e_ref = {e_ref:.3e}, {int((out[torch.float64].abs().sum(1) > 0).sum())} lit pixels")
        if R is not None:
            d[f"view/{name}/R"] = R.numpy()
        d[f"view/{name}/t"], d[f"view/{name}/f64"], d[f"view/{name}/e_ref"] = t.numpy(), out[torch.float64].numpy(), np.array(e_ref)
    # the bare rasterizer, points inside, on the rim and outside of a 24 x 40 image
    lo, hi = torch.tensor([-3.0, -3.0]), torch.tensor([RH + 2.0, RW + 2.0])
    coords = (torch.from_numpy(rng.random((2, RN, 2))).float() * (hi - lo) + lo)
    for _ in range(100):
        bad = near_decision(coords.double(), None)
        if not bad.any():
            break
        coords[bad] = torch.from_numpy(rng.random((int(bad.sum()), 2))).float() * (hi - lo) + lo
    assert not bad.any()
    d["rast/coords"] = coords.numpy()
    for C in (1, 3):
        values = torch.from_numpy(rng.uniform(-1.0, 1.0, (2, RN, C))).float()
        out = {}
        for dt in (torch.float32, torch.float64):
            torch.set_default_dtype(dt)
            out[dt] = ref.bilinear_rasterizer(coords.to(dt), values.to(dt), (RH, RW)).double()
        torch.set_default_dtype(torch.float32)
        e_ref = float((out[torch.float32] - out[torch.float64]).abs().max())
        print(f"rasterizer C = {C}: e_ref = {e_ref:.3e}")
        d[f"rast/c{C}/values"], d[f"rast/c{C}/f64"], d[f"rast/c{C}/e_ref"] = values.numpy(), out[torch.float64].numpy(), np.array(e_ref)
    path = os.path.join(HERE, "render.npz")
    np.savez_compressed(path, **d)
    print("wrote", path, f"{os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
