"""Generate tests/golden/synthesis.npz from the REFERENCE's own utils/interp.py and utils/geometry.py.

Runs only where the reference's sources are at hand (DUSTY_REFERENCE, default /root/reference):
    python tests/golden/make_synthesis_golden.py
Both files are loaded by path and `lerp`, `slerp` and `euler_angles_to_rotation_matrix` are called unmodified, as
demo.py:278-293 and :225-226 call them: endpoints [1, nz] float32, the weights the elements of torch.linspace(0, 1, n),
the angles a float32 tensor (0, pitch, -yaw) in radians.  Only their outputs are recorded.

Contents:
    meta/torch
    walk/nz<nz>/z0, walk/nz<nz>/z1            [nz] f32: seeded normal endpoints (torch.Generator().manual_seed(100 + nz))
    walk/nz<nz>/n<n>/lerp, .../slerp          [n, nz] f32: the reference's rows (nz = 1 under slerp is NaN: two numbers
                                              are always on one line)
    walk/nz<nz>/angle                         the float64 angle between the endpoints, radians (for the record: every
                                              nz > 1 pair lies between 1.2 and 1.9, where acos is well conditioned)
    view/angles [5,3] f64                     (zoom m, yaw deg, pitch deg), the demo's default first
    view/R      [5,3,3] f32                   the reference's R for each
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.synthesis_util import VIEWS, WALK_N, WALK_NZ, view_angles  # noqa: E402

REF = os.environ.get("DUSTY_REFERENCE", "/root/reference")


def load(name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(REF, "utils", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    interp, geometry = load("interp"), load("geometry")
    out = {"meta/torch": np.array(torch.__version__)}
    for nz in WALK_NZ:
        g = torch.Generator().manual_seed(100 + nz)
        z = torch.randn(2, nz, generator=g)
        out[f"walk/nz{nz}/z0"], out[f"walk/nz{nz}/z1"] = z[0].numpy().copy(), z[1].numpy().copy()
        a, b = z[0].double(), z[1].double()
        angle = float(torch.acos((a / a.norm() * (b / b.norm())).sum().clamp(-1, 1)))
        out[f"walk/nz{nz}/angle"] = np.float64(angle)
        assert nz == 1 or 1.2 < angle < 1.9, (nz, angle)
        for n in WALK_N:
            for mode in ("lerp", "slerp"):
                f = getattr(interp, mode)
                rows = torch.cat([f(w, z[[0]], z[[1]]) for w in torch.linspace(0, 1, n)], dim=0)
                assert rows.shape == (n, nz) and rows.dtype == torch.float32
                out[f"walk/nz{nz}/n{n}/{mode}"] = rows.numpy().copy()
    Rs = []
    for zoom, yaw, pitch in VIEWS:
        Rs.append(geometry.euler_angles_to_rotation_matrix(torch.tensor(view_angles(yaw, pitch)).float()).numpy())
    out["view/angles"] = np.array(VIEWS, np.float64)
    out["view/R"] = np.stack(Rs).astype(np.float32)
    path = os.path.join(HERE, "synthesis.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
