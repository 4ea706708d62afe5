"""Write dusty_gan_amd/csrc/turbo_lut.h: matplotlib's 256-entry turbo colour table as a float constant.

    python scripts/make_turbo_lut.py

Needs matplotlib (build time only; nothing imports it at run time).  The table is `cm.turbo(np.linspace(0, 1, 256))[:, :3]`,
printed with nine significant digits (float32 round-trips); tests/test_render_cpu.py compares the header with matplotlib
where it is installed.  The script also checks that the byte the image log derives from an entry, trunc(v * 255), is the
same in float32 (the kernel) and in float64 (matplotlib + TensorBoard's conversion).
"""
import os

import numpy as np
from matplotlib import cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    lut = cm.turbo(np.linspace(0, 1, 256))[:, :3]
    f32 = lut.astype(np.float32)
    b64 = np.clip(lut * 255, 0, 255).astype(np.uint8)
    b32 = np.clip(f32 * np.float32(255), 0, 255).astype(np.uint8)
    assert np.array_equal(b64, b32), "a table entry truncates to another byte in float32"
    lines = ["// matplotlib's turbo colour map, cm.turbo(np.linspace(0, 1, 256))[:, :3] (written by scripts/make_turbo_lut.py;",
             f"// matplotlib {__import__('matplotlib').__version__}).  Row i = (r, g, b) of table index i.",
             "#pragma once", "", "static constexpr float DG_TURBO_LUT[256 * 3] = {"]
    for r, g, b in f32:
        lines.append(f"    {r:.9g}f, {g:.9g}f, {b:.9g}f,")
    lines.append("};")
    path = os.path.join(ROOT, "dusty_gan_amd", "csrc", "turbo_lut.h")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
