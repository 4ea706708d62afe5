"""Generate tests/golden/corruption.npz from the REFERENCE's own functions: the target corruptions of its demo (demo.py:71-137).

Runs only where the reference's sources are at hand (DUSTY_REFERENCE, default /root/reference), on the CPU:
    python tests/golden/make_corruption_golden.py
demo.py cannot be imported (it needs streamlit and kornia).  Its text is parsed with `ast` and ONLY the definitions of
dropout_noise, sparse_hlines, sparse_vlines, random_lines, corrupt_half, corrupt_quarter, additive_noise, closing and
apply_corruption are compiled, into a namespace that holds
    torch   torch itself, with rand_like / randn_like / randperm wrapped so that what they return is recorded
    F       torch.nn.functional, with max_pool2d wrapped so that every sweep's input is recorded
    kornia  a stand-in whose filters.median_blur is this script's restatement of kornia's: F.unfold(x, 3, padding=1) - zero
            padding - and torch.median over the nine taps (the lower median of nine: the 5th smallest).
Nothing of the reference's text is copied here.

Cases [B,H,W] (keep probability; a rectangular hole at least 3 pixels deep, so that Jacobi sweeps and an in-place raster
update give different images):
    c0 [1,5,37]    keep 0.6   HW is no multiple of 4; the hole touches the top and left borders
    c1 [1,8,96]    keep 0.7
    c2 [2,16,160]  keep 0.5   sample 0's hole spans all 16 rows
Per case:
    depth, mask [B,1,H,W]        u, noise [B,1,H,W] what rand_like / randn_like returned inside apply_corruption (seed 0)
    <name>/depth, <name>/mask    apply_corruption's outputs for "additive noise", "low resolution", "dropout", "closing"
                                 (key: the name with '_' for ' ')
    median [B,1,H,W]             the stand-in's median image of depth
    sweeps [B] int32             per sample, the sweeps of closing's loop that changed the sample
    fn/dropout_u, fn/dropout (rate 0.5), fn/hlines (1/2), fn/vlines (1/4), fn/rows + fn/random_lines (rate 0.5), fn/half,
    fn/quarter                   the mask functions apply_corruption does not name
"""
import ast
import os
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DUSTY_REFERENCE", "/root/reference")
WANTED = ("dropout_noise", "sparse_hlines", "sparse_vlines", "random_lines", "corrupt_half", "corrupt_quarter",
          "additive_noise", "closing", "apply_corruption")
NAMED = ("additive noise", "low resolution", "dropout", "closing")
CASES = {"c0": ((1, 5, 37), 0.6, [(0, 4, 0, 10)]),
         "c1": ((1, 8, 96), 0.7, [(2, 8, 30, 61)]),
         "c2": ((2, 16, 160), 0.5, [(0, 16, 60, 91), (5, 14, 100, 160)])}

LOG = {"rand": [], "randn": [], "perm": [], "pool": []}


class _Recorded:
    """a module whose listed functions record what they return (or, for `inputs`, what they are given)"""

    def __init__(self, mod, outputs=(), inputs=()):
        self._mod, self._outputs, self._inputs = mod, dict(outputs), dict(inputs)

    def __getattr__(self, name):
        fn = getattr(self._mod, name)
        if name in self._outputs:
            def wrapped(*a, **k):
                r = fn(*a, **k)
                LOG[self._outputs[name]].append(r.clone())
                return r
            return wrapped
        if name in self._inputs:
            def wrapped(*a, **k):
                LOG[self._inputs[name]].append(a[0].clone())
                return fn(*a, **k)
            return wrapped
        return fn


def median_blur(x, kernel_size):
    """kornia.filters.median_blur for a 3x3 kernel, restated: zero padding, the median of the nine taps"""
    assert tuple(kernel_size) == (3, 3)
    B, C, H, W = x.shape
    taps = F.unfold(x.reshape(B * C, 1, H, W), 3, padding=1)   # [BC, 9, HW]
    return torch.median(taps, dim=1).values.reshape(B, C, H, W)


def reference_functions():
    tree = ast.parse(open(os.path.join(REF, "demo.py")).read())
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(d.name for d in defs) == sorted(WANTED)
    ns = {"torch": _Recorded(torch, outputs={"rand_like": "rand", "randn_like": "randn", "randperm": "perm"}),
          "F": _Recorded(F, inputs={"max_pool2d": "pool"}),
          "kornia": types.SimpleNamespace(filters=types.SimpleNamespace(median_blur=median_blur))}
    exec(compile(ast.Module(body=defs, type_ignores=[]), "demo.py", "exec"), ns)
    return ns


def make_case(ns, shape, keep, holes, seed):
    g = torch.Generator().manual_seed(seed)
    B, H, W = shape
    mask = (torch.rand(B, 1, H, W, generator=g) < keep).float()
    for b, (h0, h1, w0, w1) in enumerate(holes):
        mask[b, :, h0:h1, w0:w1] = 0.0
    depth = (0.05 + 0.9 * torch.rand(B, 1, H, W, generator=g)) * mask
    data = {"depth": depth, "mask": mask}
    for name in NAMED:
        for v in LOG.values():
            v.clear()
        d, m = ns["apply_corruption"](depth.clone(), mask.clone(), name)
        key = name.replace(" ", "_")
        data[f"{key}/depth"], data[f"{key}/mask"] = d, m
        if name == "additive noise":
            data["noise"], = LOG["randn"]
        if name == "dropout":
            data["u"], = LOG["rand"]
        if name == "closing":
            states = LOG["pool"] + [d]   # the image before every sweep, then the result
            data["sweeps"] = torch.tensor([sum(int(not torch.equal(a[b], c[b])) for a, c in zip(states, states[1:]))
                                           for b in range(B)], dtype=torch.int32)
            assert bool((d > 1e-8).all())
    data["median"] = median_blur(depth, (3, 3))
    for v in LOG.values():
        v.clear()
    torch.manual_seed(seed + 1)
    data["fn/dropout"] = ns["dropout_noise"](mask.clone(), 0.5)
    data["fn/dropout_u"], = LOG["rand"]
    data["fn/hlines"] = ns["sparse_hlines"](mask.clone(), 1 / 2)
    data["fn/vlines"] = ns["sparse_vlines"](mask.clone(), 1 / 4)
    data["fn/random_lines"] = ns["random_lines"](mask.clone(), 0.5)
    perm, = LOG["perm"]
    data["fn/rows"] = perm[: int(H * 0.5)].to(torch.int64)
    data["fn/half"] = ns["corrupt_half"](mask.clone())
    data["fn/quarter"] = ns["corrupt_quarter"](mask.clone())
    return data


def main():
    ns = reference_functions()
    out = {}
    for i, (case, (shape, keep, holes)) in enumerate(CASES.items()):
        data = make_case(ns, shape, keep, holes, seed=100 + i)
        print(case, shape, "sweeps", data["sweeps"].tolist())
        for k, v in data.items():
            out[f"{case}/{k}"] = v.numpy()
    path = os.path.join(HERE, "corruption.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
