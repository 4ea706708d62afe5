"""Guarded device buffers for the per-element GPU tests (tests/test_gpu_image_exact.py, tests/test_gpu_net_end.py): a kernel's
output starts as sentinels between two guards of sentinels, an accumulator is a guarded plain buffer or a slice of the registered
arena.  SENTINEL and GUARD are tests/image_exact_util.py's."""
import math

import torch

from tests import image_exact_util as U

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
MODES = ["plain", "arena"]


def dev(t, dtype=F32):
    return t.to(dtype).contiguous().to(DEV)


class Owned:
    """a kernel's output: `shape` elements that start as sentinels (or as `fill`: an accumulator) between two guards"""

    def __init__(self, shape, dtype=F32, fill=None):
        n = math.prod(shape)
        self.buf = torch.full((n + 2 * U.GUARD,), U.SENTINEL, dtype=dtype, device=DEV)
        self.t = self.buf[U.GUARD:U.GUARD + n].view(shape)
        if fill is not None:
            self.t.fill_(fill)
        self.ptr = self.t.data_ptr()

    def done(self, what, written=True):
        """the guards are intact; every owned element was written (or, for a refused launch, none was)"""
        torch.cuda.synchronize()
        b = self.buf.float().cpu()
        g = U.GUARD
        assert bool((b[:g] == U.SENTINEL).all()) and bool((b[-g:] == U.SENTINEL).all()), f"{what}: a guard was overwritten"
        own = b[g:-g] == U.SENTINEL
        if written:
            assert not bool(own.any()), f"{what}: {int(own.sum())} owned elements were never written, first at {int(own.nonzero()[0])}"
        else:
            assert bool(own.all()), f"{what}: a refused launch wrote {int((~own).sum())} elements"
        return self.t.cpu()


class Acc:
    """accumulators that start at zero (or a preloaded value): guarded plain buffers, or slices of the registered arena"""

    def __init__(self, L, mode):
        self.L, self.mode, self.owned = L, mode, []
        if mode == "arena":
            L.AccArena.begin(DEV)

    def take(self, n, preload=0.0):
        if self.mode == "arena":
            t = self.L.AccArena.take(n, DEV)
            assert t is not None
            if preload:
                t.fill_(preload)
            return t
        o = Owned((n,), fill=preload)
        self.owned.append(o)
        return o.t

    def done(self, what):
        torch.cuda.synchronize()
        for o in self.owned:
            o.done(what)
