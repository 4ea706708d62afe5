"""ctypes door to oracle/_ref/libref_fps_emd.so: the reference's own furthest-point-sampling and earth-mover's-distance
kernels built for gfx950 (oracle/Makefile.ref, oracle/ref_fps_emd_driver.hip).  Used by tests/golden/make_fps_emd_golden.py
to record tests/golden/fps_emd.npz and by tests/test_gpu_metrics.py to replay the same cases live where the library has
been built; everywhere else the fixture alone speaks for the reference."""
import ctypes
import os

import numpy as np
import torch

SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libref_fps_emd.so")


class RefFpsEmd:
    @classmethod
    def open(cls):
        """the library, or None where it has not been built"""
        return cls(SO) if os.path.exists(SO) else None

    def __init__(self, so):
        self.lib = ctypes.CDLL(so)   # links against torch's libraries: torch is imported above
        self.lib.ref_fps.restype = self.lib.ref_emd.restype = ctypes.c_int

    def fps(self, xyz, m):
        """xyz [B,n,3] float32 numpy -> idx [B,m] int32 numpy (temp filled with 1e10 as furthest_point_sampling.cpp does)"""
        vp = ctypes.c_void_p
        B, n = xyz.shape[:2]
        x = torch.from_numpy(np.ascontiguousarray(xyz, np.float32)).cuda()
        temp = torch.full((B, n), 1e10, dtype=torch.float32, device="cuda")
        idx = torch.full((B, m), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc = self.lib.ref_fps(B, n, m, vp(x.data_ptr()), vp(temp.data_ptr()), vp(idx.data_ptr()))
        assert rc == 0, rc
        return idx.cpu().numpy()

    def emd(self, a, b):
        """a [B,n,3], b [B,m,3] float32 numpy -> cost [B] float32 numpy"""
        vp = ctypes.c_void_p
        B, n, m = a.shape[0], a.shape[1], b.shape[1]
        x1 = torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
        x2 = torch.from_numpy(np.ascontiguousarray(b, np.float32)).cuda()
        match = torch.zeros(B * n * m, dtype=torch.float32, device="cuda")
        # the kernel indexes temp by block (32 of them) and reads up to 511 floats past its block's slice before it tests
        # the index (oracle/ref_fps_emd_driver.hip)
        temp = torch.zeros(32 * (n + m) * 2 + 1024, dtype=torch.float32, device="cuda")
        cost = torch.zeros(B, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rc = self.lib.ref_emd(B, n, m, vp(x1.data_ptr()), vp(x2.data_ptr()), vp(match.data_ptr()), vp(temp.data_ptr()),
                              vp(cost.data_ptr()))
        assert rc == 0, rc
        return cost.cpu().numpy()
