"""Generate tests/golden/emd_grad.npz: the yardstick of the EMD gradient (dg_emd_grad).

    python tests/golden/make_emd_grad_golden.py [out.npz]

Inputs: the clouds of the twelve paired cases tests/golden/fps_emd.npz already pins to the reference's kernels (named in
tests.emd_grad_util.EMD_GRAD_CASES; the clouds are read from that file, not stored again).  Per case:
    g1_f64 [b,n,3], g2_f64 [b,m,3]   the reference's gradient formula (matchcostgrad1 / matchcostgrad2, grad_cost = 1) in
                                     float64 over the float64 restatement of approxmatch (tests/emd_grad_util.py)
    e_ref1 [b], e_ref2 [b]           per pair, max |same formula over the FLOAT32-order match - float64|: the distance a
                                     float32 evaluation in the reference's order lies from the float64 algorithm
Run on an MI355X with oracle/_ref/libref_fps_emd.so built (oracle/Makefile.ref), the file also carries
    ref_g1, ref_g2                   the same formula over the reference KERNEL's own match matrix, read back from the
                                     buffer ref_emd fills ([i n m + l n + k]); every call runs twice, bit-identical
and e_ref is raised to max(e_ref, |ref - f64|).  meta/live says which it was.  Without the library or a GPU the file
holds the restatement's half only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import emd_grad_util as U  # noqa: E402
from tests.golden_util import load  # noqa: E402


def ref_match(ref, a, b):
    """the reference approxmatch kernel's match buffer [b * n * m] (ref_emd also runs matchcost: its cost is returned too)"""
    import ctypes
    import torch
    vp = ctypes.c_void_p
    B, n, m = a.shape[0], a.shape[1], b.shape[1]
    x1 = torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    x2 = torch.from_numpy(np.ascontiguousarray(b, np.float32)).cuda()
    match = torch.zeros(B * n * m, dtype=torch.float32, device="cuda")
    temp = torch.zeros(32 * (n + m) * 2 + 1024, dtype=torch.float32, device="cuda")   # sized as tests/ref_fps_emd_util.py
    cost = torch.zeros(B, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rc = ref.lib.ref_emd(B, n, m, vp(x1.data_ptr()), vp(x2.data_ptr()), vp(match.data_ptr()), vp(temp.data_ptr()),
                         vp(cost.data_ptr()))
    assert rc == 0, rc
    return match.cpu().numpy(), cost.cpu().numpy()


def main(out_path):
    g = load("fps_emd")
    ref = None
    try:
        import torch
        from tests.ref_fps_emd_util import RefFpsEmd
        if torch.cuda.is_available():
            ref = RefFpsEmd.open()
    except ImportError:
        pass
    d = {"meta/made_by": "tests/golden/make_emd_grad_golden.py", "meta/cases": np.array(U.EMD_GRAD_CASES),
         "meta/live": np.array(ref is not None)}
    if ref is not None:
        d["meta/device"], d["meta/torch"], d["meta/hip"] = torch.cuda.get_device_name(0), torch.__version__, str(torch.version.hip)
    for name in U.EMD_GRAD_CASES:
        a, b = g[f"emd/{name}/a"], g[f"emd/{name}/b"]
        cost64, g1, g2 = U.emd_grads(a, b, np.float64)
        assert np.allclose(cost64, g[f"emd/{name}/f64"], rtol=1e-12, atol=0), name
        _, s1, s2 = U.emd_grads(a, b, np.float32)
        e1, e2 = np.abs(s1 - g1).max((1, 2)), np.abs(s2 - g2).max((1, 2))
        if ref is not None:
            m1, c1 = ref_match(ref, a, b)
            m2, c2 = ref_match(ref, a, b)
            if not (np.array_equal(m1, m2) and np.array_equal(c1, c2)):
                raise SystemExit("the reference's kernel returned two different results for the same input: not written")
            assert np.array_equal(c1, g[f"emd/{name}/ref"]), name   # the kernels fps_emd.npz recorded
            r1, r2 = U.match_grads_ref_layout(a, b, m1)
            d[f"{name}/ref_g1"], d[f"{name}/ref_g2"] = r1, r2
            e1 = np.maximum(e1, np.abs(r1 - g1).max((1, 2)))
            e2 = np.maximum(e2, np.abs(r2 - g2).max((1, 2)))
        d[f"{name}/g1_f64"], d[f"{name}/g2_f64"], d[f"{name}/e_ref1"], d[f"{name}/e_ref2"] = g1, g2, e1, e2
        gmax = max(np.abs(g1).max(), np.abs(g2).max())
        print(name, "max|g|", gmax, "e_ref1 / max|g|", float(e1.max() / gmax), "e_ref2 / max|g|", float(e2.max() / gmax),
              flush=True)
    np.savez_compressed(out_path, **d)
    print("wrote", out_path, os.path.getsize(out_path), "bytes; live reference:", ref is not None)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "emd_grad.npz"))
