"""Record tests/golden/thin_plans.json: what dg_conv_plan / dg_wgrad_plan / dg_wgrad_has_sample_map answer for the thin
family's descriptors (tests/test_thin_pick_cpu.py reads it back and asserts equality).

    python tests/golden/make_thin_plans.py [--lib path/to/libdustygan_hip.so]

Run it against the library whose selection is the yardstick (a build of the commit BEFORE a change to csrc/conv_thin.hip;
default: the in-tree build).  No GPU is needed: nothing is launched, no pointer is dereferenced - they are 256-byte-aligned
integers, except one deliberately 8-byte-aligned `a`.

Every row goes through DG_FORCE_THIN.  It is recorded once more under DG_FORCE_AUTO where the recording library answers
with the thin family there too (no other family claims the shape, and the plan needs no device)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from dusty_gan_amd import _lib as L  # noqa: E402
from tests.test_thin_pick_cpu import TABLE, answer, fill, record  # noqa: E402

IN, OUT, W, AUX, BIAS, MASK, SUMS, DW, G = (0x10000000 + 0x1000000 * i for i in range(9))
BF, F32, X2 = L.DG_BF16, L.DG_F32, L.DG_BF16X2


def conv(mode, B, Hc, Wc, K, N, dt, in_s, out_s, **kw):
    p = L.DgConv()
    p.mode, p.adj, p.ring, p.B, p.Hc, p.Wc, p.K, p.N = mode, 0, 1, B, Hc, Wc, K, N
    p.in_, p.out, p.w = IN, OUT, W
    p.in_sb, p.in_sp, p.in_sk = in_s
    p.out_sb, p.out_sp, p.out_sn = out_s
    p.w_st, p.w_sn, p.w_sk = N * K, K, 1          # the T shadow [tap][n][k]
    p.scale, p.epi = 0.25, L.EPI_LINEAR
    p.in_dtype = p.out_dtype = p.w_dtype = dt
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def s2(B, Hc, Wc, K, N=64, dt=BF, cp=None, **kw):
    """Down1 forward / Head backward-data: a cp-channel pixel-major fine image -> N channels, NHWC"""
    cp = K if cp is None else cp
    return conv(L.MODE_S2, B, Hc, Wc, K, N, dt, (4 * Hc * Wc * cp, cp, 1), (Hc * Wc * N, N, 1), **kw)


def up(B, Hc, Wc, K, N, dt=BF, planar=False, **kw):
    """Head forward / Down1 backward-data: NHWC K channels -> N channels, fine grid, NHWC or (Head) planar fp32"""
    HW = 4 * Hc * Wc
    p = conv(L.MODE_UP, B, Hc, Wc, K, N, dt, (Hc * Wc * K, K, 1), (N * HW, 1, HW) if planar else (HW * N, N, 1), **kw)
    if planar:
        p.out_dtype = F32
    return p


def wgrad(wmode, B, Hc, Wc, Ci, Co, dt, a_s, g_s, **kw):
    p = L.DgWgrad()
    p.wmode, p.ring, p.B, p.Hc, p.Wc, p.Ci, p.Co = wmode, 1, B, Hc, Wc, Ci, Co
    p.a, p.g, p.dw, p.scale = IN, G, DW, 0.125
    p.a_sb, p.a_sp, p.a_sc = a_s
    p.g_sb, p.g_sp, p.g_sc = g_s
    p.a_dtype = p.g_dtype = dt
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def wg0(B, Hc, Wc, Ci=2, Co=64, dt=BF, **kw):
    """Down1: the fine Ci-channel image and the coarse Co-channel gradient, both NHWC"""
    return wgrad(0, B, Hc, Wc, Ci, Co, dt, (4 * Hc * Wc * Ci, Ci, 1), (Hc * Wc * Co, Co, 1), **kw)


def wg1(B, Hc, Wc, Co, cp=None, Ci=64, dt=BF, **kw):
    """Head: the coarse Ci-channel input NHWC; the fine gradient pixel-major padded to cp channels, or (cp None) planar"""
    HW = 4 * Hc * Wc
    return wgrad(1, B, Hc, Wc, Ci, Co, dt, (Hc * Wc * Ci, Ci, 1), (HW * cp, cp, 1) if cp else (Co * HW, 1, HW), **kw)


def rows():
    r = []
    add = lambda name, p, **kw: r.append((name, p, kw))
    # ---- conv, MODE_S2
    add("s2 bf16 cp2 K2: thin_s2_mfma", s2(2, 4, 64, 2))
    add("s2 bf16 cp4 K3: thin_s2_mfma", s2(2, 4, 64, 3, cp=4))
    add("s2 bf16 mask_out + EPI_LRELU", s2(2, 4, 64, 2, epi=L.EPI_LRELU, mask_out=MASK))
    add("s2 bf16 mask_in + EPI_MASK", s2(2, 4, 64, 2, epi=L.EPI_MASK, aux=AUX, mask_in=MASK))
    add("s2 bf16 Hc 2: thin_smallk", s2(2, 2, 64, 2))
    add("s2 bf16 Wc 32: refused", s2(2, 4, 32, 2))
    add("s2 bf16 Wc 96: thin_s2_mfma's multiple of 32, not the family's of 64", s2(2, 4, 96, 2))
    add("s2 bf16 dbias_rows capped", s2(32, 32, 512, 2))
    add("s2 bf16 dbias_rows 768 uncapped", s2(48, 32, 64, 2))
    add("s2 bf16 dbias_rows one block below the cap", s2(26, 59, 64, 2))
    add("s2 bf16 dbias, bias_mod 64", s2(2, 8, 64, 2, dbias=BIAS, bias_mod=64))
    add("s2 bf16 dbias, bias_mod 128: thin_smallk", s2(2, 8, 64, 2, dbias=BIAS, bias_mod=128))
    add("s2 bf16 bias with scale 0: thin_smallk", s2(2, 4, 64, 2, bias=BIAS, bias_mod=64, scale=0.0))
    add("s2 bf16 N 128: thin_smallk", s2(2, 4, 64, 2, N=128))
    add("s2 bf16 K 3 on two channels: thin_smallk", s2(2, 4, 64, 3, cp=3))
    add("s2 fp32 K2 N128: thin_smallk<2>", s2(2, 4, 64, 2, N=128, dt=F32))
    add("s2 fp32 K4 N128: thin_smallk<4>", s2(2, 4, 64, 4, N=128, dt=F32))
    add("s2 fp32 K5: refused", s2(2, 4, 64, 5, N=128, dt=F32))
    add("s2 fp32 nscale: refused", s2(2, 4, 64, 2, N=128, dt=F32, nscale=AUX))
    add("s2 fp32 dbias, bias_mod 64 < N 128: refused", s2(2, 4, 64, 2, N=128, dt=F32, dbias=BIAS, bias_mod=64))
    add("s2 no ring: refused", s2(2, 4, 64, 2, ring=0))
    # ---- conv, MODE_UP
    for n in (1, 2, 3):
        add(f"up bf16 K64 N{n}: thin_up_mfma", up(2, 8, 64, 64, n))
    add("up bf16 K64 N4: refused", up(2, 8, 64, 64, 4))
    add("up bf16 K64 N1 planar fp32 Hc20 Wc128: sum_parts 6", up(2, 20, 128, 64, 1, planar=True))
    add("up bf16 K64 N1 bf16 out Hc20 Wc128: sum_parts 0", up(2, 20, 128, 64, 1))
    add("up bf16 K64 N2 planar fp32: sum_parts 0", up(2, 20, 128, 64, 2, planar=True))
    add("up bf16 K128 N2: thin_smalln", up(2, 8, 64, 128, 2))
    add("up bf16 K192 N3: thin_smalln, over 64 KiB of LDS (the launch refuses)", up(2, 8, 64, 192, 3))
    add("up fp32 K64 N2: thin_smalln", up(2, 8, 64, 64, 2, dt=F32))
    add("up adjoint bf16 K64 N2: thin_up_mfma", up(2, 8, 64, 64, 2, adj=1))
    add("up x2 input, fp32 weights, K64: thin_up_mfma<X2>", up(2, 8, 64, 64, 2, dt=F32, in_dtype=X2))
    add("up x2 input, in_sb % 64 != 0: refused", up(2, 8, 64, 64, 2, dt=F32, in_dtype=X2, in_sb=8 * 64 * 64 + 8))
    add("up x2 input K128: thin_smalln<X2>", up(2, 8, 64, 128, 2, dt=F32, in_dtype=X2))
    add("up bf16 Wc 96: refused", up(2, 8, 96, 64, 2))
    add("up bf16 dbias: refused", up(2, 8, 64, 64, 2, dbias=BIAS, bias_mod=2))
    # ---- wgrad, wmode 0
    add("wg0 bf16 B3 Hc4 Wc64: down-mfma, 6 splits", wg0(3, 4, 64))
    for wc in (128, 256, 512, 1024, 2048):
        add(f"wg0 bf16 Wc{wc}: down-mfma", wg0(2, 4, wc))
    add("wg0 bf16 Wc4096: off 2 Wc <= 4096", wg0(2, 4, 4096))
    add("wg0 bf16 B64 Hc32: 4 rows per block", wg0(64, 32, 64))
    add("wg0 bf16 B64 Hc34: 2 rows per block", wg0(64, 34, 64))
    add("wg0 bf16 B4096 Hc64: 65536 blocks, the most the workspace form takes", wg0(4096, 64, 64))
    add("wg0 bf16 B4096 Hc66: more blocks than that, no workspace form", wg0(4096, 66, 64))
    add("wg0 bf16 misaligned a: VALU", wg0(3, 4, 64, a=IN + 8))
    add("wg0 bf16 g_mod: down-mfma has the sample map", wg0(3, 4, 64, g_mod=2))
    add("wg0 bf16 Hc3: VALU", wg0(3, 3, 64))
    add("wg0 fp32 B Hc 12: VALU, 12 splits", wg0(3, 4, 64, dt=F32))
    add("wg0 fp32 B Hc 1280: VALU, 1024 splits", wg0(40, 32, 64, dt=F32))
    add("wg0 fp32 g_mod: no workspace form, no map", wg0(3, 4, 64, dt=F32, g_mod=2))
    add("wg0 fp32 Ci4 Co128", wg0(3, 4, 64, Ci=4, Co=128, dt=F32))
    add("wg0 fp32 Ci8: refused", wg0(3, 4, 64, Ci=8, Co=128, dt=F32))
    add("wg0 fp32 Co96: refused", wg0(3, 4, 64, Co=96, dt=F32))
    add("wg0 fp32 overwrite", wg0(3, 4, 64, dt=F32), accumulate=0)
    # ---- wgrad, wmode 1
    add("wg1 bf16 cp2 Co1: up-mfma, one pass", wg1(2, 4, 64, 1, 2))
    add("wg1 bf16 cp2 Co2: up-mfma, one pass", wg1(2, 4, 64, 2, 2))
    add("wg1 bf16 cp4 Co3 Wc64: both pairs in one pass", wg1(2, 4, 64, 3, 4))
    add("wg1 bf16 cp4 Co4 Wc64: both pairs in one pass", wg1(2, 4, 64, 4, 4))
    add("wg1 bf16 cp4 Co2 Wc64: one pair", wg1(2, 4, 64, 2, 4))
    add("wg1 bf16 cp4 Co3 Wc2048: one pair per pass, no workspace form", wg1(1, 2, 2048, 3, 4))
    add("wg1 bf16 cp4 Co4 Wc2048: one pair per pass, no workspace form", wg1(1, 2, 2048, 4, 4))
    add("wg1 bf16 cp2 Co2 Wc1024: over 64 KiB of LDS", wg1(1, 2, 1024, 2, 2))
    add("wg1 bf16 cp2 Co3: more heads than channels, VALU", wg1(2, 4, 64, 3, 2))
    add("wg1 bf16 Hc3: VALU", wg1(2, 3, 64, 2, 2))
    add("wg1 bf16 Hc1: VALU", wg1(2, 1, 64, 2, 2))
    add("wg1 bf16 g_mod: no map", wg1(2, 4, 64, 2, 2, g_mod=1))
    add("wg1 fp32 Ci64 Co3 planar", wg1(2, 4, 64, 3, dt=F32))
    add("wg1 fp32 Ci128 Co3 planar: two passes", wg1(2, 4, 64, 3, Ci=128, dt=F32))
    add("wg1 fp32 Ci96: refused", wg1(2, 4, 64, 3, Ci=96, dt=F32))
    add("wg1 fp32 Co5: refused", wg1(2, 4, 64, 5, dt=F32))
    add("wg1 fp32 Wc4096: the staged rows pass 160 KiB, refused", wg1(1, 2, 4096, 3, dt=F32))
    add("wgrad wmode 2: refused", wgrad(2, 2, 4, 64, 64, 4, F32, (64, 0, 1), (4, 0, 1)))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="the recording library (default: the in-tree build)")
    a = ap.parse_args()
    if a.lib:
        L.LIB_PATH = os.path.abspath(a.lib)
    lib = L.lib()
    out = []
    for name, p, kw in rows():
        conv_pass = isinstance(p, L.DgConv)
        for force in (L.DG_FORCE_THIN, L.DG_FORCE_AUTO):
            row = {"name": name, "pass": "conv" if conv_pass else "wgrad", "force": force,
                   "desc": record(type(p), p)}
            if not conv_pass:
                row["accumulate"] = kw.get("accumulate", 1)
            assert record(type(p), fill(type(p), row["desc"])) == row["desc"]
            e = row["expect"] = answer(L, lib, row)
            thin = e.get("family") == L.DG_CONV_FAMILY_THIN or e.get("variant") in (L.DG_WGRAD_VARIANT_THIN, L.DG_WGRAD_VARIANT_THIN_MFMA)
            if force == L.DG_FORCE_THIN or (e["rc"] == L.DG_OK and thin):
                out.append(row)
    with open(TABLE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in out) + "\n]\n")
    print(len(out), "rows ->", TABLE, "from", L.LIB_PATH)
    for r in out:
        print(r["force"], r["name"], r["expect"])


if __name__ == "__main__":
    main()
