"""GAN inversion step time (dusty_gan_amd.inversion.invert) on the full-width generator: 64x1024, nz 512, ch_base 64,
dusty2, bf16 and fp32, B = 32 and 512, the step captured once and replayed.  Device events around two inversions of
different length: the difference per extra step is the replayed step's time (warm-up, capture and read-back cancel).
    python scripts/bench_inversion.py [--batches 32 512] [--dtypes bf16 fp32] [--steps 200] [--distance l1 chamfer l1+chamfer emd l1+emd] [--emd-points 1024 2048]
--nn N: also time dg_chamfer_nn against dg_chamfer_paired (the index-free floor) on B = 32 pairs of N-point clouds
(--batches or --dtypes with no value: skip the step benchmark and time the search only).
--num-code N [N ...] with --composition-layer L [L ...]: the multi-code inversion (mGANprior) at every (N, L); N = 1 is the
single-code step.  --compose: time dg_feat_compose / dg_feat_compose_bwd alone at the chosen (B, N, L, dtype) and report their
achieved bytes per second (operands streamed once: the algorithmic traffic).
Prints one JSON line per configuration."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def gpu_clock():
    """the shader clock rocm-smi reports right now (a read-only query), or None"""
    import re
    import subprocess
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        m = re.search(r"sclk clock level: \d+: \((\d+)Mhz\)", out)
        return int(m.group(1)) if m else None
    except Exception:
        return None


def bench_nn(n, B=32, reps=10, warm=3):
    """dg_chamfer_nn against dg_chamfer_paired on the same B pairs of n-point clouds, the two alternating: `warm` untimed
    rounds, then `reps` rounds of one event-timed launch each; median and minimum per kernel, and the shader clock read
    right after the timed rounds"""
    from dusty_gan_amd import _lib as L
    lib = L.lib()
    gen = torch.Generator(device="cuda").manual_seed(0)
    a = torch.rand(B, n, 3, device="cuda", generator=gen)
    b = torch.rand(B, n, 3, device="cuda", generator=gen)
    dist = torch.empty(B, n, device="cuda")
    idx = torch.empty(B, n, dtype=torch.int32, device="cuda")
    mean = torch.empty(B, device="cuda")

    def nn():
        L.check(lib.dg_chamfer_nn(L.ptr(a), 3 * n, 3, 1, n, L.ptr(b), 3 * n, 3, 1, n, B, L.ptr(dist), L.ptr(idx), L.stream_ptr()),
                "dg_chamfer_nn")

    def paired():
        L.check(lib.dg_chamfer_paired(L.ptr(a), n, L.ptr(b), n, B, L.ptr(mean), L.stream_ptr()), "dg_chamfer_paired")

    fns = (("dg_chamfer_paired", paired), ("dg_chamfer_nn", nn))
    times = {name: [] for name, _ in fns}
    for r in range(warm + reps):
        for name, fn in fns:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= warm:
                times[name].append(e0.elapsed_time(e1))
    clock = gpu_clock()
    res = {name: round(sorted(t)[len(t) // 2], 3) for name, t in times.items()}
    res["min"] = {name: round(min(t), 3) for name, t in times.items()}
    res["sclk_mhz"] = clock
    res["ratio"] = round(res["dg_chamfer_nn"] / res["dg_chamfer_paired"], 3)
    res["tflops_nn"] = round(8.0 * B * n * n / (res["dg_chamfer_nn"] * 1e-3) / 1e12, 1)
    print(json.dumps({"what": "nearest-neighbour search, ms", "B": B, "n": n, **res}), flush=True)


def bench_compose(B, N, layer, dt, reps=20, warm=5):
    """the two composition kernels on full-width feature maps of layer `layer` (64x1024, channels 512 / 256 / 128 / 64):
    median event time of one launch and the algorithmic bytes (forward: N maps read, one written; backward: g once per code - it
    is re-read from the caches, counted once per scan here - N maps read, N written) per second"""
    from dusty_gan_amd import _lib as L
    lib = L.lib()
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[dt]
    es = 2 if dt == "bf16" else 4
    P, C = (4 * 64) << (2 * layer), 512 >> layer
    a = torch.randn(B * N, P, C, device="cuda").to(dtype)
    g = torch.randn(B, P, C, device="cuda").to(dtype)
    alpha = torch.full((B, N, C), 1.0 / N, device="cuda")
    out, dpre, dalpha = torch.empty_like(g), torch.empty_like(a), torch.empty_like(alpha)
    nchunk = max(1, min(64, P, (P * C * es) // 65536))
    parts = torch.zeros(B * N * nchunk * C, device="cuda")
    tickets = torch.zeros(B * N, dtype=torch.int32, device="cuda")
    code = L.dtype_code(dtype)

    def fwd():
        L.check(lib.dg_feat_compose(L.ptr(a), L.ptr(alpha), L.ptr(out), code, B, N, P, C, L.stream_ptr()), "dg_feat_compose")

    def bwd():
        L.check(lib.dg_feat_compose_bwd(L.ptr(g), L.ptr(a), L.ptr(alpha), L.ptr(dpre), L.ptr(dalpha), L.ptr(parts), L.ptr(tickets),
                                        nchunk, code, B, N, P, C, L.stream_ptr()), "dg_feat_compose_bwd")

    nbytes = {"dg_feat_compose": (B * N + B) * P * C * es, "dg_feat_compose_bwd": (2 * B * N + B) * P * C * es}
    for name, fn in (("dg_feat_compose", fwd), ("dg_feat_compose_bwd", bwd)):
        ts = []
        for r in range(warm + reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= warm:
                ts.append(e0.elapsed_time(e1))
        med = sorted(ts)[len(ts) // 2]
        print(json.dumps({"what": name, "dtype": dt, "B": B, "N": N, "layer": layer, "P": P, "C": C, "ms": round(med, 4),
                          "min_ms": round(min(ts), 4), "bytes": nbytes[name], "TB_per_s": round(nbytes[name] / (med * 1e-3) / 1e12, 3),
                          "sclk_mhz": gpu_clock()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="*", default=[32, 512], help="no value: skip the step benchmark")
    ap.add_argument("--dtypes", nargs="*", default=["bf16", "fp32"], help="no value: skip the step benchmark")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--short", type=int, default=20)
    ap.add_argument("--distance", nargs="+", default=["l1"], help="'+'-joined terms out of l1, l2, chamfer, emd; one run each")
    ap.add_argument("--emd-points", type=int, nargs="+", default=[2048], help="K of the emd term; one run each")
    ap.add_argument("--nn", type=int, default=0)
    ap.add_argument("--num-code", type=int, nargs="+", default=[1], help="latents per scan; above 1: multi-code inversion")
    ap.add_argument("--composition-layer", type=int, nargs="+", default=[], help="0..3, with --num-code above 1")
    ap.add_argument("--compose", action="store_true", help="time the two composition kernels alone instead of the step")
    a = ap.parse_args()
    combos = [(n, l) for n in a.num_code for l in (a.composition_layer if n > 1 else [None])]
    if a.compose:
        for dt in a.dtypes:
            for B in a.batches:
                for n, l in combos:
                    if n > 1:
                        bench_compose(B, n, l, dt)
        return
    if a.nn:
        bench_nn(a.nn)
    from dusty_gan_amd.inversion import invert
    from dusty_gan_amd.models import dusty
    from dusty_gan_amd.utils.lidar import LiDAR
    lidar = LiDAR(64, 1024, 0.9, 120.0).use_nominal_angles().to("cuda")
    from dusty_gan_amd.models.gans.dcgan_eqlr import Generator
    for dt in a.dtypes:
        dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[dt]
        torch.manual_seed(0)
        bb = Generator(512, {"depth": 1, "confidence": 2}, 64, 512, (64, 1024), ring=True)
        bb.set_precision(dtype)
        G = dusty.DUSty2(bb, tau=1, drop_const=-1).to("cuda").eval()
        gum = torch.zeros(1, 1, 64, 1024)
        for B in a.batches:
            ref = torch.rand(B, 1, 64, 1024, device="cuda")
            mask = (torch.rand(B, 1, 64, 1024, device="cuda") > 0.1).float()
            runs = ((d, k, c) for d in a.distance for k in (a.emd_points if "emd" in d.split("+") else [None]) for c in combos)
            for dist, K, (ncode, layer) in runs:
                names = tuple(dist.split("+"))
                kw = dict(gumbel_noise=gum, distance=names[0] if len(names) == 1 else names,
                          lidar=lidar if ("chamfer" in names or "emd" in names) else None)
                if K is not None:
                    kw.update(emd_points=K)
                if ncode > 1:
                    kw.update(num_code=ncode, composition_layer=layer)
                invert(G, ref, mask, num_step=a.short, **kw)   # warm-up: shadows, workspaces, clocks
                ms = {}
                for n in (a.short, a.steps):
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    invert(G, ref, mask, num_step=n, **kw)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[n] = e0.elapsed_time(e1)
                step_ms = (ms[a.steps] - ms[a.short]) / (a.steps - a.short)
                print(json.dumps({"what": "inversion step (graph replay)", "arch": "dusty2", "shape": [64, 1024], "nz": 512,
                                  "dtype": dt, "B": B, "distance": dist, "emd_points": K, "num_code": ncode, "composition_layer": layer, "sclk_mhz": gpu_clock(), "ms_per_step": round(step_ms, 4),
                                  "s_per_1000_steps": round(step_ms, 4),
                                  "ms_total": {str(k): round(v, 2) for k, v in ms.items()}}), flush=True)
            del ref, mask
        del G, bb
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
