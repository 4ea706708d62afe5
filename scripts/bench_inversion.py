"""GAN inversion step time (dusty_gan_amd.inversion.invert) on the full-width generator: 64x1024, nz 512, ch_base 64,
dusty2, bf16 and fp32, B = 32 and 512, the step captured once and replayed.  Device events around two inversions of
different length: the difference per extra step is the replayed step's time (warm-up, capture and read-back cancel).
    python scripts/bench_inversion.py [--batches 32 512] [--dtypes bf16 fp32] [--steps 200]
Prints one JSON line per configuration."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 512])
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--short", type=int, default=20)
    a = ap.parse_args()
    from dusty_gan_amd.inversion import invert
    from dusty_gan_amd.models import dusty
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
            invert(G, ref, mask, num_step=a.short, gumbel_noise=gum)   # warm-up: shadows, workspaces, clocks
            ms = {}
            for n in (a.short, a.steps):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                invert(G, ref, mask, num_step=n, gumbel_noise=gum)
                e1.record()
                torch.cuda.synchronize()
                ms[n] = e0.elapsed_time(e1)
            step_ms = (ms[a.steps] - ms[a.short]) / (a.steps - a.short)
            print(json.dumps({"what": "inversion step (graph replay)", "arch": "dusty2", "shape": [64, 1024], "nz": 512,
                              "dtype": dt, "B": B, "ms_per_step": round(step_ms, 4),
                              "s_per_1000_steps": round(step_ms, 4), "ms_total": {str(k): round(v, 2) for k, v in ms.items()}}),
                  flush=True)
            del ref, mask
        del G, bb
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
