"""What each inversion loss reaches: after --steps steps on scripts/bench_inversion.py's targets (dusty2 64x1024, random
weights, uniform random inverse depth with a tenth of the rays dropped), the Chamfer distance of the evaluation's CSV column
(compute_cd between the target's points and the generated ones) and the earth mover's distance on the target's K
furthest-point-sampled rays, divided by K (the "emd" term's own value), as means over the batch - one JSON line per loss.

    python scripts/inversion_terms_table.py [--batch 32] [--steps 1000] [--dtype bf16] [--emd-points 2048]
        [--distance l1 chamfer emd l1+emd]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--emd-points", type=int, default=2048)
    ap.add_argument("--distance", nargs="+", default=["l1", "chamfer", "emd", "l1+emd"])
    a = ap.parse_args()
    from dusty_gan_amd.evaluate_reconstruction import flatten
    from dusty_gan_amd.inversion import EmdState, PointMaps, invert
    from dusty_gan_amd.models import dusty
    from dusty_gan_amd.models.gans.dcgan_eqlr import Generator
    from dusty_gan_amd.utils.lidar import LiDAR, postprocess
    from dusty_gan_amd.utils.metrics.distance import compute_cd, earth_mover_distance
    H, W, B, K = 64, 1024, a.batch, a.emd_points
    lidar = LiDAR(H, W, 0.9, 120.0).use_nominal_angles().to("cuda")
    torch.manual_seed(0)
    bb = Generator(512, {"depth": 1, "confidence": 2}, 64, 512, (H, W), ring=True)
    bb.set_precision({"bf16": torch.bfloat16, "fp32": torch.float32}[a.dtype])
    G = dusty.DUSty2(bb, tau=1, drop_const=-1).to("cuda").eval()
    gum = torch.zeros(1, 1, H, W)
    ref = torch.rand(B, 1, H, W, device="cuda")
    mask = (torch.rand(B, 1, H, W, device="cuda") > 0.1).float()
    ref = ref * mask
    M = EmdState(PointMaps(ref, lidar, 1e-8), K)   # the sample the "emd" term draws on this target
    take = M.idx.long()[:, :, None].expand(-1, -1, 3)
    R = flatten(M.maps.R)
    for dist in a.distance:
        names = tuple(dist.split("+"))
        res = invert(G, ref, mask, num_step=a.steps, distance=names[0] if len(names) == 1 else names, gumbel_noise=gum,
                     lidar=lidar if ("chamfer" in names or "emd" in names) else None, emd_points=K)
        P = flatten(postprocess(res["out"], lidar, tol=1e-8)["points"])
        cd = compute_cd(R, P)
        emd = earth_mover_distance(P.gather(1, take).contiguous(), M.Rs) / K
        print(json.dumps({"what": "inversion terms", "dtype": a.dtype, "B": B, "steps": a.steps, "distance": dist, "emd_points": K,
                          "loss_mean": float(res["loss"].mean()), "cd_mean": float(cd.mean()), "emd_over_K_mean": float(emd.mean()),
                          "kept_rays_mean": float((P.abs().sum(dim=2) > 0).float().sum(dim=1).mean())}), flush=True)


if __name__ == "__main__":
    main()
