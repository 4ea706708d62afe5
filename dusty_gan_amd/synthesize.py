"""Draw scans from a trained generator -- reference: the synthesis mode of demo.py (:188-234, :265-338) as a command.

    python -m dusty_gan_amd.synthesize --model-path <ckpt.pth> --config-path <config.yaml>
        [--num-samples 4] [--latent random|lerp|slerp] [--seed 0] [--tol 0]
        [--zoom 60] [--yaw -45] [--pitch 60] [--save-dir-path .] [--no-images] [--no-bins]

Under <save-dir-path>/synthesis/ it writes
    latents.npy            [n, in_ch]: the latents (Philox(seed) draws, or the lerp / slerp walk between the first two)
    points/<i:06d>.bin     scan i as KITTI records (x, y, z, 0) in metres, float32, the valid pixels in row-major order
    <picture>.png          the demo's pictures, the n samples side by side (make_grid): inv, inv_orig, normal, bev,
                           confidence[_pix|_img], mask[_pix|_img]; inverse depths times the demo's color_scale, turbo
    bev_rgba.png           the bird's-eye view under (zoom, yaw, pitch) with alpha = every channel != 0 (demo.py:325-326)
The EMA generator with fixed Gumbel noise, as the demo sets it up.  Scans are generated, exported and written a batch at a
time; --num-samples is not capped at the demo's 8.  The library is dusty_gan_amd/synthesis.py."""
import argparse
import os
import os.path as osp

COLOR_SCALE = 1 / 0.4   # demo.py's color_scale
BEV_SIZE = 512          # demo.py:321


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--model-path", type=str, required=True)
    parser.add_argument("--config-path", type=str, required=True)
    parser.add_argument("--num-samples", type=int, default=4)
    parser.add_argument("--latent", type=str, default="random", choices=["random", "lerp", "slerp"])
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--tol", type=float, default=0)
    parser.add_argument("--zoom", type=float, default=60, help="metres (demo.py: 1 .. 120)")
    parser.add_argument("--yaw", type=float, default=-45, help="degrees")
    parser.add_argument("--pitch", type=float, default=60, help="degrees")
    parser.add_argument("--save-dir-path", type=str, default=".")
    parser.add_argument("--no-images", action="store_true")
    parser.add_argument("--no-bins", action="store_true")
    args = parser.parse_args(argv)
    if args.num_samples < 1:
        parser.error("--num-samples must be at least 1")
    return args


def picture_name(tag):
    """a picture's file name from its train.image_tags tag: "synth/inv/orig" -> "inv_orig.png" """
    return tag.split("/", 1)[1].replace("/", "_") + ".png"


def pictures_of(out, R, t):
    """[(file name, [B,1|3,H,W] tensor, color, scale)] of demo.py:298-326 for one batch of synthesize()'s dict (with
    normals), plus the bird's-eye view's alpha under the name "bev_alpha" """
    import torch

    from .train import image_tags
    from .utils.render import flatten, render_point_clouds
    out = dict(out)
    out["bev"] = render_point_clouds(flatten(out["points"]), flatten(out["normals"]), L=BEV_SIZE, R=R, t=t)
    if "mask" in out and out["mask"].shape[1] == 2:
        out["mask_prod"] = torch.prod(out["mask"], dim=1, keepdim=True)
    pics = []
    for tag, key, channel, color in image_tags(out):
        if key not in out:
            continue
        x = out[key] if channel is None else out[key][:, channel:channel + 1]
        pics.append((picture_name(tag), x.float().clone(), color, COLOR_SCALE if key in ("depth", "depth_orig") else 1.0))
    pics.append(("bev_alpha", torch.all(out["bev"] != 0.0, dim=1, keepdim=True).float(), False, 1.0))
    return pics


def main(argv=None):
    """-> the directory written (<save-dir-path>/synthesis)"""
    args = parse_args(argv)
    import numpy as np
    import torch

    from . import synthesis as S
    from . import utils
    cfg, G, lidar, device = utils.setup(args.model_path, args.config_path, ema=True, fix_noise=True)
    utils.set_requires_grad(G, False)
    if lidar.angle is None:
        raise RuntimeError(f"no angle grid: {lidar.angle_file!r} does not exist (utils/lidar.py:120)")
    out_dir = osp.join(args.save_dir_path, "synthesis")
    os.makedirs(out_dir, exist_ok=True)
    written = []
    n, B = args.num_samples, int(cfg.solver.batch_size)
    latents = S.sample_latents(cfg, device, n, args.latent, args.seed)
    np.save(osp.join(out_dir, "latents.npy"), latents.cpu().numpy())
    written.append(osp.join(out_dir, "latents.npy"))
    images = not args.no_images
    if images:
        R, t = (v.to(device) for v in S.view(args.zoom, args.yaw, args.pitch))
    pictures = {}   # file name -> ([tensors, a batch each], color, scale)
    for i in range(0, n, B):
        out = S.synthesize(cfg, G, lidar, latents[i:i + B], tol=args.tol, normals=images)
        if not args.no_bins:
            records, counts = S.export_points(out["depth"], lidar, tol=args.tol, from_tanh=False)
            written += S.write_bins(records, counts, osp.join(out_dir, "points"), first_index=i)
        if images:
            for name, x, color, scale in pictures_of(out, R, t):
                pictures.setdefault(name, ([], color, scale))[0].append(x)
    if images:
        from PIL import Image

        from .utils.render import image_grid
        grids = {name: image_grid(torch.cat(xs, dim=0), color=color, scale=scale).cpu().numpy()
                 for name, (xs, color, scale) in pictures.items()}
        alpha = grids.pop("bev_alpha")[..., :1]
        grids["bev_rgba.png"] = np.concatenate([grids["bev.png"], alpha], axis=2)
        for name, grid in grids.items():
            path = osp.join(out_dir, name)
            Image.fromarray(grid).save(path)
            written.append(path)
    for path in written:
        print("wrote:", path)
    return out_dir


if __name__ == "__main__":
    main()
