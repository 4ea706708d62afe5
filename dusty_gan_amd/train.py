"""python -m dusty_gan_amd.train [key=value ...] [--out-dir DIR]

The reference's train.py (:37-190): the training loop around `Trainer.step` with its logs.  The arguments are its Hydra
overrides (`dataset=kitti_odometry`, `model=dusty2_dcgan_eqlr`, `solver.batch_size=32`, `resume=models/checkpoint_X.pth`
...), composed by utils.config.load_config; a relative `dataset.root` or `resume` is resolved against the invoking
directory.  Under DIR (default outputs/<date>/<time>, like Hydra's run directory):
    .hydra/config.yaml                    the composed config (what evaluate_reconstruction --config-path and utils.setup read)
    models/checkpoint_<step:010d>.pth     every solver.checkpoint.save_model iterations and at the end
    scalars.jsonl                         one object per logged iteration: iteration, step (= images seen), the step's
                                          scalars every save_stats iterations, validation scores as score/<key> every test
    images/<tag>/<step:010d>.png          every save_image iterations, the reference's tags (real/* once, at step 1)
If torch.utils.tensorboard imports, the same scalars and images also go to a SummaryWriter in DIR.  The pictures are made
on the GPU (utils/render.py: the bird's-eye view, the colour-mapped grids); PIL only encodes the PNG.

Under a launcher (RANK / WORLD_SIZE / LOCAL_RANK, e.g. python -m torch.distributed.run --nproc-per-node N -m
dusty_gan_amd.train ...) every process joins the process group and trains its share of the batch; rank 0 alone logs,
validates and saves.
"""
import argparse
import datetime
import json
import os
import os.path as osp
import sys

SCALE = 1 / 0.4  # for visibility (train.py:25)
REAL_TAGS = ("real/inv", "real/inv_aug", "real/normal", "real/bev")


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m dusty_gan_amd.train", description=__doc__.split("\n\n")[1],
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("overrides", nargs="*", metavar="key=value", help="Hydra-style overrides of the config tree")
    p.add_argument("--out-dir", type=str, default=None, help="run directory (default: outputs/<date>/<time>)")
    args = p.parse_args(argv)
    for ov in args.overrides:
        if "=" not in ov or ov.startswith("="):
            p.error(f"not a key=value override: {ov!r}")
    return args


def default_out_dir(now=None):
    now = now or datetime.datetime.now()
    return osp.join("outputs", now.strftime("%Y-%m-%d"), now.strftime("%H-%M-%S"))


def compose(overrides, cwd=None):
    """the run's config: load_config plus train.py:179-182 (paths relative to the invoking directory)"""
    from .utils.config import load_config
    cwd = cwd or os.getcwd()
    cfg = load_config(list(overrides))
    root = cfg.dataset.get("root")
    if root and not osp.isabs(str(root)):
        cfg.dataset.root = osp.join(cwd, str(root))
    if cfg.resume is not None and not osp.isabs(str(cfg.resume)):
        cfg.resume = osp.join(cwd, str(cfg.resume))
    return cfg


def local_config(cfg, gpu, ngpus):
    """train.py:53-66: this worker's share of the batch"""
    assert cfg.solver.batch_size % ngpus == 0
    local_batch_size = int(cfg.solver.batch_size / ngpus)
    assert local_batch_size % cfg.solver.num_accumulation == 0
    local_batch_size = int(local_batch_size / cfg.solver.num_accumulation)
    return {"gpu": gpu, "ngpus": ngpus, "batch_size": local_batch_size,
            "num_workers": int((cfg.num_workers + ngpus - 1) / ngpus)}


def prepare_out_dir(cfg, out_dir):
    """create the run directory's layout and write the composed config; returns the absolute directory"""
    from .utils.config import dump_config
    out_dir = osp.abspath(out_dir)
    for sub in (".hydra", "models", "images"):
        os.makedirs(osp.join(out_dir, sub), exist_ok=True)
    dump_config(cfg, osp.join(out_dir, ".hydra", "config.yaml"))
    return out_dir


def image_tags(out):
    """[(tag, key, channel slice or None, color)] of train.py:125-151 for a generate() result"""
    tags = []
    if "depth" in out:
        tags += [("synth/inv", "depth", None, True), ("synth/normal", "normals", None, False), ("synth/bev", "bev", None, False)]
    if "depth_orig" in out:
        tags.append(("synth/inv/orig", "depth_orig", None, True))
    if "confidence" in out:
        if out["confidence"].shape[1] == 2:
            tags += [("synth/confidence/pix", "confidence", 0, True), ("synth/confidence/img", "confidence", 1, True)]
        elif out["confidence"].shape[1] == 1:
            tags.append(("synth/confidence", "confidence", 0, True))
    if "mask" in out:
        if out["mask"].shape[1] == 2:
            tags += [("synth/mask/pix", "mask", 0, False), ("synth/mask/img", "mask", 1, False), ("synth/mask", "mask_prod", None, False)]
        elif out["mask"].shape[1] == 1:
            tags.append(("synth/mask", "mask", None, False))
    return tags


class RunLog:
    """rank 0's logs: scalars.jsonl, images/<tag>/<step>.png and, where it imports, a TensorBoard SummaryWriter"""

    def __init__(self, out_dir):
        self.out_dir = out_dir
        self.scalars = open(osp.join(out_dir, "scalars.jsonl"), "a")
        try:
            from torch.utils.tensorboard import SummaryWriter
            self.writer = SummaryWriter(out_dir)
        except ImportError:
            self.writer = None

    def add_scalars(self, iteration, step, values):
        self.scalars.write(json.dumps({"iteration": iteration, "step": step, **{k: float(v) for k, v in values.items()}}) + "\n")
        self.scalars.flush()
        if self.writer is not None:
            for key, scalar in values.items():
                self.writer.add_scalar(key, scalar, step)

    def add_image(self, tensor, tag, step, color=True, scale=1.0):
        """log_imgs (train.py:28-34)"""
        from PIL import Image

        from .utils.render import image_grid
        grid = image_grid(tensor, color=color, scale=scale).cpu().numpy()
        path = osp.join(self.out_dir, "images", tag, "{:010d}.png".format(int(step)))
        os.makedirs(osp.dirname(path), exist_ok=True)
        Image.fromarray(grid).save(path)
        if self.writer is not None:
            self.writer.add_image(tag, grid, step, dataformats="HWC")

    def close(self):
        self.scalars.close()
        if self.writer is not None:
            self.writer.close()


def bird_eye_view(out, device):
    import torch

    from .utils.render import flatten, render_point_clouds
    return render_point_clouds(flatten(out["points"]), flatten(out["normals"]),
                               t=torch.tensor([0, 0, 0.5], device=device, dtype=torch.float32))


def log_real_preview(log, trainer):
    """train.py:85-97"""
    inv_real, mask_real = trainer.fetch_reals(next(trainer.loader))
    real = trainer.postprocess({"depth": inv_real, "mask": mask_real})
    real_aug = trainer.postprocess({"depth": trainer.A(inv_real)})
    log.add_image(real["depth"], "real/inv", 1, scale=SCALE)
    log.add_image(real_aug["depth"], "real/inv_aug", 1, scale=SCALE)
    if "normals" in real:   # (no angle grid, no point map: utils.lidar.postprocess)
        log.add_image(real["normals"], "real/normal", 1, color=False)
        log.add_image(bird_eye_view(real, trainer.device), "real/bev", 1, color=False)


def log_synth_images(log, trainer, step):
    """train.py:123-151"""
    import torch
    out = dict(trainer.generate())
    if "points" in out:
        out["bev"] = bird_eye_view(out, trainer.device)
    if "mask" in out and out["mask"].shape[1] == 2:
        out["mask_prod"] = torch.prod(out["mask"], dim=1, keepdim=True)
    for tag, key, channel, color in image_tags(out):
        if key not in out:
            continue
        x = out[key] if channel is None else out[key][:, channel:channel + 1]
        log.add_image(x, tag, step, color=color, scale=SCALE if key in ("depth", "depth_orig") else 1.0)


def init_distributed(cfg):
    """(rank, world, local rank): joins the launcher's process group when there is one (as bench.py's ranks do)"""
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
        os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
        backend = str(cfg.dist_backend)
        ndev = torch.cuda.device_count()
        if backend == "nccl" and ndev < world:
            raise SystemExit(f"WORLD_SIZE={world} but this node has {ndev} GPU(s); RCCL needs one device per rank")
        local_rank = local_rank % max(ndev, 1)
        torch.cuda.set_device(local_rank)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    return rank, world, local_rank


def main(argv=None):
    args = parse_args(argv)
    cfg = compose(args.overrides)
    import torch
    import torch.distributed as dist
    import yaml

    from .trainers import dcgan_amp
    rank, world, local_rank = init_distributed(cfg)
    out_dir = osp.abspath(args.out_dir or default_out_dir())
    log = None
    if rank == 0:
        print(yaml.safe_dump(json.loads(json.dumps(cfg)), sort_keys=False))
        out_dir = prepare_out_dir(cfg, out_dir)
    trainer = dcgan_amp.Trainer(cfg, local_config(cfg, local_rank, world))

    total_img = cfg.solver.total_kimg * 1000
    total_iteration = int(total_img / cfg.solver.batch_size)
    ckpt = cfg.solver.checkpoint
    models_dir = osp.join(out_dir, "models")

    def iteration_to_imgs(i):
        return int(i * cfg.solver.batch_size)

    if rank == 0:
        log = RunLog(out_dir)
        log_real_preview(log, trainer)
        print("iteration start:", trainer.start_iteration + 1)
        print("iteration total:", total_iteration)

    start, final = trainer.start_iteration + 1, None
    try:
        for i in range(start, total_iteration + 1):
            scalars = trainer.step(i)
            step = iteration_to_imgs(i)
            if rank != 0:
                continue
            line = {}
            if i % ckpt.save_stats == 0:
                line.update(scalars.items())
            if i % ckpt.save_image == 0:
                log_synth_images(log, trainer, step)
            if i % ckpt.test == 0:
                line.update({"score/" + k: v for k, v in trainer.validation().items()})
            if line:
                log.add_scalars(i, step, line)
            if i % ckpt.save_model == 0:
                trainer.save_models("{:010d}".format(int(step)), int(step), directory=models_dir)
        if rank == 0:
            step = iteration_to_imgs(total_iteration)
            final = trainer.save_models("{:010d}".format(int(step)), int(step), directory=models_dir)
            print("saved", final)
    finally:
        if log is not None:
            log.close()
        if world > 1 and dist.is_initialized():
            dist.destroy_process_group()
    return {"out_dir": out_dir, "start_iteration": start, "total_iteration": total_iteration, "checkpoint": final}


if __name__ == "__main__":
    main()
    sys.exit(0)
