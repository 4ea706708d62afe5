"""Generate tests/golden/inversion.npz from the REFERENCE's own modules (GAN inversion, evaluate_reconstruction.py).

Runs only where the reference's sources are at hand (DUSTY_REFERENCE, default /root/reference):
    python tests/golden/make_inversion_golden.py
It imports the reference generator (models.define_G), SphericalOptimizer and masked_loss from utils/__init__.py and
utils/metrics/depth.py.  utils/__init__.py imports cv2 / omegaconf and, through utils.lidar / utils.geometry, the
rendering stack - none of it is used by the two functions taken from it, so those modules are empty placeholders here
(the way make_golden.py stands in for torchvision).  The inversion loop itself (evaluate_reconstruction.py:84-118) is a
script body, not a function: it is restated below line for line, with the injected latent and perturbations in place of
torch.randn, and the LR / noise schedules of :72-77 and :100-104.

Contents, for arch none / dusty1 / dusty2 x distance l1 / l2 at the step-fixture size (32x64, in_ch 8, ch_base 4,
ch_max 16, B = 3), num_step = 6 (step 0 runs with lr = 0):
    <arch>_<dist>/init/G/*   the generator's state_dict          <arch>_<dist>/gumbel  fixed pixel noise [1,1,H,W]
    <arch>_<dist>/inv_ref, mask                                 <arch>_<dist>/latent0 [B,nz]
    <arch>_<dist>/noise [S,B,nz]  the perturbation of step k (strength included)
    <arch>_<dist>/s<k>/loss [B], grad [B,nz] (d loss / d latent), latent [B,nz] (after the step)
    sched/k, sched/lr, sched/noise   the schedules at num_step = 1000
    depth/*   compute_depth_error / compute_depth_accuracy on crafted depth maps (incl. an all-masked-out sample)
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("DUSTY_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

import models  # noqa: E402  (reference package)


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _load_ref_utils():
    """utils/__init__.py with its unused heavy imports as placeholders"""
    for name in ("cv2", "omegaconf"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["omegaconf"].OmegaConf = None
    pkg = types.ModuleType("utils")
    pkg.__path__ = [os.path.join(REF, "utils")]
    sys.modules["utils"] = pkg
    geo = types.ModuleType("utils.geometry")
    geo.estimate_surface_normal = None
    lid = types.ModuleType("utils.lidar")
    lid.LiDAR = None
    sys.modules["utils.geometry"], sys.modules["utils.lidar"] = geo, lid
    return _load(os.path.join(REF, "utils", "__init__.py"), "ref_utils_init")


ref_utils = _load_ref_utils()
depth_metrics = _load(os.path.join(REF, "utils", "metrics", "depth.py"), "ref_depth_metrics")


class Cfg(dict):
    __getattr__ = dict.__getitem__


def make_cfg(arch, in_ch, ch_base, ch_max, shape):
    heads = {"none": {"depth": 1}, "dusty1": {"depth": 1, "confidence": 1}, "dusty2": {"depth": 1, "confidence": 2}}
    gen = Cfg(arch=f"{arch}/dcgan_eqlr", in_ch=in_ch, out_ch=heads[arch], ch_base=ch_base, ch_max=ch_max,
              drop_const=-1, shape=shape, tau=1)
    dis = Cfg(arch="dcgan_eqlr", in_ch=1, ch_base=ch_base, ch_max=ch_max, shape=shape)
    return Cfg(model=Cfg(gen=gen, dis=dis, ring=True))


# evaluate_reconstruction.py:72-77 (stylegan2's schedule) and :100-104 (the perturbation's strength)
def lr_schedule(iteration, num_step, lr_rampup_ratio=0.05, lr_rampdown_ratio=0.25):
    t = iteration / num_step
    gamma = min(1.0, (1.0 - t) / lr_rampdown_ratio)
    gamma = 0.5 - 0.5 * np.cos(gamma * np.pi)
    gamma = gamma * min(1.0, t / lr_rampup_ratio)
    return gamma


def noise_strength(current_step, num_step, noise_ratio=0.75, noise_sigma=1.0):
    progress = current_step / num_step
    w = max(0.0, 1.0 - progress / noise_ratio)
    return 0.05 * noise_sigma * w ** 2


def make_case(data, arch, distance, seed, in_ch=8, ch_base=4, ch_max=16, shape=(32, 64), B=3, num_step=6):
    torch.manual_seed(seed)
    H, W = shape
    G = models.define_G(make_cfg(arch, in_ch, ch_base, ch_max, list(shape)))
    G.eval()   # utils.setup (utils/__init__.py:131-133)
    for p in G.parameters():
        p.requires_grad_(False)   # utils.set_requires_grad(G, False)
    gumbel = torch.zeros(1, 1, H, W)
    if arch != "none":
        u1, u2 = torch.rand(1, 1, H, W), torch.rand(1, 1, H, W)
        gumbel = -torch.log(torch.log(u1 + 1e-10) / torch.log(u2 + 1e-10) + 1e-10)
        (G.gumbel_pixel if arch == "dusty2" else G.gumbel).fixed_noise = gumbel   # fix_noise=True
    # targets: a reconstructable scan (G's own output at a hidden latent) with dropped points, preprocess_reals (:63-69)
    with torch.no_grad():
        z_star = torch.randn(B, in_ch)
        key = "depth_orig" if arch != "none" else "depth"
        inv_star = ref_utils.tanh_to_sigmoid(G(z_star)[key])
    mask = (torch.rand(B, 1, H, W) > 0.2).float()
    inv_ref = mask * (0.7 * inv_star + 0.3 * torch.rand(B, 1, H, W)) + (1 - mask) * 0.0
    latent = torch.randn(B, in_ch)
    latent.div_(latent.pow(2).mean(dim=1, keepdim=True).add(1e-9).sqrt())   # :87-88
    noise = torch.stack([noise_strength(k, num_step) * torch.randn(B, in_ch) for k in range(num_step)])
    pre = f"{arch}_{distance}"
    for k, v in G.state_dict().items():
        data[f"{pre}/init/G/{k}"] = v.numpy()
    data[f"{pre}/gumbel"], data[f"{pre}/inv_ref"], data[f"{pre}/mask"] = gumbel.numpy(), inv_ref.numpy(), mask.numpy()
    data[f"{pre}/latent0"], data[f"{pre}/noise"] = latent.clone().numpy(), noise.numpy()   # (the loop updates latent in place)
    # :89-118
    latent = torch.nn.Parameter(latent).requires_grad_()
    optim = ref_utils.SphericalOptimizer(params=[latent], lr=0.1)
    scheduler = torch.optim.lr_scheduler.LambdaLR(optim, lr_lambda=lambda it: lr_schedule(it, num_step))
    for current_step in range(num_step):
        out = G(latent + noise[current_step])
        inv_gen = ref_utils.tanh_to_sigmoid(out["depth_orig"] if "dusty" in arch else out["depth"])
        loss = ref_utils.masked_loss(inv_ref, inv_gen, mask, distance)
        optim.zero_grad()
        loss.backward(gradient=torch.ones_like(loss))
        data[f"{pre}/s{current_step}/loss"] = loss.detach().numpy()
        data[f"{pre}/s{current_step}/grad"] = latent.grad.detach().clone().numpy()
        optim.step()
        scheduler.step()
        data[f"{pre}/s{current_step}/latent"] = latent.detach().clone().numpy()
    for k, v in (("arch", arch), ("distance", distance), ("B", B), ("in_ch", in_ch), ("ch_base", ch_base),
                 ("ch_max", ch_max), ("shape", shape), ("num_step", num_step)):
        data[f"{pre}/meta/{k}"] = np.array(v)


def make_depth(data):
    """crafted depth maps (metres): sample 0 all valid, 1 a sparse mask, 2 no valid pixel (NaN, as the reference)"""
    g = torch.Generator().manual_seed(7)
    B, H, W = 3, 16, 64
    ref = 0.9 + 119.1 * torch.rand(B, 1, H, W, generator=g)
    gen = ref * torch.exp(0.4 * torch.randn(B, 1, H, W, generator=g))
    gen = gen.clamp(0.9, 120.0)
    mask = torch.ones(B, 1, H, W)
    mask[1] = (torch.rand(1, H, W, generator=g) > 0.7).float()
    mask[2] = 0.0
    data["depth/ref"], data["depth/gen"], data["depth/mask"] = ref.numpy(), gen.numpy(), mask.numpy()
    for name, d in (("error", depth_metrics.compute_depth_error(ref, gen, mask)),
                    ("accuracy", depth_metrics.compute_depth_accuracy(ref, gen, mask))):
        for k, v in d.items():
            data[f"depth/{name}/{k}"] = v.numpy()


def main():
    data = {"meta/torch": np.array(torch.__version__)}
    seed = 100
    for arch in ("none", "dusty1", "dusty2"):
        for distance in ("l1", "l2"):
            make_case(data, arch, distance, seed)
            seed += 1
    ks = np.array([0, 1, 10, 49, 50, 51, 100, 500, 740, 749, 750, 751, 760, 900, 999])
    data["sched/k"] = ks
    data["sched/lr"] = np.array([lr_schedule(int(k), 1000) for k in ks], dtype=np.float64)
    data["sched/noise"] = np.array([noise_strength(int(k), 1000) for k in ks], dtype=np.float64)
    make_depth(data)
    path = os.path.join(HERE, "inversion.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, len(data), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
