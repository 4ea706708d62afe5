"""Generate tests/golden/chamfer_inversion.npz from the REFERENCE's own modules: GAN inversion with the Chamfer loss of
the reference's demo (demo.py:491-530).

Runs only where the reference's sources are at hand (DUSTY_REFERENCE, default /root/reference), on the CPU:
    python tests/golden/make_chamfer_inversion_golden.py
It imports the reference's define_G (the DUSty1 / DUSty2 wrappers in eval mode with a fixed Gumbel noise), utils.postprocess,
Coordinate.inv_to_xyz (utils/lidar.py, on a synthetic angle grid), SphericalOptimizer and masked_loss.  utils/__init__.py's
unused heavy imports are placeholders (make_inversion_golden.py's loader, config and schedules are imported); utils.geometry's surface normals, which postprocess
computes and the loss never reads, return zeros.  The reference's Chamfer extension cannot be built for a CPU run without its
CUDA file, so nnsearch and the backward (chamfer_distance.cpp:39-62,82-140) are restated as a torch.autograd.Function
(tests/chamfer_inv_util.ChamferFn): squared differences summed in coordinate order, the first minimum wins.  The loop body
(demo.py:491-530) is a script, restated below with the injected latent and perturbations; every loss term is kept per
sample (the loss is a [B] vector backpropagated with ones, demo.py:525).

Every case runs twice, in float32 and in float64, from the same weights and inputs.  Contents, per case of
chamfer_inv_util.CASES at the step-fixture size (32x64, in_ch 8, ch_base 4, ch_max 16, B = 3, 6 steps; 2048 points):
    <case>/init/G/*, gumbel, inv_ref, mask_bits (np.packbits), latent0, noise [S,B,nz], meta/*
                                            (under the case meta/inputs names: dusty2's two cases share one set)
    <case>/s<k>/loss, grad, latent          float64 run       <case>/s<k>/e_loss, e_grad, e_latent   |float32 - float64|
    <case>/head/raw [B,heads,H,W] float32   the head's output at step 0 (float64 run, rounded)  - chamfer-only cases
    <case>/head/grad, head/e_grad           d loss / d (head output) of the float64 run (stored rounded to float32: 2^-24
                                            relative, far below the tests' 1e-6 floor) and |float32 - float64| (rounded DOWN
                                            to 8 significant bits for the file's size: a bound from it is never wider)
    pairs/<name>/idx (int16)                the float64 first-minimum matches A -> B of the stand-alone pairs, whose points
                                            chamfer_inv_util.pair(name, meta/pair_seed) rebuilds
Conditions asserted here (seeds are advanced until they hold; the checked seeds are stored in meta/*): in every search of
every float64 run and of every stand-alone pair except the dyadic one, the nearest NON-coincident runner-up is farther than
min (1 + 2^-18); on the dyadic pair ties exist and the first index is recorded."""
import copy
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("DUSTY_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(1, os.path.dirname(os.path.dirname(HERE)))

import models  # noqa: E402  (reference package)

from tests import chamfer_inv_util as U  # noqa: E402

MARGIN = 1.0 + 2.0 ** -18


# the reference's utils/__init__.py (postprocess, SphericalOptimizer, masked_loss) behind its placeholders, the fixture
# generator's config and the two schedules: the ones tests/golden/make_inversion_golden.py already has
sys.path.insert(2, HERE)
import make_inversion_golden as M  # noqa: E402

ref_utils, Cfg, make_cfg, lr_schedule, noise_strength = M.ref_utils, M.Cfg, M.make_cfg, M.lr_schedule, M.noise_strength
ref_utils.estimate_surface_normal = lambda xyz, mode="closest": torch.zeros_like(xyz)   # (the loss never reads the normals)
sys.modules["utils.render"] = types.ModuleType("utils.render")   # (points_to_depth only)
sys.modules["utils"].render = sys.modules["utils.render"]
ref_lidar = M._load(os.path.join(REF, "utils", "lidar.py"), "utils.lidar")   # the real Coordinate


class Grid(ref_lidar.Coordinate):
    """the reference's Coordinate on a given angle table"""

    def __init__(self, angle, shape):
        self._angle = angle
        super().__init__(min_depth=U.MIN_DEPTH, max_depth=U.MAX_DEPTH, shape=shape)

    def init_coordmap(self, H, W):
        return self._angle


def run_loop(G, arch, gumbel, angle, inv_ref, mask, latent0, noise, distance, dtype):
    """demo.py:491-530 in `dtype`; returns per step (loss, grad, latent) and step 0's head output and gradient"""
    G = copy.deepcopy(G).to(dtype)
    H, W = inv_ref.shape[2:]
    if arch != "none":
        (G.gumbel_pixel if arch == "dusty2" else G.gumbel).fixed_noise = gumbel.to(dtype)
    coord = Grid(angle.to(dtype), (H, W))
    inv_ref, mask, noise = inv_ref.to(dtype), mask.to(dtype), noise.to(dtype)
    points_ref = coord.inv_to_xyz(inv_ref, U.TOL)
    latent = torch.nn.Parameter(latent0.to(dtype).clone()).requires_grad_()
    optim = ref_utils.SphericalOptimizer(params=[latent], lr=0.1)
    num_step = noise.shape[0]
    sched = torch.optim.lr_scheduler.LambdaLR(optim, lr_lambda=lambda it: lr_schedule(it, num_step))
    head_mod = (G.backbone if arch != "none" else G)[4]
    seen = {}
    hook = head_mod.register_forward_hook(lambda m, i, o: seen.update(o))
    steps, head = [], None
    for k in range(num_step):
        out = G(latent + noise[k])
        raw = dict(seen)
        for v in raw.values():
            v.retain_grad()
        out = ref_utils.postprocess(out, coord, U.TOL)
        inv_gen = out["depth_orig"] if "dusty" in arch else out["depth"]
        loss = 0
        if "chamfer" in distance:
            dl, dr = U.ChamferFn.apply(U.flatten(points_ref), U.flatten(out["points"]))
            loss = loss + dl.mean(dim=1) + dr.mean(dim=1)
        if "l1" in distance:
            loss = loss + ref_utils.masked_loss(inv_ref, inv_gen, mask, "l1")
        if "l2" in distance:
            loss = loss + ref_utils.masked_loss(inv_ref, inv_gen, mask, "l2")
        optim.zero_grad()
        loss.backward(gradient=torch.ones_like(loss))
        if k == 0:
            keys = ["depth"] + (["confidence"] if arch != "none" else [])
            head = (torch.cat([raw[n].detach() for n in keys], dim=1), torch.cat([raw[n].grad for n in keys], dim=1))
        grad = latent.grad.detach().clone()
        optim.step()
        sched.step()
        steps.append((loss.detach().clone(), grad, latent.detach().clone()))
    hook.remove()
    return steps, head


def margins_ok(records):
    for x1, x2 in records:
        for a, b in zip(x1, x2):
            if float(U.runner_up_ratio(a, b).min()) <= MARGIN or float(U.runner_up_ratio(b, a).min()) <= MARGIN:
                return False
    return True


def make_case(data, name, arch, distance, seed, in_ch=8, ch_base=4, ch_max=16, shape=(32, 64), B=3, num_step=6, shares=None):
    torch.manual_seed(seed)
    H, W = shape
    G = models.define_G(make_cfg(arch, in_ch, ch_base, ch_max, list(shape)))
    G.eval()
    for p in G.parameters():
        p.requires_grad_(False)
    gumbel = torch.zeros(1, 1, H, W)
    if arch != "none":
        u1, u2 = torch.rand(1, 1, H, W), torch.rand(1, 1, H, W)
        gumbel = -torch.log(torch.log(u1 + 1e-10) / torch.log(u2 + 1e-10) + 1e-10)
        (G.gumbel_pixel if arch == "dusty2" else G.gumbel).fixed_noise = gumbel
    with torch.no_grad():
        z_star = torch.randn(B, in_ch)
        key = "depth_orig" if arch != "none" else "depth"
        inv_star = ref_utils.tanh_to_sigmoid(G(z_star)[key])
    mask = (torch.rand(B, 1, H, W) > 0.2).float()
    inv_ref = mask * (0.7 * inv_star + 0.3 * torch.rand(B, 1, H, W)) + (1 - mask) * 0.0
    latent0 = torch.randn(B, in_ch)
    latent0.div_(latent0.pow(2).mean(dim=1, keepdim=True).add(1e-9).sqrt())
    noise = torch.stack([noise_strength(k, num_step) * torch.randn(B, in_ch) for k in range(num_step)])
    angle = U.angle_grid(H, W)
    args = (G, arch, gumbel, angle, inv_ref, mask, latent0, noise, distance)
    U.ChamferFn.record = []
    s64, h64 = run_loop(*args, torch.float64)
    records, U.ChamferFn.record = U.ChamferFn.record, None
    if not margins_ok(records):
        return False
    s32, h32 = run_loop(*args, torch.float32)
    if shares is None:   # (a case made from another's seed has the same generator and inputs: stored once)
        for k, v in G.state_dict().items():
            data[f"{name}/init/G/{k}"] = v.numpy()
        data[f"{name}/gumbel"], data[f"{name}/inv_ref"] = gumbel.numpy(), inv_ref.numpy()
        data[f"{name}/mask_bits"] = np.packbits(mask.numpy().astype(np.uint8).ravel())
        data[f"{name}/latent0"], data[f"{name}/noise"] = latent0.numpy(), noise.numpy()
    for k, ((l64, g64, z64), (l32, g32, z32)) in enumerate(zip(s64, s32)):
        for key, v64, v32 in (("loss", l64, l32), ("grad", g64, g32), ("latent", z64, z32)):
            data[f"{name}/s{k}/{key}"] = v64.numpy()
            data[f"{name}/s{k}/e_{key}"] = (v32.double() - v64).abs().float().numpy()
    if distance == ("chamfer",):
        data[f"{name}/head/raw"] = h64[0].float().numpy()
        data[f"{name}/head/grad"] = h64[1].float().numpy()
        e = (h32[1].double() - h64[1]).abs().float().numpy()
        data[f"{name}/head/e_grad"] = (e.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)   # rounded DOWN to 8 bits
    for k, v in (("arch", arch), ("distance", "+".join(distance)), ("B", B), ("in_ch", in_ch), ("ch_base", ch_base),
                 ("ch_max", ch_max), ("shape", shape), ("num_step", num_step), ("seed", seed),
                 ("inputs", shares or name)):
        data[f"{name}/meta/{k}"] = np.array(v)
    return True


def make_pairs(data):
    seed = 500
    while True:
        ok = True
        for name in U.PAIR_NAMES:
            if name == U.DYADIC[0]:
                continue
            a, b = U.pair(name, seed)
            ok = ok and float(U.runner_up_ratio(a, b).min()) > MARGIN
        if ok:
            break
        seed += 2
    for name in U.PAIR_NAMES:
        a, b = U.pair(name, seed)
        _, idx = U.nn_first(a.double(), b.double())
        data[f"pairs/{name}/idx"] = idx.numpy().astype(np.int16)
    a, b = U.pair(U.DYADIC[0], seed)
    d, idx = U.nn_first(a.double(), b.double())
    ties = int(((U.sqdist(a.double(), b.double()) == d[:, None]).sum(dim=1) > 1).sum())
    assert ties > a.shape[0] // 2, ties   # the dyadic pair is about ties
    data["meta/pair_seed"] = np.array(seed)
    print("pairs: seed", seed, "dyadic points with a tied minimum:", ties, "of", a.shape[0])


def main():
    data = {"meta/torch": np.array(torch.__version__)}
    seed = 300
    for name, arch, distance in U.CASES[:2]:
        while not make_case(data, name, arch, distance, seed):
            print(name, "seed", seed, "rejected (a runner-up within the margin)")
            seed += 1
        print(name, "seed", seed)
        seed += 1
    # dusty2: chamfer alone and l1 + chamfer from ONE seed - the same generator, target and perturbations, stored once
    (n3, a3, d3), (n4, a4, d4) = U.CASES[2:]
    while not (make_case(data, n3, a3, d3, seed) and make_case(data, n4, a4, d4, seed, shares=n3)):
        print(n3, n4, "seed", seed, "rejected (a runner-up within the margin)")
        seed += 1
    print(n3, n4, "seed", seed)
    make_pairs(data)
    path = os.path.join(HERE, "chamfer_inversion.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, len(data), "arrays", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main()
