"""Generate tests/golden/mgan_inversion.npz from the REFERENCE's own modules: multi-code GAN inversion (mGANprior), the
"#latents > 1" mode of the reference's demo (demo.py:353-366, 456-530).

Runs only where the reference's sources are at hand (DUSTY_REFERENCE, default /root/reference):
    python tests/golden/make_mgan_inversion_golden.py
Like make_inversion_golden.py (whose loaders it uses) it imports the reference generator (models.define_G), SphericalOptimizer
and masked_loss.  The demo's loop is the body of a Streamlit callback, not a function: it is restated below around the
reference's own modules - N latents, the composition weights alpha [N,C,1,1] = 1/N, the forward hook on the module named
`layer_name` that replaces its output by (o * alpha).sum(dim=0, keepdim=True), SphericalOptimizer(lr 0.1) on the latents and
torch.optim.Adam(lr 1e-3) on alpha under the same LambdaLR schedule - with the injected latent and perturbations in place of
torch.randn.

Contents, at the step-fixture size (32x64, in_ch 8, ch_base 4, ch_max 16: a0..a3 have 16 / 16 / 8 / 4 channels), B = 1 (the
reference's form), N = 4, num_step = 6 (step 0 runs with lr = 0), for the cases
    none_l1 at layers 0, 2, 3;  dusty2_l1 at layers 1, 3;  dusty1_l2 at layer 2       (key <arch>_<dist>_L<layer>):
    <case>/init/G/*   the generator's state_dict       <case>/gumbel  fixed pixel noise [1,1,H,W]
    <case>/inv_ref, mask [1,1,H,W]                      <case>/latent0 [N,nz]
    <case>/noise [S,N,nz]  the perturbation of step k (strength included)
    <case>/s<k>/loss [1], grad [N,nz] (d loss / d latent), dalpha [N,C], latent [N,nz] and alpha [N,C] (after the step)
    <case>/meta/*  arch, distance, layer, layer_name, N, seed, sizes
Every case's seed is the first one (from its start value) for which, at every step k >= 1, min |g| / max |g| > 1e-4 over the
latent gradient and over the alpha gradient: an early Adam step is about lr sign(g), so a component within rounding of zero
would make the recorded trajectory a coin toss.
"""
import os

import numpy as np
import torch

import make_inversion_golden as M   # (sets up the reference's packages on import)

HERE = os.path.dirname(os.path.abspath(__file__))
models, ref_utils = M.models, M.ref_utils

CASES = (("none", "l1", 0), ("none", "l1", 2), ("none", "l1", 3), ("dusty2", "l1", 1), ("dusty2", "l1", 3), ("dusty1", "l2", 2))


def make_case(arch, distance, layer, seed, N=4, in_ch=8, ch_base=4, ch_max=16, shape=(32, 64), num_step=6):
    torch.manual_seed(seed)
    H, W = shape
    G = models.define_G(M.make_cfg(arch, in_ch, ch_base, ch_max, list(shape)))
    G.eval()
    for p in G.parameters():
        p.requires_grad_(False)
    gumbel = torch.zeros(1, 1, H, W)
    if arch != "none":
        u1, u2 = torch.rand(1, 1, H, W), torch.rand(1, 1, H, W)
        gumbel = -torch.log(torch.log(u1 + 1e-10) / torch.log(u2 + 1e-10) + 1e-10)
        (G.gumbel_pixel if arch == "dusty2" else G.gumbel).fixed_noise = gumbel   # fix_noise=True
    with torch.no_grad():   # the target: a reconstructable scan with dropped points (as make_inversion_golden.py)
        z_star = torch.randn(1, in_ch)
        key = "depth_orig" if arch != "none" else "depth"
        inv_star = ref_utils.tanh_to_sigmoid(G(z_star)[key])
    mask = (torch.rand(1, 1, H, W) > 0.2).float()
    inv_ref = mask * (0.7 * inv_star + 0.3 * torch.rand(1, 1, H, W)) + (1 - mask) * 0.0
    latent = torch.randn(N, in_ch)
    latent.div_(latent.pow(2).mean(dim=1, keepdim=True).add(1e-8).sqrt())   # demo.py:459-460
    noise = torch.stack([M.noise_strength(k, num_step) * torch.randn(N, in_ch) for k in range(num_step)])
    layer_name = f"backbone.{layer}" if arch != "none" else f"{layer}"
    data = {}
    for k, v in G.state_dict().items():
        data[f"init/G/{k}"] = v.numpy()
    data["gumbel"], data["inv_ref"], data["mask"] = gumbel.numpy(), inv_ref.numpy(), mask.numpy()
    data["latent0"], data["noise"] = latent.clone().numpy(), noise.numpy()
    # demo.py:461-488
    latent = torch.nn.Parameter(latent).requires_grad_()
    optim_z = ref_utils.SphericalOptimizer(params=[latent], lr=0.1)
    sched = lambda it: M.lr_schedule(it, num_step)
    scheduler_z = torch.optim.lr_scheduler.LambdaLR(optim_z, lr_lambda=sched)
    hooked, feature_ch = [], None
    with torch.no_grad():   # get_feature_shapes (demo.py:141-163) for the one layer
        for name, module in G.named_modules():
            if name == layer_name:
                h = module.register_forward_hook(lambda m, i, o: hooked.append(o.shape))
                G(torch.randn(1, in_ch))
                h.remove()
    feature_ch = hooked[0][1]
    alpha = torch.full((N, feature_ch, 1, 1), fill_value=1 / N)
    alpha = torch.nn.Parameter(alpha).requires_grad_()

    def feature_composition(m, i, o):
        o = (o * alpha).sum(dim=0, keepdim=True)
        return o

    n_hooks = 0
    for name, module in G.named_modules():
        if name == layer_name:
            module.register_forward_hook(feature_composition)
            n_hooks += 1
    assert n_hooks == 1, layer_name
    optim_a = torch.optim.Adam([alpha], lr=0.001)
    scheduler_a = torch.optim.lr_scheduler.LambdaLR(optim_a, lr_lambda=sched)
    ok = True
    # demo.py:491-530 (l1 / l2 terms; B = 1, so masked_loss(...).mean() is the scan's loss)
    for cur_step in range(num_step):
        out = G(latent + noise[cur_step])
        inv_gen = ref_utils.tanh_to_sigmoid(out["depth_orig"] if "dusty" in arch else out["depth"])
        loss = ref_utils.masked_loss(inv_ref, inv_gen, mask, distance)
        assert loss.shape == (1,)
        optim_z.zero_grad()
        optim_a.zero_grad()
        loss.backward(gradient=torch.ones_like(loss))
        gz, ga = latent.grad.detach().clone(), alpha.grad.detach().clone().view(N, feature_ch)
        if cur_step >= 1:
            ok = ok and float(gz.abs().min() / gz.abs().max()) > 1e-4 and float(ga.abs().min() / ga.abs().max()) > 1e-4
        data[f"s{cur_step}/loss"], data[f"s{cur_step}/grad"], data[f"s{cur_step}/dalpha"] = loss.detach().numpy(), gz.numpy(), ga.numpy()
        optim_z.step()
        scheduler_z.step()
        optim_a.step()
        scheduler_a.step()
        data[f"s{cur_step}/latent"] = latent.detach().clone().numpy()
        data[f"s{cur_step}/alpha"] = alpha.detach().clone().view(N, feature_ch).numpy()
    for k, v in (("arch", arch), ("distance", distance), ("layer", layer), ("layer_name", layer_name), ("N", N), ("seed", seed),
                 ("in_ch", in_ch), ("ch_base", ch_base), ("ch_max", ch_max), ("shape", shape), ("num_step", num_step)):
        data[f"meta/{k}"] = np.array(v)
    return ok, data


def main():
    out = {"meta/torch": np.array(torch.__version__)}
    seed = 300
    for arch, distance, layer in CASES:
        while True:
            ok, data = make_case(arch, distance, layer, seed)
            seed += 1
            if ok:
                break
            print("seed", seed - 1, "has a gradient component within 1e-4 of zero: next")
        pre = f"{arch}_{distance}_L{layer}"
        for k, v in data.items():
            out[f"{pre}/{k}"] = v
        print(pre, "seed", int(data["meta/seed"]), "loss", [float(data[f"s{k}/loss"][0]) for k in range(6)])
    path = os.path.join(HERE, "mgan_inversion.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
