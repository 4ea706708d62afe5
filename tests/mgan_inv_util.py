"""Multi-code GAN inversion (mGANprior, demo.py:456-530), test side: the fixture's cases and the restatement of the loop on the
oracle's layer functions (oracle.dusty_oracle.proj / up / head / maskout, used as they are) with the composition between them."""
from collections import OrderedDict

import torch

from oracle import dusty_oracle as O
from tests.test_inversion_cpu import _emu_bf16, _null, lr_lambda

# (arch, distance, composition layer) of tests/golden/mgan_inversion.npz
CASES = (("none", "l1", 0), ("none", "l1", 2), ("none", "l1", 3), ("dusty2", "l1", 1), ("dusty2", "l1", 3), ("dusty1", "l2", 2))
IDS = [f"{a}_{d}_L{l}" for a, d, l in CASES]


def fixture_case(g, arch, distance, layer):
    pre = f"{arch}_{distance}_L{layer}/"
    params = {k[len(pre) + 7:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre + "init/G/")}
    t = lambda k: torch.from_numpy(g[pre + k])
    return dict(pre=pre, params=params, gumbel=t("gumbel"), inv_ref=t("inv_ref"), mask=t("mask"), latent0=t("latent0"),
                noise=t("noise"), S=int(g[pre + "meta/num_step"]), N=int(g[pre + "meta/N"]), name=str(g[pre + "meta/layer_name"]))


def multi_code_generator(params, z, alpha, layer, arch, noise):
    """G on z [B,N,nz] with the feature maps of the N codes blended at a[layer] by alpha [B,N,C] (the demo's forward hook
    o -> (o * alpha).sum(dim=0, keepdim=True), per scan), eval mode.  Under O.EMU.bf16 the composite is rounded where the
    engine stores it (_rf) and so is the gradient that reaches it (_rg: the unmasked backward-data launch stores bf16)."""
    B, N, nz = z.shape
    p = O._g_prefix(params)
    h = O.proj(z.reshape(B * N, nz), params[p + "0.0.module.weight"], params[p + "0.1.bias"])
    for i in (1, 2, 3):
        if i <= layer:
            h = O.up(h, params[p + f"{i}.1.module.weight"], params[p + f"{i}.2.bias"])
    C = h.shape[1]
    h = O._rf(O._rg((h.view(B, N, *h.shape[1:]) * alpha.view(B, N, C, 1, 1)).sum(dim=1)))
    for i in (1, 2, 3):
        if i > layer:
            h = O.up(h, params[p + f"{i}.1.module.weight"], params[p + f"{i}.2.bias"])
    out = OrderedDict()
    for name in ("depth", "confidence"):
        wk = p + f"4.heads.{name}.1.module.weight"
        if wk in params:
            out[name] = O.head(h, params[wk], params[p + f"4.heads.{name}.1.module.bias"])
    out["depth"] = torch.tanh(out["depth"])
    dc = float(params["drop_const"]) if "drop_const" in params else -1.0
    return O.maskout(out, arch, noise, 1.0, dc, training=False)


def oracle_invert_multi(params, arch, gumbel, inv_ref, mask, latent0, noise, num_step, distance, layer, alpha0=None,
                        alpha_lr=1e-3, dtype=None):
    """the demo's multi-code loop restated on the oracle; latent0 [B,N,nz], noise [S,B,N,nz].  Returns per step
    (loss [B], d loss / d latent [B,N,nz], d loss / d alpha [B,N,C], latent and alpha after the step)."""
    B, _, H, W = inv_ref.shape
    N = latent0.shape[1]
    nzd = {"pixel": gumbel.expand(B, 1, H, W)} if arch != "none" else None
    p = O._g_prefix(params)
    C = params[p + "0.1.bias"].numel() if layer == 0 else params[p + f"{layer}.2.bias"].numel()
    latent = torch.nn.Parameter(latent0.clone())
    alpha = torch.nn.Parameter(torch.full((B, N, C), 1.0 / N) if alpha0 is None else alpha0.clone())
    opt_z = torch.optim.Adam([latent], lr=0.1)
    opt_a = torch.optim.Adam([alpha], lr=alpha_lr)
    sched = lambda it: lr_lambda(it, num_step)
    sch_z = torch.optim.lr_scheduler.LambdaLR(opt_z, lr_lambda=sched)
    sch_a = torch.optim.lr_scheduler.LambdaLR(opt_a, lr_lambda=sched)
    res = []
    for k in range(num_step):
        with (_emu_bf16() if dtype is not None else _null()):
            out = multi_code_generator(params, latent + noise[k], alpha, layer, arch, nzd)
        d = out["depth_orig"] if arch != "none" else out["depth"]
        diff = inv_ref - (d + 1.0) / 2.0
        per = diff.abs() if distance == "l1" else diff ** 2
        loss = (per * mask).sum(dim=(1, 2, 3)) / mask.sum(dim=(1, 2, 3))
        opt_z.zero_grad()
        opt_a.zero_grad()
        loss.backward(gradient=torch.ones_like(loss))
        gz, ga = latent.grad.detach().clone(), alpha.grad.detach().clone()
        opt_z.step()
        with torch.no_grad():   # SphericalOptimizer: every code's row back to unit RMS
            latent.div_(latent.pow(2).mean(dim=2, keepdim=True).add(1e-9).sqrt())
        sch_z.step()
        opt_a.step()
        sch_a.step()
        res.append((loss.detach().clone(), gz, ga, latent.detach().clone(), alpha.detach().clone()))
    return res
