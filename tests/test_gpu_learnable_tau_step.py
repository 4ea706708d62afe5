"""`model.gen.tau: null` - the learnable Gumbel temperature - through the whole `Trainer.step`, against fixtures the
reference's own modules produced with tau=None (tests/golden/make_learnable_tau_golden.py): test_gpu_step's golden loop at the
project's 1e-3, plus the temperature weights' gradients, updates, optimizer state, checkpoints and the inference paths.

The temperature gradient is a sum that cancels 20- to 50-fold, so it is held to 1e-3 of the MAGNITUDE of what was summed,
A = sigmoid(w) sum |terms| (recorded by the generator: rel-L2's normalisation, the error over the size of the summands); the
fixtures' seeds keep |grad| >= 0.01 A, so a wrong constant factor of 2 misses that bound ten times over.  At beta1 = 0 the first
Adam steps are lr * sign(g): the after-step weights at rel-L2 1e-3 pin the gradient's sign."""
import math

import pytest
import torch

from tests.golden_util import load, rel_l2, step_rand, sub
from tests.test_gpu_step import grads_by_name

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = ["dusty1_ltau", "dusty2_ltau"]
TAU_KEYS = {"dusty1": ["gumbel.weight"], "dusty2": ["gumbel_pixel.weight", "gumbel_image.weight"]}
TOL = 1e-3


def make_trainer(arch, shape, in_ch, ch_base, ch_max, B, tau="null", pl=0.0, n_acc=1, amp=False, ring=True, gp=1.0):
    from dusty_gan_amd.trainers.dcgan_amp import Trainer
    from dusty_gan_amd.utils.config import load_config
    model = {"dusty1": "dusty1_dcgan_eqlr", "dusty2": "dusty2_dcgan_eqlr"}[arch]
    cfg = load_config([f"model={model}", "dataset=synthetic", f"dataset.shape=[{shape[0]},{shape[1]}]",
                       f"model.gen.in_ch={in_ch}", f"model.gen.ch_base={ch_base}", f"model.gen.ch_max={ch_max}",
                       f"model.dis.ch_base={ch_base}", f"model.dis.ch_max={ch_max}", f"model.ring={str(ring).lower()}",
                       f"solver.batch_size={B * n_acc}", f"solver.loss.gp={gp}", f"enable_amp={str(amp).lower()}",
                       f"solver.num_accumulation={n_acc}", "dataset.pool=1", f"solver.loss.pl={pl}", f"model.gen.tau={tau}"])
    return Trainer(cfg, {"gpu": 0, "ngpus": 1, "batch_size": B, "num_workers": 0})


def trainer_of(g, **kw):
    return make_trainer(str(g["meta/arch"]), tuple(int(v) for v in g["meta/shape"]), int(g["meta/in_ch"]), int(g["meta/ch_base"]),
                        int(g["meta/ch_max"]), int(g["meta/B"]), gp=float(g["meta/gp"]), **kw)


def _softplus(w):
    return w + math.log1p(math.exp(-w)) if w > 0 else math.log1p(math.exp(w))


@pytest.fixture(scope="module", params=CASES)
def trained(request, tmp_path_factory):
    """the fixture's steps on the GPU, every criterion of test_step_matches_reference_golden asserted on the way, and a saved
    checkpoint: (golden, trainer, checkpoint path, config path)"""
    g = load("step_" + request.param)
    arch, steps = str(g["meta/arch"]), int(g["meta/steps"])
    tr = trainer_of(g)
    names = [k for k, _ in tr.G.named_parameters()]
    # the reference's parameter names and order (its state_dict adds the wrapper's buffer in front)
    assert names[-len(TAU_KEYS[arch]):] == TAU_KEYS[arch] and names == [k for k in sub(g, "init/G") if k != "drop_const"]
    tr.G.load_state_dict(sub(g, "init/G"))
    tr.D.load_state_dict(sub(g, "init/D"))
    tr.G_ema.load_state_dict(sub(g, "init/G"))
    assert abs(tr.ema_decay - float(g["meta/ema_decay"])) < 1e-12
    for it in range(steps):
        pre = f"s{it}"
        pol, mask = torch.from_numpy(g[f"{pre}/pol"]), torch.from_numpy(g[f"{pre}/mask"])
        x_real, m_real = tr.fetch_reals({"depth": pol, "mask": mask})
        assert rel_l2(x_real.cpu(), g[f"{pre}/x_real"]) < 1e-5
        rand = step_rand(g, it)
        tr.optimize_D(reals=[(x_real, m_real)], rands=[rand])
        synth = {k: v.detach().cpu().clone() for k, v in tr._mb[0]["synth"].items()}
        gD = grads_by_name(tr.optim_D)
        sc = tr.optimize_G().cpu().tolist()
        gG = grads_by_name(tr.optim_G)
        got = {"loss/D/output/real": sc[0], "loss/D/output/fake": sc[1], "loss/D/adversarial": sc[2],
               "loss/D/gradient_penalty": sc[3], "loss/G/adversarial": sc[4]}
        for k, v in sub(g, f"{pre}/scalar").items():
            assert abs(got[k] - float(v)) <= TOL * max(1.0, abs(float(v))), (k, got[k], float(v))
        for k, v in sub(g, f"{pre}/synth").items():
            if k == "mask":
                assert (synth[k] != v).float().mean() < 1e-3
            else:
                assert rel_l2(synth[k], v) < TOL, k
        for k, v in sub(g, f"{pre}/grad_D").items():
            assert rel_l2(gD[k], v) < TOL, ("grad_D", k)
        mags = sub(g, f"{pre}/grad_G_mag")
        assert sorted(mags) == sorted(TAU_KEYS[arch])
        for k, v in sub(g, f"{pre}/grad_G").items():
            if k in mags:
                A, got_g, ref_g = float(mags[k]), float(gG[k]), float(v)
                print(f"TAU GRAD {request.param} step {it} {k}: got {got_g:.9g} ref {ref_g:.9g} A {A:.6g} "
                      f"|got - ref| / A = {abs(got_g - ref_g) / A:.3g} |ref| / A = {abs(ref_g) / A:.3g}")
                assert abs(ref_g) >= 0.01 * A, (k, ref_g, A)              # (the fixture's own condition)
                assert abs(got_g - ref_g) <= TOL * A, ("grad_G", k, got_g, ref_g, A)
            else:
                assert rel_l2(gG[k], v) < TOL, ("grad_G", k)
        for tag, net in (("G", tr.G), ("D", tr.D), ("G_ema", tr.G_ema)):
            sd = net.state_dict()
            for k, v in sub(g, f"{pre}/after/{tag}").items():
                assert rel_l2(sd[k].cpu(), v) < TOL, (tag, k, sd[k].cpu(), v)
    d = tmp_path_factory.mktemp("ltau_" + request.param)
    path = tr.save_models("0000000004", 4, directory=str(d))
    from dusty_gan_amd.utils.config import dump_config
    cfg_path = str(d / "config.yaml")
    dump_config(tr.cfg, cfg_path)
    return g, tr, path, cfg_path


def test_step_matches_reference_golden_with_learnable_tau(trained):
    """the loop above passed; the optimizer's state in torch.optim.Adam's format follows named_parameters(), the new
    parameters' included"""
    g, tr, _, _ = trained
    arch, steps = str(g["meta/arch"]), int(g["meta/steps"])
    for tag, opt, net in (("G", tr.optim_G, tr.G), ("D", tr.optim_D, tr.D)):
        sdo = opt.state_dict()
        names = [k for k, _ in net.named_parameters()]
        assert sdo["param_groups"][0]["params"] == list(range(len(names)))
        assert sorted(sdo["state"]) == list(range(len(names)))
        for i, (k, p) in enumerate(net.named_parameters()):
            st = sdo["state"][i]
            assert tuple(st["exp_avg_sq"].shape) == tuple(p.shape) == tuple(st["exp_avg"].shape), (tag, k)
            assert int(st["step"]) == steps
            assert rel_l2(st["exp_avg_sq"], g[f"final/optim_{tag}/{k}/exp_avg_sq"]) < TOL, (tag, k)
    n = len(TAU_KEYS[arch])
    names = [k for k, _ in tr.G.named_parameters()]
    assert names[-n:] == TAU_KEYS[arch]
    assert (tr.G.store.view("tau_w") != 0).all() and (tr.G_ema.store.view("tau_w") != 0).all()   # trained, and averaged


def test_checkpoint_roundtrip_keys_and_other_kind(trained):
    g, tr, path, _ = trained
    arch = str(g["meta/arch"])
    sd = torch.load(path, map_location="cpu")
    for net in ("G", "G_ema"):
        assert list(sd[net].keys())[-len(TAU_KEYS[arch]):] == TAU_KEYS[arch]
        assert list(sd[net].keys()) == list(sub(g, "init/G").keys())
        for k in TAU_KEYS[arch]:
            assert sd[net][k].shape == ()
    tr2 = trainer_of(g)
    tr2.G.load_state_dict(sd["G"]); tr2.D.load_state_dict(sd["D"]); tr2.G_ema.load_state_dict(sd["G_ema"])
    tr2.optim_G.load_state_dict(sd["optim_G"]); tr2.optim_D.load_state_dict(sd["optim_D"])
    assert torch.equal(tr2.G.store.flat.cpu(), tr.G.store.flat.cpu())
    assert torch.equal(tr2.G_ema.store.flat.cpu(), tr.G_ema.store.flat.cpu())
    assert torch.equal(tr2.G.store.v.cpu(), tr.G.store.v.cpu())
    assert torch.equal(tr2.D.store.v.cpu(), tr.D.store.v.cpu())
    # a model of the other kind: torch's usual errors, both ways
    fixed = trainer_of(g, tau=1)
    assert fixed.G.store.n < tr.G.store.n and "tau_w" not in fixed.G.store.seg
    with pytest.raises(RuntimeError, match="Unexpected key"):
        fixed.G.load_state_dict(sd["G"])
    with pytest.raises(RuntimeError, match="Missing key"):
        tr2.G.load_state_dict(fixed.G.state_dict())


def test_path_length_with_learnable_tau_is_refused():
    with pytest.raises(NotImplementedError, match="pl"):
        make_trainer("dusty2", (32, 64), 8, 4, 16, 4, pl=2.0)


def test_setup_inversion_and_raydrop_on_the_trained_generator(trained):
    """utils.setup rebuilds the eval G_ema with the by-value tau of the inference paths synchronised from the loaded weight; GAN
    inversion and the ray-drop sampling run on it, and - hard masks do not depend on a positive slope - a fixed-tau copy of the
    same network forms the same masks"""
    from dusty_gan_amd import inversion, raydrop
    from dusty_gan_amd.models import define_G
    from dusty_gan_amd.utils import setup
    g, tr, path, cfg_path = trained
    arch = str(g["meta/arch"])
    cfg, G, lidar, device = setup(path, cfg_path, ema=True, fix_noise=False)
    assert not G.training and torch.equal(G.store.flat.cpu(), tr.G_ema.store.flat.cpu())
    w_pixel = float(tr.G_ema.store.view("tau_w")[0])
    want = 1.0 / (_softplus(w_pixel) + 1.0)
    assert w_pixel != 0.0 and abs(G.backbone.tau - want) <= 2.0 ** -22 * want, (G.backbone.tau, want)
    H, W = (int(v) for v in g["meta/shape"])
    B, nz = 2, int(g["meta/in_ch"])
    gen = torch.Generator().manual_seed(3)
    z = torch.randn(B, nz, generator=gen).to(device)
    u1, u2 = torch.rand(B, 1, H, W, generator=gen), torch.rand(B, 1, H, W, generator=gen)
    noise = (-torch.log(torch.log(u1 + 1e-10) / torch.log(u2 + 1e-10) + 1e-10)).to(device)
    out = {k: v.clone() for k, v in G(z, noise={"pixel": noise}).items()}
    # the fixed-tau copy: the same parameters without the temperature weights
    cfg.model.gen.tau = 1
    Gf = define_G(cfg)
    Gf.eval()
    Gf.load_state_dict({k: v for k, v in G.state_dict().items() if k not in TAU_KEYS[arch]})
    Gf.to(device)
    outf = Gf(z, noise={"pixel": noise})
    for k in ("mask", "depth", "depth_orig", "confidence"):
        assert torch.equal(out[k], outf[k]), k
    assert 0.0 < float(out["mask"][:, 0].mean()) < 1.0
    # two inversion steps towards the first recorded batch, then the keep masks from its logits
    inv_ref = ((torch.from_numpy(g["s0/x_real"]) + 1.0) / 2.0).to(device)
    mask_ref = torch.from_numpy(g["s0/mask"]).float().to(device)
    res = inversion.invert(G, inv_ref, mask_ref, num_step=2, seed=5, gumbel_noise=noise[:1])
    assert torch.isfinite(res["loss"]).all() and torch.isfinite(res["latent"]).all()
    assert abs(G.backbone.tau - want) <= 2.0 ** -22 * want
    conf = res["out"]["confidence"].clone()
    win = torch.zeros(B, H * W, dtype=torch.int32, device=device)
    keep = raydrop.sample_keep(conf, win, G.backbone.masker, G.backbone.tau, realisations=2, seed=9)
    keepf = raydrop.sample_keep(conf, win, Gf.backbone.masker, 1.0, realisations=2, seed=9)
    assert keep.shape == (B, 2, H, W) and torch.equal(keep, keepf)
