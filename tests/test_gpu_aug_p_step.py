"""`solver.augment_p` < 1 through the whole `Trainer.step`: against fixtures the reference's own modules produced with
DiffAugment(p = 0.5) (tests/golden/make_aug_gate_golden.py: step_none_augp.npz, step_dusty2_augp.npz - 32x64, B = 4, two steps,
fp32; every A(.) call holds at least two gate states, the G phase's fake sets all four), every criterion of
tests/test_gpu_step.py's golden loop at its 1e-3; under the captured step graph; and p = 1 against a trainer built without the key."""
import pytest
import torch

from tests import aug_gate_ref as R
from tests.golden_util import load, rel_l2, step_rand, sub
from tests.test_gpu_step import grads_by_name

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3


def make_trainer(arch, shape, in_ch, ch_base, ch_max, B, amp=False, extra=()):
    from dusty_gan_amd.trainers.dcgan_amp import Trainer
    from dusty_gan_amd.utils.config import load_config
    model = {"none": "dcgan_eqlr", "dusty1": "dusty1_dcgan_eqlr", "dusty2": "dusty2_dcgan_eqlr"}[arch]
    cfg = load_config([f"model={model}", "dataset=synthetic", f"dataset.shape=[{shape[0]},{shape[1]}]",
                       f"model.gen.in_ch={in_ch}", f"model.gen.ch_base={ch_base}", f"model.gen.ch_max={ch_max}",
                       f"model.dis.ch_base={ch_base}", f"model.dis.ch_max={ch_max}", "model.ring=true",
                       f"solver.batch_size={B}", f"enable_amp={str(amp).lower()}", "dataset.pool=1", *extra])
    return Trainer(cfg, {"gpu": 0, "ngpus": 1, "batch_size": B, "num_workers": 0})


@pytest.mark.parametrize("case", ["none_augp", "dusty2_augp"])
def test_step_matches_reference_golden_at_p_half(case):
    g = load("step_" + case)
    arch, B, steps = str(g["meta/arch"]), int(g["meta/B"]), int(g["meta/steps"])
    assert float(g["meta/augment_p"]) == 0.5 and B == 4 and steps == 2
    tr = make_trainer(arch, tuple(int(v) for v in g["meta/shape"]), int(g["meta/in_ch"]), int(g["meta/ch_base"]),
                      int(g["meta/ch_max"]), B, extra=["solver.augment_p=0.5"])
    assert tr.A.p == 0.5 and tr.ada is None
    tr.G.load_state_dict(sub(g, "init/G"))
    tr.D.load_state_dict(sub(g, "init/D"))
    tr.G_ema.load_state_dict(sub(g, "init/G"))
    assert abs(tr.ema_decay - float(g["meta/ema_decay"])) < 1e-12
    fake_states = []
    for it in range(steps):
        pre = f"s{it}"
        pol, mask = torch.from_numpy(g[f"{pre}/pol"]), torch.from_numpy(g[f"{pre}/mask"])
        x_real, m_real = tr.fetch_reals({"depth": pol, "mask": mask})
        assert rel_l2(x_real.cpu(), g[f"{pre}/x_real"]) < 1e-5
        rand = step_rand(g, it)
        for j, rp in enumerate(rand["aug"]):                 # the fixture's own condition: mixed gates in every call
            st = R.gate_state(rp)
            assert len(set(st.tolist())) >= 2, (it, j, st)
            if j == 3:
                fake_states += st.tolist()
        # A(real) alone, against the reference's recorded augmented batch
        xa = tr.A.apply(x_real.clone(), tr.A.params_to_device(rand["aug"][0], DEV))
        assert rel_l2(xa.cpu(), g[f"{pre}/x_real_aug"]) < 1e-5
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
        for k, v in sub(g, f"{pre}/grad_G").items():
            assert rel_l2(gG[k], v) < TOL, ("grad_G", k)
        for tag, net in (("G", tr.G), ("D", tr.D), ("G_ema", tr.G_ema)):
            sd = net.state_dict()
            for k, v in sub(g, f"{pre}/after/{tag}").items():
                assert rel_l2(sd[k].cpu(), v) < TOL, (tag, k)
    assert set(fake_states) == {0, 1, 2, 3}
    sdo = tr.optim_D.state_dict()
    for i, (k, _) in enumerate(tr.D.named_parameters()):
        assert rel_l2(sdo["state"][i]["exp_avg_sq"], g[f"final/optim_D/{k}/exp_avg_sq"]) < TOL
        assert int(sdo["state"][i]["step"]) == steps


def test_step_at_p_half_replays_from_a_graph(monkeypatch):
    """64x256, bf16, solver.augment_p = 0.5, the trainer's own draws: 2 eager + 3 replayed steps end on the bits of 5 eager steps,
    and the draws it made hold every gate state"""
    def run(graph):
        monkeypatch.setenv("DUSTY_GAN_GRAPH", "1" if graph else "0")
        torch.manual_seed(616)
        tr = make_trainer("dusty2", (64, 256), 128, 64, 256, 8, amp=True, extra=["solver.augment_p=0.5"])
        sc = [dict(tr.step(i).items()) for i in range(5)]
        assert (tr._graph is not None) == graph
        return tr, sc
    a, sa = run(True)
    b, sb = run(False)
    for net in ("G", "D", "G_ema"):
        fa, fb = getattr(a, net).store.flat.cpu(), getattr(b, net).store.flat.cpu()
        assert torch.equal(fa, fb), (net, rel_l2(fa, fb))
    assert a.A._rng.offset == b.A._rng.offset == 5 * 2 * 4 * 8       # 2 counters per sample, 4 sets of 8 samples, 5 steps
    # what the next step would draw: mixed gates
    rp = a.A.draw_sets(4, 8, 64, 256, DEV)
    st = torch.cat([R.gate_state({k: v.cpu().long() for k, v in s.items()}) for s in rp])
    assert set(st.tolist()) == {0, 1, 2, 3}


def test_p_one_is_the_trainer_without_the_key(monkeypatch):
    """solver.augment_p = 1.0 and no controller: the same launches, the same bits, the same scalar keys"""
    monkeypatch.setenv("DUSTY_GAN_GRAPH", "1")
    out = []
    for extra in ((), ("solver.augment_p=1.0",)):
        torch.manual_seed(77)
        tr = make_trainer("dusty2", (32, 64), 8, 4, 16, 4, extra=extra)
        sc = [dict(tr.step(i).items()) for i in range(4)]
        out.append((tr, sc))
    (a, sa), (b, sb) = out
    assert sa == sb and list(sa[0]) == a._scalar_keys()[0] == b._scalar_keys()[0]
    for net in ("G", "D", "G_ema"):
        assert torch.equal(getattr(a, net).store.flat, getattr(b, net).store.flat), net
    assert a.A._rng.offset == b.A._rng.offset


def test_augment_p_out_of_range_is_refused():
    with pytest.raises(ValueError):
        make_trainer("none", (32, 64), 8, 4, 16, 4, extra=["solver.augment_p=1.5"])
