"""`model.gen.tau: null` under the captured step graph and under gradient accumulation.  The head kernels read the temperature
weights from the fp32 master in memory, so a replayed graph follows the training: 2 eager + 3 replayed steps end on the very bits of
5 eager steps (the temperature sums travel through the fixed-point slots: no sum on this path depends on the order of its terms)."""
import pytest
import torch

from oracle import dusty_oracle as O
from tests.golden_util import rel_l2
from tests.test_gpu_learnable_tau_step import make_trainer
from tests.test_gpu_step import grads_by_name

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_learnable_tau_step_replays_from_a_graph(monkeypatch):
    """dusty2, 64x256, bf16, B = 8: the same parameters, bit for bit, after 2 eager + 3 replayed steps as after 5 eager steps from
    one seed - both temperature weights trained (non-zero; at beta1 = 0 Adam moves a weight by about lr a step: |w| <= 5 lr)"""
    def run(graph):
        monkeypatch.setenv("DUSTY_GAN_GRAPH", "1" if graph else "0")
        torch.manual_seed(616)
        tr = make_trainer("dusty2", (64, 256), 128, 64, 256, 8, amp=True)
        sc = [dict(tr.step(i).items()) for i in range(5)]
        assert (tr._graph is not None) == graph
        if graph:
            assert sum(isinstance(g, torch.cuda.CUDAGraph) for g in tr._graph) == 1
        return tr, sc
    a, sa = run(True)
    b, sb = run(False)
    for net in ("G", "D", "G_ema"):
        fa, fb = getattr(a, net).store.flat.cpu(), getattr(b, net).store.flat.cpu()
        assert torch.equal(fa, fb), (net, rel_l2(fa, fb))
    for x, y in zip(sa, sb):
        for k in x:
            assert abs(x[k] - y[k]) <= 1e-6 * max(1.0, abs(y[k])), (k, x[k], y[k])
    lr = float(a.optim_G.lr)
    w = a.G.store.view("tau_w").cpu()
    print("TAU WEIGHTS after 5 steps (lr %g):" % lr, w.tolist(), "G_ema:", a.G_ema.store.view("tau_w").cpu().tolist())
    assert w.numel() == 2 and bool((w != 0).all()) and bool((w.abs() <= 5 * lr).all()), (w, lr)
    assert bool((a.G_ema.store.view("tau_w") != 0).all())
    # the wrapper's parameters are views of the store: the state dict carries what the graph trained
    sd = a.G.state_dict()
    assert [float(sd["gumbel_pixel.weight"]), float(sd["gumbel_image.weight"])] == w.tolist()


def test_gradient_accumulation_equals_full_batch_with_learnable_tau():
    """num_accumulation = 2 with micro-batches of B / 2 == one batch of B (32x64, fp32), the temperature gradients included"""
    arch, shape, nz, cb, cm, B = "dusty2", (32, 64), 8, 4, 16, 4
    tr1 = make_trainer(arch, shape, nz, cb, cm, B)
    tr2 = make_trainer(arch, shape, nz, cb, cm, B // 2, n_acc=2)
    sd = tr1.G.state_dict()
    sd["gumbel_pixel.weight"], sd["gumbel_image.weight"] = torch.tensor(0.3), torch.tensor(-0.7)   # (off the symmetric start)
    for tr in (tr1, tr2):
        tr.G.load_state_dict(sd)
        tr.D.load_state_dict(tr1.D.state_dict())
        tr.G_ema.load_state_dict(sd)
    gen = torch.Generator().manual_seed(5)
    H, W = shape
    x = torch.rand(B, 1, H, W, generator=gen) * 2 - 1
    m = torch.ones(B, 1, H, W)
    rand = {"z": torch.randn(B, nz, generator=gen),
            "noise": {"pixel": O.logistic_noise(torch.rand(B, 1, H, W, generator=gen), torch.rand(B, 1, H, W, generator=gen)),
                      "image": O.logistic_noise(torch.rand(B, 1, 1, 1, generator=gen), torch.rand(B, 1, 1, 1, generator=gen))},
            "aug": [O.draw_augment_params(B, H, W, gen) for _ in range(4)]}

    def half(r, s):
        return {"z": r["z"][s], "noise": {k: v[s] for k, v in r["noise"].items()},
                "aug": [{k: v[s] for k, v in rp.items()} for rp in r["aug"]]}
    xd, md = x.to(DEV), m.to(DEV)
    h = B // 2
    tr1.optimize_D(reals=[(xd, md)], rands=[rand])
    tr2.optimize_D(reals=[(xd[:h].contiguous(), md[:h]), (xd[h:].contiguous(), md[h:])],
                   rands=[half(rand, slice(0, h)), half(rand, slice(h, B))])
    tr1.optimize_G()
    tr2.optimize_G()
    g1, g2 = grads_by_name(tr1.optim_G), grads_by_name(tr2.optim_G)
    assert list(g1)[-2:] == ["gumbel_pixel.weight", "gumbel_image.weight"]
    for k in g1:
        assert rel_l2(g2[k], g1[k]) < 1e-4, (k, g1[k] if g1[k].numel() == 1 else None, g2[k] if g2[k].numel() == 1 else None)
    assert float(g1["gumbel_pixel.weight"]) != 0.0 and float(g1["gumbel_image.weight"]) != 0.0
