"""The four routes of Proj.weight's gradient (trainers/dcgan_amp.py `ProjRoute`) in one process: each environment
configuration takes the route it names, `FlatAdam.regen_grad` is set exactly on the in-optimizer routes, and three steps on
any route train like three steps with the gradient materialised by the backward pass."""
import pytest
import torch

from tests.golden_util import rel_l2
from tests.test_gpu_step import make_trainer

pytestmark = pytest.mark.gpu

# route -> the environment that selects it (one rank, bf16, one micro-batch, beta1 = 0)
CONFIGS = {
    "MATERIALISED": {"DUSTY_GAN_FUSE_PROJ": "0"},
    "FUSED": {},
    "GATHER": {"DUSTY_GAN_FORCE_SEG": "1", "DUSTY_GAN_FUSE_PROJ": "0"},
    "GATHER_FUSED": {"DUSTY_GAN_FORCE_SEG": "1"},
}
_RUNS = {}


def _run(name, pl):
    """3 eager steps of the smallest net whose Proj the optimizer's MFMA epilogue takes (tests/test_gpu_ddp.py fused_worker:
    nz = 128, 2 * 4 * 16 = 128 rows, 40 samples), once per (configuration, pl)"""
    if (name, pl) not in _RUNS:
        with pytest.MonkeyPatch.context() as mp:
            for k in ("DUSTY_GAN_FUSE_PROJ", "DUSTY_GAN_FUSE_PROJ_FP32", "DUSTY_GAN_FORCE_SEG"):
                mp.delenv(k, raising=False)
            mp.setenv("DUSTY_GAN_GRAPH", "0")
            for k, v in CONFIGS[name].items():
                mp.setenv(k, v)
            torch.manual_seed(400)
            tr = make_trainer("dusty1", True, (32, 64), 128, 4, 16, 40, amp=True, pl=pl)
            for i in range(3):
                tr.step(i)
            torch.cuda.synchronize()
            _RUNS[(name, pl)] = {"route": tr.proj_route, "regen": tr.optim_G.regen_grad is not None,
                                 "G": tr.G.store.flat.cpu(), "E": tr.G_ema.store.flat.cpu(), "V": tr.G.store.v.cpu()}
    return _RUNS[(name, pl)]


@pytest.mark.parametrize("pl", [0.0, 2.0])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_each_configuration_takes_its_route_and_trains_like_the_materialised_one(name, pl):
    from dusty_gan_amd.trainers.dcgan_amp import ProjRoute
    got = _run(name, pl)
    assert got["route"] is ProjRoute[name], got["route"]
    assert got["regen"] == ProjRoute[name].in_optimizer
    if name == "MATERIALISED":
        return
    ref = _run("MATERIALISED", pl)
    assert ref["route"] is ProjRoute.MATERIALISED and not ref["regen"]
    # the bounds tests/test_gpu_ddp.py::test_two_ranks_fused_proj_optimizer_matches_unfused holds for this net and step count
    # (fused against unfused: same bf16 operands, same fp32 accumulation; an atomics-reordered last bit may flip one pixel of
    # the hard Gumbel threshold)
    for key, bound in (("G", 2e-3), ("E", 2e-3), ("V", 5e-2)):
        err = rel_l2(got[key], ref[key])
        print(f"{name} pl={pl} {key}: rel-L2 {err:.3e}")
        assert err < bound, (name, pl, key, err)
