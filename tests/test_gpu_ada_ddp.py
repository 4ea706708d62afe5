"""The adaptive augmentation controller with several ranks: every rank must apply the SAME adjustment, so the iteration's integer
sign sum and count are summed over the ranks (utils/dist.py allreduce_sum) before the window takes them.  Two ranks over RCCL on two
devices (skipped on a one-GPU box, as tests/test_gpu_ddp.py's RCCL tests are), and the same two ranks sharing one GPU over gloo."""
import datetime
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.ada_ref import Ada, F

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
PG_TIMEOUT = datetime.timedelta(seconds=240)
B, STEPS = 8, 6
ADA = ["solver.augment_p=0.5", "solver.ada.target=0.6", "solver.ada.interval=2", "solver.ada.kimg=0.08"]   # 8 * 2 / 80 = 0.2 a window


def worker(rank, world, init_file, out_dir, backend):
    from dusty_gan_amd.trainers.dcgan_amp import Trainer
    from dusty_gan_amd.utils.config import load_config
    if backend == "nccl":
        torch.cuda.set_device(rank)
        dist.init_process_group("nccl", init_method=f"file://{init_file}", rank=rank, world_size=world,
                                device_id=torch.device("cuda", rank), timeout=PG_TIMEOUT)
    else:
        dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world, timeout=PG_TIMEOUT)
    torch.manual_seed(300)
    cfg = load_config(["model=dcgan_eqlr", "dataset=synthetic", "dataset.shape=[32,64]", "model.gen.in_ch=8", "model.gen.ch_base=4",
                       "model.gen.ch_max=16", "model.dis.ch_base=4", "model.dis.ch_max=16", f"solver.batch_size={B}",
                       "enable_amp=false", "dataset.pool=3", *ADA])
    tr = Trainer(cfg, {"gpu": rank if backend == "nccl" else 0, "ngpus": world, "batch_size": B // world, "num_workers": 0})
    scal = [dict(tr.step(i).items()) for i in range(STEPS)]
    torch.save({"scal": scal, "ada": tr._ada_record(), "p": float(tr.A.p.item()), "D": tr.D.store.flat.cpu()},
               os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def check(outs):
    a, b = outs
    assert a["ada"] == b["ada"] and a["p"] == b["p"] and torch.equal(a["D"], b["D"])
    ref = Ada(0.5, target=0.6, interval=2, kimg=0.08, batch_size=B)
    for i, s in enumerate(a["scal"]):
        k = round(s["augment/rt"] * B)              # the rank mean of the ranks' mean signs: the job's sign sum / B
        assert abs(s["augment/rt"] * B - k) < 1e-5
        ref.add(k, B)
        p = ref.advance()
        assert np.float32(s["augment/p"]).tobytes() == F(p).tobytes(), (i, s["augment/p"], p)
    assert a["ada"] == ref.state()


def run(backend):
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(worker, args=(2, os.path.join(td, "init"), td, backend), nprocs=2, join=True)
        return [torch.load(os.path.join(td, f"r{r}.pt")) for r in range(2)]


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="RCCL needs one device per rank: this box has one GPU")
def test_two_ranks_over_rccl_move_p_together():
    check(run("nccl"))


def test_two_ranks_on_one_gpu_move_p_together():
    check(run("gloo"))
