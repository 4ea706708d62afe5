"""The adaptive controller of DiffAugment's p: dg_ada_update (csrc/ada.hip) bit for bit against the float32 restatement
(tests/ada_ref.py), and the trainer with `solver.ada` on - its two scalars, eager against replayed, and a resume mid-window."""
import ctypes

import numpy as np
import pytest
import torch

from tests.ada_ref import Ada, F, signs

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPECIAL = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1e-30, -1e-30]


@pytest.fixture(scope="module")
def L():
    from dusty_gan_amd import _lib
    _lib.lib()
    return _lib


def read_state(L, st):
    w = st.cpu().numpy()
    s = L.DgAdaState.from_buffer_copy(w.tobytes())
    assert ctypes.sizeof(L.DgAdaState) == 32 == w.nbytes
    return {"p": float(np.float32(s.p)), "sign_sum": int(s.sign_sum), "count": int(s.count), "steps": int(s.steps)}


def logits(B, call, kind):
    """[B] float32, all positive / all negative / mixed in sign, with special values - +-0, +-inf, NaN, tiny normals - in place of
    up to half of them (B = 1: in place of every third call's logit)"""
    g = np.random.default_rng(1000 * B + call)
    y = np.abs(g.standard_normal(B)).astype(np.float32) + np.float32(0.5)
    y = {"pos": y, "neg": -y, "mix": y * np.where(g.random(B) < 0.5, -1, 1).astype(np.float32)}[kind]
    sp = np.array(SPECIAL, dtype=np.float32)
    if B == 1:
        if call % 3 == 2:
            y[0] = sp[call % len(sp)]
    else:
        n = min(B // 2, len(sp))
        y[g.permutation(B)[:n]] = sp[:n]
    return y


@pytest.mark.parametrize("B", [1, 7, 300])
def test_ada_update_matches_the_restatement(L, B):
    """12 calls, interval 4: the p trajectory and both scalar slots, bit for bit; the step 0.25 = B * 4 / (kimg 1000) moves p through
    the clamp at 1 and back"""
    lib = L.lib()
    kimg, target, interval, p0 = B * 4 / 250.0, 0.25, 4, 0.625
    ref = Ada(p0, target=target, interval=interval, kimg=kimg, batch_size=B)
    st = torch.zeros(8, dtype=torch.int32, device=DEV)
    st[:1].view(torch.float32).fill_(p0)
    pend = torch.zeros(2, dtype=torch.int64, device=DEV)
    slots = torch.full((4,), -7.0, device=DEV)
    ps = []
    for call in range(12):
        y = logits(B, call, "pos" if call < 8 else "neg")
        yd = torch.from_numpy(y).to(DEV)
        slots[:2] = 0.0                                  # (the step's arena hands the slots out zeroed)
        L.check(lib.dg_ada_update(yd.data_ptr(), B, st.data_ptr(), pend.data_ptr(), 1, target, interval, B, kimg, 1.0,
                                  slots.data_ptr(), slots.data_ptr() + 4, None), "dg_ada_update")
        rt_w, p_w = ref.update(y)
        got = slots.cpu().numpy()
        assert got[0].tobytes() == F(rt_w).tobytes() and got[1].tobytes() == F(p_w).tobytes(), (call, got, rt_w, p_w)
        assert (got[2:] == -7.0).all()
        assert read_state(L, st) == ref.state(), call
        assert pend.cpu().tolist() == [0, 0]
        ps.append(float(p_w))
    print(f"[ada] B {B}: p = {ps}")
    assert max(ps) == 1.0 and len(set(ps)) >= 3          # the trajectory moved, and met the clamp


def test_ada_update_split_over_calls_and_ranks(L):
    """gradient accumulation and several ranks: calls that only add to the pending pair, sums added from outside (the other
    ranks'), then one call without logits that ends the iteration - the state a single call on all the logits reaches"""
    lib = L.lib()
    B, kimg, target, interval = 6, 0.024, 0.0, 1
    ya, yb = logits(B, 1, "pos"), logits(B, 2, "mix")
    ref = Ada(0.5, target=target, interval=interval, kimg=kimg, batch_size=2 * B)
    ref.add(signs(ya), B)
    ref.add(signs(yb), B)
    ref.add(3, 5)                                       # another rank's share
    p_w = ref.advance()
    st = torch.zeros(8, dtype=torch.int32, device=DEV)
    st[:1].view(torch.float32).fill_(0.5)
    pend = torch.zeros(2, dtype=torch.int64, device=DEV)
    slots = torch.zeros(2, device=DEV)
    for y in (ya, yb):
        yd = torch.from_numpy(y).to(DEV)
        L.check(lib.dg_ada_update(yd.data_ptr(), B, st.data_ptr(), pend.data_ptr(), 0, target, interval, 2 * B, kimg, 0.5,
                                  slots.data_ptr(), slots.data_ptr() + 4, None))
    assert pend.cpu().tolist() == [signs(ya) + signs(yb), 2 * B] and read_state(L, st)["steps"] == 0
    want_rt = F(F(0.5) * (F(signs(ya)) / F(B))) + F(F(0.5) * (F(signs(yb)) / F(B)))
    assert slots.cpu().numpy()[0].tobytes() == F(want_rt).tobytes()
    # three micro-batches: rt_scale = 1 / 3 is not a power of two - the product and the sum each round once, in that order
    third, acc3, slot3 = float(F(1.0) / F(3.0)), F(0.0), torch.zeros(1, device=DEV)
    pend3, st3 = torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV)
    for call in range(3):
        y = logits(7, 20 + call, "mix")
        yd = torch.from_numpy(y).to(DEV)
        L.check(lib.dg_ada_update(yd.data_ptr(), 7, st3.data_ptr(), pend3.data_ptr(), 0, target, interval, 21, kimg, third,
                                  slot3.data_ptr(), None, None))
        acc3 = F(acc3 + F(F(third) * F(F(signs(y)) / F(7))))
    assert slot3.cpu().numpy()[0].tobytes() == F(acc3).tobytes()
    pend += torch.tensor([3, 5], device=DEV)
    L.check(lib.dg_ada_update(None, 0, st.data_ptr(), pend.data_ptr(), 1, target, interval, 2 * B, kimg, 0.5, None,
                              slots.data_ptr() + 4, None))
    assert read_state(L, st) == ref.state() and slots.cpu().numpy()[1].tobytes() == F(p_w).tobytes()
    # refusals launch nothing
    for bad in (lib.dg_ada_update(None, 0, st.data_ptr(), pend.data_ptr(), 0, target, interval, B, kimg, 1.0, None, None, None),
                lib.dg_ada_update(None, 0, st.data_ptr(), pend.data_ptr(), 1, target, 0, B, kimg, 1.0, None, None, None),
                lib.dg_ada_update(None, 0, st.data_ptr(), pend.data_ptr(), 1, target, interval, B, 0.0, 1.0, None, None, None),
                lib.dg_ada_update(None, 0, None, pend.data_ptr(), 1, target, interval, B, kimg, 1.0, None, None, None)):
        assert bad == L.DG_EINVAL
    assert read_state(L, st) == ref.state()


# ---- the trainer ------------------------------------------------------------------------------------------------------------------
ADA = ["solver.augment_p=0.5", "solver.ada.target=0.6", "solver.ada.interval=2", "solver.ada.kimg=0.04"]
B = 4


def cfg(extra=(), resume=None):
    from dusty_gan_amd.utils.config import load_config
    c = load_config(["model=dcgan_eqlr", "dataset=synthetic", "dataset.shape=[32,64]", "model.gen.in_ch=8", "model.gen.ch_base=4",
                     "model.gen.ch_max=16", "model.dis.ch_base=4", "model.dis.ch_max=16", f"solver.batch_size={B}",
                     "enable_amp=false", "dataset.pool=3", *extra])
    c.resume = resume
    return c


def trainer(extra=ADA, resume=None, seed=11):
    from dusty_gan_amd.trainers.dcgan_amp import Trainer
    torch.manual_seed(seed)
    return Trainer(cfg(extra, resume), {"gpu": 0, "ngpus": 1, "batch_size": B, "num_workers": 0})


def params(t):
    return torch.cat([getattr(t, net).store.flat.cpu() for net in ("G", "D", "G_ema")])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """8 steps with the controller on: replayed (2 eager + capture + replays), eager, and 5 steps -> checkpoint (mid-window at
    interval 2) -> a new trainer resumed from it -> 3 more"""
    import os
    before = os.environ.get("DUSTY_GAN_GRAPH")
    out = {}
    for name, graph in (("graph", "1"), ("eager", "0")):
        os.environ["DUSTY_GAN_GRAPH"] = graph
        tr = trainer()
        out[name] = (tr, [dict(tr.step(i).items()) for i in range(8)])
    os.environ["DUSTY_GAN_GRAPH"] = "1"
    b = trainer()
    for i in range(5):
        b.step(i)
    d = tmp_path_factory.mktemp("ada")
    path = b.save_models("mid", 5 * B, directory=str(d))
    c = trainer(resume=path, seed=999)
    out["resumed"] = (c, [dict(c.step(i).items()) for i in range(5, 8)])
    out["path"] = path
    if before is None:
        os.environ.pop("DUSTY_GAN_GRAPH", None)
    else:
        os.environ["DUSTY_GAN_GRAPH"] = before
    return out


def test_trainer_scalars_follow_the_restatement(runs):
    tr, sc = runs["graph"]
    assert tr._graph is not None and tr.ada == {"target": 0.6, "interval": 2, "kimg": 0.04}
    assert list(sc[0])[-2:] == ["augment/rt", "augment/p"]
    ref = Ada(0.5, target=0.6, interval=2, kimg=0.04, batch_size=B)
    ps = []
    for i, s in enumerate(sc):
        k = round(s["augment/rt"] * B)
        assert abs(s["augment/rt"] * B - k) < 1e-6 and -B <= k <= B
        ref.add(k, B)
        p = ref.advance()
        assert np.float32(s["augment/p"]).tobytes() == F(p).tobytes(), (i, s["augment/p"], p)
        ps.append(float(p))
    print("[ada] trainer p:", ps, "rt:", [s["augment/rt"] for s in sc])
    assert len(set(ps)) >= 2                            # p moved: 0.2 per window of two iterations
    assert tr._ada_record() == ref.state()
    assert float(tr.A.p.item()) == ps[-1]               # the draw reads the controller's p


def test_eager_and_replayed_runs_are_bit_identical(runs):
    (a, sa), (b, sb) = runs["graph"], runs["eager"]
    assert b._graph is None
    assert torch.equal(params(a), params(b))
    assert [s["augment/p"] for s in sa] == [s["augment/p"] for s in sb] and [s["augment/rt"] for s in sa] == [s["augment/rt"] for s in sb]
    assert a._ada_record() == b._ada_record()


def test_resume_mid_window_ends_like_the_uninterrupted_run(runs):
    (a, sa), (c, sc) = runs["graph"], runs["resumed"]
    st = torch.load(runs["path"], weights_only=True)["resume_state"]["ada"]
    assert set(st) == {"p", "sign_sum", "count", "steps"} and st["steps"] == 5 and st["count"] == B   # one iteration into a window
    assert sc == sa[5:]
    assert c._ada_record() == a._ada_record()
    assert torch.equal(params(a), params(c))


def test_checkpoint_without_the_record_starts_at_augment_p(runs, tmp_path):
    sd = torch.load(runs["path"], weights_only=False)
    sd["resume_state"].pop("ada")
    path = str(tmp_path / "no_ada.pth")
    torch.save(sd, path)
    d = trainer(resume=path, seed=999)
    assert d._ada_record() == {"p": 0.5, "sign_sum": 0, "count": 0, "steps": 0}


def test_without_the_controller_nothing_is_added():
    tr = trainer(extra=())
    assert tr.ada is None and tr.A.p == 1.0 and "augment/p" not in tr._scalar_keys()[0] and tr._snap_n() == 8
    assert "ada" not in tr._position()
    off = trainer(extra=["solver.augment_p=0.25", "solver.ada.target=null"])
    assert off.ada is None and off.A.p == 0.25
    for bad in ("solver.ada.interval=0", "solver.ada.kimg=0", "solver.ada.kimg=-1", "solver.ada.target=1.5"):
        with pytest.raises(ValueError, match=bad.split("=")[0].replace(".", r"\.")):
            trainer(extra=["solver.ada.target=0.6", bad] if "target" not in bad else [bad])
