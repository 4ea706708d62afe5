"""Data-parallel exchange for the training step: one process per GPU, torch.distributed over RCCL ("nccl" backend on
ROCm) / xGMI.  Replaces what DistributedDataParallel does for the reference (trainers/dcgan_amp.py:68-69, SURVEY.md
§2.3): a parameter broadcast at construction and a gradient average per network per step.

The flat ParamStore makes each exchange ONE collective on ONE contiguous fp32 buffer (no bucketing, no per-parameter
hooks); the 1/world_size of DDP's averaging is folded into the Adam kernel (`gscale`), so the collective is a plain
SUM.  With num_accumulation > 1 the exchange happens once, after the last micro-batch (the reference's
DDP.no_sync() schedule, utils/context_manager.py:21-35).  The path shards by sample only: there is no other
collective on the data path.
"""
import os

import torch
import torch.distributed as dist


def world_size():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def rank():
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def through_backend():
    """True when the step's exchanges go through torch.distributed: several ranks - or ONE rank with an initialised
    process group and DUSTY_GAN_FORCE_SEG=1, which runs the multi-rank call pattern (async bucketed all-reduces, operand
    all-gathers, work handles waited between hipGraph segments) through RCCL on a single-GPU box
    (tests/test_gpu_ddp.py::test_single_rank_rccl_runs_the_multi_rank_schedule)."""
    if not (dist.is_available() and dist.is_initialized()):
        return False
    return dist.get_world_size() > 1 or os.environ.get("DUSTY_GAN_FORCE_SEG", "0") == "1"


def local_batch(global_batch, ngpus, num_accumulation):
    """per-GPU per-micro-batch size, with the reference's divisibility asserts (train.py:54-57)"""
    assert global_batch % ngpus == 0
    b = global_batch // ngpus
    assert b % num_accumulation == 0
    return b // num_accumulation


def broadcast_params(flats, src=0):
    """DDP's constructor broadcast: every rank starts from rank `src`'s parameters."""
    if world_size() > 1:
        for t in flats:
            dist.broadcast(t, src=src)


def broadcast_int(value, device, src=0):
    """rank `src`'s integer on every rank (< 2^63); the value itself without a process group"""
    if world_size() == 1:
        return int(value)
    t = torch.tensor([int(value)], dtype=torch.int64, device=device if dist.get_backend() == "nccl" else "cpu")
    dist.broadcast(t, src=src)
    return int(t.item())


_SIDE = {"group": None, "made": False}


def side_group():
    """A gloo process group beside an nccl default group, for decisions that must not depend on the communicator they are
    ABOUT (round-5 advice: `all_agree` ran its all-reduce on the RCCL communicator right after an aborted capture whose
    recorded nodes included RCCL collectives).  Collective: every rank calls it at the same point (the Trainer's
    constructor); None without a process group, with one rank, or when the default group already is gloo."""
    if not _SIDE["made"]:
        _SIDE["made"] = True
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1 and dist.get_backend() != "gloo":
            try:
                _SIDE["group"] = dist.new_group(backend="gloo")
            except Exception:  # noqa: BLE001  (no gloo in this build: the default group has to do)
                _SIDE["group"] = None
    return _SIDE["group"]


def all_agree(ok, device=None):
    """True iff `ok` is true on EVERY rank (a blocking MIN all-reduce of one flag; the flag itself without a process
    group).  The ranks use it to take one decision about something each of them tried alone - whether the step's
    collectives could be captured inside its hipGraph: a rank that fell back to segments while its peers replay captured
    collectives would be the only one issuing host-side calls.  Runs over the gloo side group when there is one (a CPU
    tensor over sockets: nothing the failed capture touched)."""
    if world_size() == 1:
        return bool(ok)
    side = side_group()
    if side is not None:
        t = torch.tensor([1 if ok else 0], dtype=torch.int32)
        dist.all_reduce(t, op=dist.ReduceOp.MIN, group=side)
        return bool(int(t.item()))
    dev = device if (device is not None and dist.get_backend() == "nccl") else "cpu"
    t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return bool(int(t.item()))


def capture_decision(in_graph, local_ok, everyone_ok, world):
    """What a rank does after its attempt to capture the training step (trainers/dcgan_amp.py `_step_graph`):
      "keep"      replay what was captured
      "segments"  discard it and capture again as hipGraph segments with the collectives as host calls between them
      "eager"     keep launching eagerly (a multi-rank job must not die of a refused capture)
      "raise"     single process: the failure is the caller's to see
    in_graph: the attempt had the collectives inside the capture; local_ok: this rank's capture went through;
    everyone_ok: all_agree(local_ok) - only consulted for in-graph attempts, where ONE rank falling back means ALL do."""
    if in_graph:
        return "keep" if (local_ok and everyone_ok) else "segments"
    if local_ok:
        return "keep"
    return "raise" if world == 1 else "eager"


def allreduce_grads(flat_grad, async_op=False):
    """SUM all-reduce of one network's flat gradient buffer; returns (work handle or None, gscale) where gscale is the
    factor the optimizer applies to turn the sum into DDP's average."""
    w = world_size()
    if not through_backend():
        return None, 1.0
    work = dist.all_reduce(flat_grad, op=dist.ReduceOp.SUM, async_op=async_op)
    return (work if async_op else None), 1.0 / w


def allreduce_sum(t):
    """SUM all-reduce of a small integer tensor in place (the adaptive augmentation controller's sign sum and count): every
    rank then holds the job's totals.  Nothing to do in a single process."""
    if through_backend():
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t


def mean_scalars(t):
    """one packed collective for the logged scalars (the reference does one all_reduce + .item() per key,
    trainers/dcgan_amp.py:319-323), issued asynchronously: returns (tensor, finish) where `finish()` waits for the
    exchange and returns the rank average - called when the values are first READ (the step that follows never waits for
    it; the reference blocks on every key's .item())"""
    w = world_size()
    if w == 1:
        return t, None
    work = dist.all_reduce(t, op=dist.ReduceOp.SUM, async_op=True)

    def finish():
        work.wait()
        return t / w
    return t, finish


def all_gather_pair(outs, ins):
    """two all-gathers (Proj's gradient operands) as ONE asynchronous exchange: on the nccl backend both calls are
    coalesced into one RCCL group (one enqueue on RCCL's stream, one event hand-off instead of two); elsewhere two async
    calls.  Returns something with .wait()."""
    if not through_backend():
        for o, t in zip(outs, ins):
            o.view(torch.uint8).copy_(t.contiguous().view(torch.uint8))
        return Works([])
    if dist.get_backend() == "nccl" and hasattr(dist, "_coalescing_manager"):
        # the documented fast path (no `device`): the two calls are recorded and issued as ONE
        # allgather_into_tensor_coalesced whose work handle the manager keeps.  (With `device` torch 2.10 replaces that
        # handle by group._end_coalescing(device), which may be None - a wait() that orders nothing.)
        cm = None
        try:
            with dist._coalescing_manager(async_ops=True) as cm:
                for o, t in zip(outs, ins):
                    dist.all_gather_into_tensor(o.view(torch.uint8), t.contiguous().view(torch.uint8))
        except (TypeError, AttributeError, AssertionError):   # a torch without coalesced all-gathers
            cm = None
            dist.distributed_c10d._world.pg_coalesce_state.pop(dist.distributed_c10d._get_default_group(), None)
        if cm is not None and len(cm.works) > 0:
            return cm
        # no handle to wait on: issue the two exchanges one by one (idempotent if the coalesced one did run)
    return Works([all_gather_into(o, t, async_op=True) for o, t in zip(outs, ins)])


def all_gather_cat(t):
    """concatenation over ranks of a flat device tensor (any dtype: moved as raw bytes so every backend takes it)"""
    w = world_size()
    if w == 1:
        return t
    raw = t.contiguous().view(torch.uint8)
    out = torch.empty(w * raw.numel(), dtype=torch.uint8, device=t.device)
    if dist.get_backend() == "nccl":
        dist.all_gather_into_tensor(out, raw)
    else:
        dist.all_gather(list(out.view(w, -1).unbind(0)), raw)
    return out.view(t.dtype)


def all_gather_into(out, t, async_op=False):
    """all-gather of a flat device tensor into the preallocated `out` (world * t.numel() elements, same dtype); the
    storage of `out` is reused on every step so the consumers can sit inside a captured hipGraph.  async_op: returns the
    work handle (the caller waits where the result is first needed) instead of blocking the stream."""
    w = world_size()
    raw = t.contiguous().view(torch.uint8)
    dst = out.view(torch.uint8)
    work = None
    if not through_backend():
        dst.copy_(raw)
    elif dist.get_backend() == "nccl":
        work = dist.all_gather_into_tensor(dst, raw, async_op=async_op)
    else:
        work = dist.all_gather(list(dst.view(w, -1).unbind(0)), raw, async_op=async_op)
    return work if async_op else out


class Works:
    """several work handles waited as one"""

    def __init__(self, works):
        self.works = [w for w in works if w is not None]

    def wait(self):
        for w in self.works:
            w.wait()
