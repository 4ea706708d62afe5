#!/usr/bin/env python3
"""Benchmark of the dusty-gan training hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W
    (N > 1: either under a launcher - python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N
     ... - or bare: with no WORLD_SIZE in the environment bench.py starts the N ranks itself and relays rank 0's line)

One "step" = one `Trainer.step` (D update + G update + EMA, reference trainers/dcgan_amp.py:162-325) on synthetic
64x1024 range images resident in HBM, 32 images per GPU (weak scaling).  Prints ONE JSON line on rank 0:
metric = G+D training throughput in images/s (whole job), with steps/s beside it, a `roofline` object for the
dominant kernel (HIP-event timed) and a `cpu_baseline` object (the CPU oracle timed on the host cores, N=1 only).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

# dense MFMA peaks, /opt/skills/guides/MI355X_MICROARCH.md.  fp32x3: every product is three bf16 products
# (x_hi w_hi + x_lo w_hi + x_hi w_lo on operands stored as split-bf16 pairs, DG_BF16X2): a third of the bf16 rate in
# fp32-equivalent FLOPs.  (Round 4 split fp32 operands in registers, two half-used matrix instructions per 4 k: 1/8.)
PEAK_TFLOPS = {"bf16": 2500.0, "fp32": 157.3, "fp32x3": 833.3}
PEAK_HBM_GBS = 8000.0
PEAK_CLOCK_GHZ = 2.4   # the clock the dense peaks are quoted at


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--precision", choices=["bf16", "fp32", "fp32x3"], default="bf16",
                    help="bf16: the timed mode; fp32: exact parity mode; fp32x3: fp32 parameters, split-bf16 pairs on the bf16 kernels")
    ap.add_argument("--arch", choices=["none", "dusty1", "dusty2"], default=None,
                    help="default: BASELINE configs[1] (dcgan_eqlr baseline) at every N - one weak-scaling series; dusty2 = configs[3]'s model")
    ap.add_argument("--batch", type=int, default=32, help="images per GPU per step")
    ap.add_argument("--shape", type=int, nargs=2, default=[64, 1024])
    ap.add_argument("--gp", type=float, default=1.0, help="R1 weight (solver.loss.gp); 0 disables R1")
    ap.add_argument("--pl", type=float, default=0.0, help="path-length weight (solver.loss.pl); 0 = the shipped solver")
    ap.add_argument("--no-augment", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the short lines for BASELINE configs 3 / 4-share / 5-share appended after the timed region")
    ap.add_argument("--other-steps", type=int, default=10, help="timed steps of each appended configuration")
    ap.add_argument("--soak-steps", type=int, default=2000,
                    help="replayed steps of the long window appended behind the timed region (N = 1 headline run; 0 = none)")
    ap.add_argument("--no-clock", action="store_true", help="skip the held-clock probe (scripts/conv_clock.py on the diagnostic library)")
    ap.add_argument("--cpu-batch", type=int, default=32, help="batch of the bounded CPU-oracle sample (default: the workload's own)")
    ap.add_argument("--cpu-steps", type=int, default=2, help="timed oracle steps of the CPU sample (~13 s of CPU work at batch 32)")
    ap.add_argument("--cpu-threads", type=int, default=16, help="host threads for the CPU-oracle sample")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (its scalars, the updated G / D / G_ema) as DIR/<name>.npy")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def make_trainer(args, rank, local_rank, world):
    from dusty_gan_amd.trainers.dcgan_amp import Trainer
    from dusty_gan_amd.utils.config import load_config
    # the metric's configuration (BASELINE.json configs[1]: dcgan_eqlr baseline, 64x1024, 32 images per GPU) at every N,
    # so that the 1/2/4/8-GPU values are one weak-scaling series; --arch dusty1|dusty2 selects the DUSty variants
    arch = args.arch or "none"
    model = {"none": "dcgan_eqlr", "dusty1": "dusty1_dcgan_eqlr", "dusty2": "dusty2_dcgan_eqlr"}[arch]
    ov = [f"model={model}", "dataset=synthetic", f"dataset.shape=[{args.shape[0]},{args.shape[1]}]",
          f"solver.batch_size={args.batch * world}", f"solver.loss.gp={args.gp}", f"solver.loss.pl={args.pl}",
          f"enable_amp={'true' if args.precision == 'bf16' else 'false'}"]
    if args.no_augment:
        ov.append("solver.augment=[]")
    cfg = load_config(ov)
    torch.manual_seed(1234 + rank)
    os.environ["DUSTY_GAN_FP32_SPLIT"] = "1" if args.precision == "fp32x3" else "0"   # (read by the Trainer's constructor)
    tr = Trainer(cfg, {"gpu": local_rank, "ngpus": world, "batch_size": args.batch, "num_workers": 0})
    return tr, arch


def flops_per_sample(shape, arch, gp):
    """Algorithmic FLOPs the schedule executes per sample per step (2*MAC, no border waste): SURVEY.md §8d's F_G/F_D
    at this shape, with 3 F_G + 10 F_D passes when R1 is on (one D(real) forward and one backward-data pass fewer
    than the reference's 12) and 3 F_G + 8 F_D without."""
    H, W = shape
    s = (H * W) / (64 * 1024)
    n_out = {"none": 1, "dusty1": 2, "dusty2": 3}[arch]
    f_g = 2 * (67108864 + 3 * 536870912 + 16777216 * n_out) * s
    f_d = 2 * (393216 + 33554432 + 3 * 536870912 + 131072) * s
    return 3 * f_g + (10 if gp > 0 else 8) * f_d, f_g, f_d


def step_model(shape, arch, gp, batch, es, P_G, P_D):
    """Whole-step roofline terms per GPU (on the schedule that is EXECUTED - DESIGN.md §3):
    T_flop  = executed conv FLOPs / dense MFMA peak;
    T_bytes = minimal HBM bytes / 8 TB/s, where the bytes are
      * generator parameters: optimizer + EMA read p, v, ema and write p, v, ema (24 B) + the low-precision shadow the
        kernels read (written once, read by the forward and by the backward-data pass): 24 + 3 es bytes per parameter
        (Proj.weight's gradient is formed inside the optimizer from 17 MB of operands and never stored; beta1 = 0 so
        exp_avg is neither read nor written);
      * discriminator parameters: SURVEY's 17 fp32 streams (4 forward reads, 5 backward reads, gradient, 7 Adam);
      * activations: every feature map / image of every executed pass written once and read once in the compute type:
        2 es B (3 A_G + n_D A_D) with n_D = 10 (R1 on) or 8 executed discriminator passes."""
    H, W = shape
    n_out = {"none": 1, "dusty1": 2, "dusty2": 3}[arch]
    hw = H * W
    a_g = hw * (512 / 256 + 256 / 64 + 128 / 16 + 64 / 4 + n_out)   # a0..a3 on their grids + the head images
    a_d = hw * (1 + 2 + 64 / 4 + 128 / 16 + 256 / 64 + 512 / 256)   # image, BlurVH pair, h1..h4
    n_d = 10 if gp > 0 else 8
    fl, _, _ = flops_per_sample(shape, arch, gp)
    nbytes = P_G * (24 + 3 * es) + P_D * 17 * 4 + 2 * es * batch * (3 * a_g + n_d * a_d)
    return fl * batch, nbytes


def roofline_pass(tr, steps=6):
    """Instrumented steps (HIP events on the launch stream around every conv / wgrad launch), run right after the
    timed region on the same workload.  Every step issues the same launches in the same order, so each launch position has
    `steps` samples: its time is their MEDIAN (round 5 summed two eager steps and read 9 % off the replayed step's kernel
    trace on a box with a long tail).  Returns per family: ms / flops / bytes / launches PER STEP."""
    from dusty_gan_amd import engine as E
    import statistics
    E.PROFILE = []
    marks = [0]
    for i in range(steps):
        tr.step(i)
        marks.append(len(E.PROFILE))
    torch.cuda.synchronize()
    rec, E.PROFILE = E.PROFILE, None
    per = [rec[marks[i]:marks[i + 1]] for i in range(steps)]
    n0 = len(per[0])
    same = all(len(p) == n0 and all(a[0] == b[0] and a[5] == b[5] for a, b in zip(p, per[0])) for p in per)
    if not same:   # (never seen; fall back to plain sums over the steps that look like the first)
        per = [p for p in per if len(p) == n0] or per[:1]
    fam = {}
    detail = {}
    for k in range(n0):
        name, flops, nbytes, _, _, tag = per[0][k]
        ms = statistics.median(p[k][3].elapsed_time(p[k][4]) for p in per)
        d = detail.setdefault((name, tag), [0.0, 0.0, 0])
        d[0] += ms
        d[1] += flops
        d[2] += 1
        f = fam.setdefault(name, {"ms": 0.0, "flops": 0.0, "bytes": 0.0, "n": 0})
        f["ms"] += ms
        f["flops"] += flops
        f["bytes"] += nbytes
        f["n"] += 1
    if os.environ.get("DUSTY_BENCH_DETAIL"):
        for (name, tag), (ms, fl, n) in sorted(detail.items(), key=lambda kv: -kv[1][0]):
            print(f"  {name:20s} {tag:40s} n={n:3d} avg {1e3 * ms / n:8.1f} us  {fl / (ms * 1e-3) / 1e12:7.1f} TFLOP/s",
                  file=sys.stderr)
    for f in fam.values():
        f["steps"] = len(per)
    return fam


def soak(tr, steps):
    """`steps` more replayed steps of the timed workload with a HIP event after each (same protocol as the timed region: the
    previous step's scalars are read back while the next runs): the long window behind the K-step headline - percentiles of
    the per-step device time and the wall-clock mean."""
    import gc
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    gc.collect()
    gc.disable()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    marks[0].record()
    prev = None
    for i in range(steps):
        cur = tr.step(i)
        marks[i + 1].record()
        if prev is not None:
            _ = list(prev.values())
        prev = cur
        if i % 100 == 99:
            progress(f"soak step {i + 1}")      # (N > 1: the supervisor watches for progress lines)
    _ = list(prev.values())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    gc.enable()
    per = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
    q = lambda f: round(per[min(len(per) - 1, int(f * len(per)))], 4)
    return {"steps": steps, "ms_per_step_wall": round(1e3 * dt / steps, 4), "seconds": round(dt, 2),
            "step_ms_device": {"p10": q(0.10), "p50": q(0.50), "p90": q(0.90), "p99": q(0.99), "min": round(per[0], 4),
                               "max": round(per[-1], 4)}}


DUMP_SAMPLE = 1 << 18   # elements kept of a larger tensor: G's 67M-element projection alone would be 268 MB


def dump_outputs(tr, scal, path):
    """What the timed path hands its caller after its last step: the step's scalars (float64) and the networks it updated in
    place - the G, D and G_ema state dicts (float32) - as <path>/<name>.npy.  A tensor of more than DUMP_SAMPLE elements is
    stored as a sample of its flattened elements: the same seeded, sorted indices in every run, so that two builds run with
    the same arguments (hence the same seeded inputs) can be compared file for file.  About 10 MB at the default workload."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for k, v in scal.items():
        np.save(os.path.join(path, "scalar." + k.replace("/", ".") + ".npy"), np.array(v, np.float64))
    for net in ("G", "D", "G_ema"):
        for k, v in getattr(tr, net).state_dict().items():
            v = v.detach()
            if v.numel() > DUMP_SAMPLE:
                idx = np.sort(np.random.default_rng(0).choice(v.numel(), DUMP_SAMPLE, replace=False))
                v = v.reshape(-1)[torch.from_numpy(idx).to(v.device)]
            np.save(os.path.join(path, f"{net}.{k}.npy"), v.float().cpu().numpy())


def held_clock():
    """the clock the chip holds inside the dominant conv kernel: scripts/conv_clock.py on the diagnostic build of the
    library (built by __graft_entry__.build()), as a CHILD process after the timed region; None when that library is absent"""
    import subprocess
    diag = os.path.join(ROOT, "dusty_gan_amd", "csrc", "libdustygan_hip_diag.so")
    if not os.path.exists(diag):
        return None, "no diagnostic library (make -C dusty_gan_amd/csrc diag DIAGBITS=8)"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["DUSTY_GAN_LIB_DIAG"] = "1"
    try:
        res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "conv_clock.py"), "2"], capture_output=True,
                             text=True, timeout=120, env=env)
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
        if res.returncode != 0 or not line:
            return None, f"conv_clock.py exited {res.returncode}: {res.stderr[-200:]}"
        r = json.loads(line[-1])
        return r.get("clock_ghz"), r
    except Exception as e:  # noqa: BLE001
        return None, f"{type(e).__name__}: {e}"


def cpu_baseline(args, arch):
    """The CPU oracle (oracle/dusty_oracle.py: the reference's algorithm in stock torch CPU ops, validated against the
    reference's modules) timed on this host: one warm-up + `--cpu-steps` timed steps of the SAME workload (batch 32 at
    64x1024: 6.6 s per step on 16 threads of the GPU box; the batch-4 sample of rounds 1-2 ran 1.3x more images/s)."""
    from oracle import dusty_oracle as O
    # torch's CPU conv kernels stop scaling (and then collapse) far below this host's thread count at batch 4:
    # measured on the GPU box (scripts/cpu_threads.py: 8/16/32/64/128 threads -> 0.85/0.73/0.86/1.27/2.83 s per
    # batch-4 step), 16 threads are the fastest; all 256 take 133 s.
    torch.set_num_threads(min(args.cpu_threads, os.cpu_count() or 1))
    H, W = args.shape
    B = args.cpu_batch
    gen = torch.Generator().manual_seed(0)
    G = O.init_G(f"{arch}/dcgan_eqlr", 512, 64, 512, (H, W), gen)
    D = O.init_D(1, 64, 512, (H, W), gen)
    G_ema = {k: v.clone() for k, v in G.items()}
    oG, oD = O.new_optim_state(G), O.new_optim_state(D)
    policy = () if args.no_augment else ("brightness", "saturation", "contrast", "translation", "cutout")
    cfg = O.StepConfig(arch=arch, w_gp=args.gp, policy=policy)
    times = []
    for it in range(1 + args.cpu_steps):
        x = torch.rand(B, 1, H, W, generator=gen) * 2 - 1
        rand = {"z": torch.randn(B, 512, generator=gen),
                "noise": {"pixel": O.logistic_noise(torch.rand(B, 1, H, W, generator=gen), torch.rand(B, 1, H, W, generator=gen)),
                          "image": O.logistic_noise(torch.rand(B, 1, 1, 1, generator=gen), torch.rand(B, 1, 1, 1, generator=gen))},
                "aug": [O.draw_augment_params(B, H, W, gen) for _ in range(4)]}
        t0 = time.perf_counter()
        O.train_step(G, D, G_ema, oG, oD, it + 1, cfg, x, rand)
        times.append(time.perf_counter() - t0)
    t = sum(times[1:]) / len(times[1:])
    return {"value": round(B / t, 3), "unit": "images/s", "steps_per_sec_at_sample_batch": round(1.0 / t, 4),
            "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"{len(times) - 1} timed oracle steps (after 1 warm-up) at batch {B} of {args.batch}, {H}x{W}, "
                      f"fp32, stock torch CPU ops, {sum(times[1:]):.1f} s of CPU work"}


def kernel_source_sha():
    """sha256 over the kernel sources (csrc/*.hip, *.h, sorted): identifies the code a PMC collection was made on.  (The
    GPU box has no .git, so a commit id cannot be checked there; the sources can.)"""
    import glob
    import hashlib
    h = hashlib.sha256()
    root = os.path.join(ROOT, "dusty_gan_amd", "csrc")
    for path in sorted(glob.glob(os.path.join(root, "*.hip")) + glob.glob(os.path.join(root, "*.h"))):
        h.update(os.path.basename(path).encode())
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def bench_config_key(args, arch):
    """the workload a PMC collection belongs to"""
    return {"arch": arch, "shape": list(args.shape), "batch": args.batch, "precision": args.precision, "gp": args.gp,
            "pl": args.pl, "augment": not args.no_augment}


PMC_FILE = "profiles/r06_pmc_traffic.json"


def pmc_traffic(kernel, args, arch):
    """HBM-side bytes per launch of `kernel` from the committed rocprofv3 PMC passes (FETCH_SIZE / WRITE_SIZE cannot be
    collected from inside the process; profiles/README.md says how the file is made: scripts/pmc_traffic.py).  The file
    records the hash of the kernel sources AND the workload it was collected on; a number from other sources or another
    configuration is reported as null, never copied."""
    path = os.path.join(ROOT, PMC_FILE)
    try:
        with open(path) as f:
            d = json.load(f)
        if d.get("kernel_source_sha") != kernel_source_sha():
            return None, f"stale: collected on sources {d.get('kernel_source_sha')}, running {kernel_source_sha()}"
        if d.get("config") != bench_config_key(args, arch):
            return None, f"collected on another configuration ({d.get('config')})"
        return round(d["kernels"][kernel]["bytes_per_launch"]), f"{PMC_FILE} @ {d.get('git_sha', '?')}"
    except (OSError, KeyError, ValueError) as e:
        return None, f"not collected ({type(e).__name__})"


def pmc_step_traffic(args, arch):
    """measured HBM-side bytes of one whole step (every kernel of the PMC passes, divided by the steps the passes ran) and
    the three big families' shares - beside `roofline.step.bytes`, the minimal-traffic model; None unless collected on
    these sources and this workload"""
    try:
        with open(os.path.join(ROOT, PMC_FILE)) as f:
            d = json.load(f)
        if d.get("kernel_source_sha") != kernel_source_sha() or d.get("config") != bench_config_key(args, arch):
            return None
        return {"bytes": round(d["all_kernels"]["bytes_per_step"]), "steps_in_trace": d["steps"],
                "families": {k: round(v["bytes_per_step"]) for k, v in d["kernels"].items()}, "source": PMC_FILE}
    except (OSError, KeyError, ValueError):
        return None


def other_config_lines(args):
    """Short runs of BASELINE.json's other single-GPU workloads AFTER the timed region of the headline configuration (so
    the driver's record carries them too): configs[2] dusty1, configs[3]'s per-GPU share (dusty2, 32 images), configs[4]'s
    per-GPU share (dusty2, 128x2048, 64 images).  Same protocol at a smaller K.  Each one runs in a freshly started CHILD
    process of this file (subprocess, never exec: this process has initialised the GPU) under a timeout, so a HIP fault,
    an out-of-memory kill or a hang in an appended configuration costs its own entry, never the headline record."""
    import subprocess
    out = {}
    for tag, arch, shape, batch, prec, gp, extra in (
            ("config3_dusty1_64x1024_b32", "dusty1", [64, 1024], 32, args.precision, args.gp, []),
            ("config4_share_dusty2_64x1024_b32", "dusty2", [64, 1024], 32, args.precision, args.gp, []),
            ("config5_share_dusty2_128x2048_b64", "dusty2", [128, 2048], 64, args.precision, args.gp, []),
            # SURVEY 8d, config 2 as BASELINE.json words it (no R1, no DiffAugment named): solver.loss.gp=0 solver.augment=[]
            ("config2_nogp_noaug", "none", [64, 1024], 32, args.precision, 0.0, ["--no-augment"]),
            # the headline workload in the fast parity mode (<= 1e-3 tolerance class)
            ("config2_none_64x1024_b32_fp32x3", "none", [64, 1024], 32, "fp32x3", args.gp, [])):
        cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--arch", arch, "--shape", str(shape[0]), str(shape[1]),
               "--batch", str(batch), "--steps", str(args.other_steps), "--warmup", "5", "--precision", prec,
               "--gp", str(gp), "--pl", str(args.pl), "--no-roofline", "--no-cpu-baseline", "--no-other-configs",
               "--soak-steps", "0", "--no-clock"] + extra
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env)
            line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
            if res.returncode != 0 or not line:
                out[tag] = {"error": f"child exited {res.returncode}: {res.stderr[-300:]}"}
                continue
            r = json.loads(line[-1])
            out[tag] = {"ms_per_step": r["ms_per_step"], "images_per_sec": r["value"], "steps": r["steps"], "warmup": r["warmup"],
                        "dtype": r["dtype"], "launch_mode": r["launch_mode"], "step_ms_device_p50": r["step_ms_device"]["p50"],
                        "step_flops_fraction_of_mfma_peak": r["step_flops_fraction_of_mfma_peak"]}
        except subprocess.TimeoutExpired:
            out[tag] = {"error": "child timed out after 240 s"}
        except Exception as e:  # noqa: BLE001  (instrumentation after the timed region: never at the price of the line)
            out[tag] = {"error": f"{type(e).__name__}: {e}"}
    return out


# ---------------------------------------------------------------------------------------------------------------------
# N > 1: every rank is a SUPERVISOR that starts the measuring process as a child and never touches the GPU itself.
# The default multi-rank schedule replays RCCL collectives captured inside the step's hipGraph; no box this repository
# has been measured on had two GPUs, so a deadlock of that form at replay must cost one attempt, not the record:
#   attempt 0  collectives inside the one graph          (the trainer's default on the nccl backend)
#   attempt 1  DUSTY_GAN_GRAPH_COMM=0: hipGraph segments with the collectives as host calls between them
#   attempt 2  DUSTY_GAN_GRAPH_DDP=0:  eager launches
# A child that dies, stops making progress for STALL seconds or exceeds CAP seconds fails the attempt for ALL ranks (a flag
# in the launcher's TCP store); every supervisor then kills its child's process group and starts a NEW child of the next
# mode on a fresh rendezvous port - never a re-exec or a restart inside a process that has initialised the GPU.
# Reference: train.py:44-57,185-186 (one worker per GPU, file-store rendezvous, no retry of any kind).
ATTEMPTS = (("collectives inside the hipGraph", {}),
            ("hipGraph segments, collectives between them", {"DUSTY_GAN_GRAPH_COMM": "0"}),
            ("eager launches", {"DUSTY_GAN_GRAPH_COMM": "0", "DUSTY_GAN_GRAPH_DDP": "0"}))


def progress(what):
    """the measuring child tells its supervisor that it is alive (one appended line per phase / step)"""
    path = os.environ.get("DUSTY_BENCH_PROGRESS")
    if path:
        try:
            with open(path, "a") as fh:
                fh.write(f"{time.time():.3f} {what}\n")
        except OSError:
            pass


def _supervisor_store(rank, world):
    """the key-value store the supervisors coordinate through: the launcher's own TCP store (torch.distributed.run keeps
    one at MASTER_ADDR:MASTER_PORT and tells its workers to join it as clients), else one hosted by rank 0's supervisor"""
    import datetime
    addr, port = os.environ.get("MASTER_ADDR", "127.0.0.1"), int(os.environ["MASTER_PORT"])
    agent = os.environ.get("TORCHELASTIC_USE_AGENT_STORE", "") == "True"
    return dist.TCPStore(addr, port, None, (not agent) and rank == 0, timeout=datetime.timedelta(seconds=120),
                         wait_for_workers=False)


def _kill_group(proc):
    import signal
    try:
        os.killpg(proc.pid, signal.SIGKILL)
    except (ProcessLookupError, PermissionError):
        pass
    try:
        proc.wait(timeout=30)
    except Exception:  # noqa: BLE001
        pass


def supervise(args):
    """run the measuring child of this rank through ATTEMPTS (see above); rank 0 relays the successful child's JSON line"""
    import socket
    import subprocess
    import tempfile
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ["WORLD_SIZE"])
    stall = float(os.environ.get("DUSTY_BENCH_STALL_S", "180"))     # no progress line for this long = hung
    cap = float(os.environ.get("DUSTY_BENCH_CAP_S", "600"))         # wall-clock budget of one attempt
    first = int(os.environ.get("DUSTY_BENCH_FIRST_ATTEMPT", "0"))
    child_cmd = os.environ.get("DUSTY_BENCH_CHILD_CMD")             # (tests: a stand-in for the measuring process)
    store = _supervisor_store(rank, world)
    pfx = f"dusty_bench/{os.environ.get('TORCHELASTIC_RUN_ID', 'x')}/{os.environ.get('TORCHELASTIC_RESTART_COUNT', '0')}"
    history = []
    tmp = tempfile.mkdtemp(prefix=f"dusty_bench_r{rank}_")
    live = {"proc": None}

    def _reap(signum=None, frame=None):
        """the supervisor is going away (an exception in the poll loop, SIGTERM / SIGINT from the launcher's teardown): its
        measuring child runs in a session of its own and would otherwise survive holding the GPU"""
        if live["proc"] is not None and live["proc"].poll() is None:
            _kill_group(live["proc"])
        if signum is not None:
            sys.exit(128 + signum)
    import signal
    for sig in (signal.SIGTERM, signal.SIGINT):
        try:
            signal.signal(sig, _reap)
        except (ValueError, OSError):   # (not the main thread: tests)
            pass
    try:
        return _supervise_attempts(args, rank, world, stall, cap, first, child_cmd, store, pfx, history, tmp, live)
    finally:
        _reap()


def _supervise_attempts(args, rank, world, stall, cap, first, child_cmd, store, pfx, history, tmp, live):
    import socket
    import subprocess
    for a in range(first, len(ATTEMPTS)):
        name, extra = ATTEMPTS[a]
        key = f"{pfx}/a{a}"
        if rank == 0:
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                store.set(f"{key}/port", str(sk.getsockname()[1]))
        port = store.get(f"{key}/port").decode()
        env = dict(os.environ)
        env.update(extra)
        env.update({"DUSTY_BENCH_CHILD": "1", "DUSTY_BENCH_ATTEMPT": str(a), "MASTER_PORT": port,
                    "DUSTY_BENCH_PROGRESS": os.path.join(tmp, f"progress_a{a}")})
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # the child's process group meets on its OWN port with rank 0's child as the host (not the launcher's store, where
        # the keys of a failed attempt would still lie)
        for k in ("TORCHELASTIC_USE_AGENT_STORE",):
            env.pop(k, None)
        out_path = os.path.join(tmp, f"stdout_a{a}")
        cmd = child_cmd.split() if child_cmd else [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]
        t0 = time.time()
        with open(out_path, "w") as fout:
            proc = subprocess.Popen(cmd, env=env, stdout=fout, start_new_session=True)
        live["proc"] = proc
        outcome, last_size, last_change = None, -1, t0
        while outcome is None:
            time.sleep(0.25)
            rc = proc.poll()
            now = time.time()
            if rc is not None:
                outcome = "ok" if rc == 0 else f"child exited {rc}"
                break
            if store.check([f"{key}/fail"]):
                outcome = "failed on another rank: " + store.get(f"{key}/fail").decode()
                break
            try:
                size = os.path.getsize(env["DUSTY_BENCH_PROGRESS"])
            except OSError:
                size = 0
            if size != last_size:
                last_size, last_change = size, now
            if now - last_change > stall:
                outcome = f"no progress for {stall:.0f} s (rank {rank})"
            elif now - t0 > cap:
                outcome = f"exceeded {cap:.0f} s (rank {rank})"
        if outcome != "ok":
            if not store.check([f"{key}/fail"]):
                store.set(f"{key}/fail", outcome)
            _kill_group(proc)
        else:
            store.set(f"{key}/done/{rank}", "ok")
            # everyone's child must have finished: a rank whose child is still stuck fails the attempt for all
            t1 = time.time()
            keys = [f"{key}/done/{r}" for r in range(world)]
            while not store.check(keys):
                if store.check([f"{key}/fail"]):
                    outcome = "failed on another rank: " + store.get(f"{key}/fail").decode()
                    break
                if time.time() - t1 > stall:
                    outcome = "the other ranks did not finish"
                    store.set(f"{key}/fail", outcome)
                    break
                time.sleep(0.25)
        history.append({"attempt": a, "mode": name, "outcome": outcome, "seconds": round(time.time() - t0, 1)})
        if outcome == "ok":
            # Every rank says that it has SEEN the attempt succeed, and rank 0 - whose process may host the store when no
            # launcher does - leaves only when all have (bounded): returning at once took the store away under a peer's last
            # poll about once in thirty runs of tests/test_bench_supervisor.py ("Failed to recv ... Connection was likely
            # closed" -> that supervisor exited 1 behind a good record).  After its `seen` a rank makes no store call.
            try:
                store.set(f"{key}/seen/{rank}", "1")
            except Exception:  # noqa: BLE001  (the record is rank 0's business; nothing left to coordinate)
                pass
            if rank == 0:
                line = None
                with open(out_path) as fh:
                    for ln in fh:
                        if ln.startswith("{"):
                            line = ln
                if line is None:
                    print("bench.py supervisor: the child printed no JSON line", file=sys.stderr)
                    return 1
                rec = json.loads(line)
                rec.setdefault("distributed", {})["launch_attempts"] = history
                print(json.dumps(rec), flush=True)
                t2, seen = time.time(), [f"{key}/seen/{r}" for r in range(world)]
                try:
                    while not store.check(seen) and time.time() - t2 < 10.0:
                        time.sleep(0.05)
                except Exception:  # noqa: BLE001
                    pass
            return 0
        print(f"bench.py supervisor (rank {rank}): attempt {a} [{name}] failed: {outcome}", file=sys.stderr, flush=True)
    return 1


def self_launch(args):
    """`python bench.py --gpus N` with N > 1 and no rendezvous in the environment: start the N ranks ourselves (the
    reference's train.py:185-186 does mp.spawn(main_worker, nprocs=ngpus)) and relay rank 0's JSON line.  Runs before
    anything touches the GPU; the children are ordinary `torch.distributed.run` workers of this same file."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    # every worker is a supervisor (above) with its own per-attempt budget; this is the belt over those braces
    budget = len(ATTEMPTS) * float(os.environ.get("DUSTY_BENCH_CAP_S", "600")) + 300
    proc = subprocess.Popen(cmd, env=env, start_new_session=True)
    try:
        return proc.wait(timeout=budget)
    except subprocess.TimeoutExpired:
        print(f"bench.py: the launcher did not finish within {budget:.0f} s; killing its process group", file=sys.stderr)
        import signal
        try:   # SIGTERM first: every supervisor's handler kills its measuring child's own session before it goes
            os.killpg(proc.pid, signal.SIGTERM)
            proc.wait(timeout=20)
        except Exception:  # noqa: BLE001
            pass
        _kill_group(proc)
        return 1


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and os.environ.get("DUSTY_BENCH_CHILD") != "1" \
            and os.environ.get("DUSTY_BENCH_SUPERVISE", "1") != "0":
        sys.exit(supervise(args))     # (before anything touches the GPU)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    backend = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # one node: the ranks find each other on the loopback interface (a hostname that resolves to an unreachable
        # address otherwise stalls the bootstrap of gloo / RCCL until their timeouts); the data path is xGMI, not sockets
        os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
        os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
        # one rank per GPU over RCCL ("nccl" on ROCm).  DUSTY_BENCH_BACKEND=gloo lets the N > 1 code path be exercised on
        # a single-GPU box (ranks share the device, buffers travel through the host) - a functional check, not a number.
        backend = os.environ.get("DUSTY_BENCH_BACKEND", "nccl")
        ndev = torch.cuda.device_count()
        if backend == "nccl" and ndev < world:
            raise SystemExit(f"bench.py --gpus {world}: this node has {ndev} GPU(s); RCCL needs one device per rank "
                             "(DUSTY_BENCH_BACKEND=gloo runs the ranks on shared devices as a functional check)")
        local_rank = local_rank % max(ndev, 1)
        torch.cuda.set_device(local_rank)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    elif os.environ.get("DUSTY_GAN_FORCE_SEG", "0") == "1" and os.environ.get("DUSTY_BENCH_BACKEND") == "nccl":
        # one rank, the multi-rank schedule, every exchange through RCCL (identity collectives): what the call pattern
        # itself costs on one GPU, with no wire time (utils/dist.py through_backend)
        import socket
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                                device_id=torch.device("cuda", 0))
    if args.gpus != world and rank == 0:
        print(f"note: --gpus {args.gpus} but WORLD_SIZE={world}; using WORLD_SIZE", file=sys.stderr)
    progress("process group up")
    tr, arch = make_trainer(args, rank, local_rank, world)
    progress("trainer constructed")

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # Everything the timed region needs from the host is made BEFORE the warm-up: the per-step HIP events (one after every
    # step on the launch stream - the replayed graph / the eager launches of a step run on torch's current stream, so
    # consecutive events bracket exactly one step) and the garbage collection (no collector pass inside the timed region: one
    # run showed a single 12.6 ms step among 2.9 ms ones, a host-side stall).  Round 6: with the collection (50-100 ms of host
    # time) BETWEEN warm-up and timed region the GPU sat idle long enough to drop its clocks, and the first ~15 timed steps
    # ran 3-15 % above the steady state whatever the warm-up length (profiles/r06_timed_region_ramp.txt) - 2 % of a 20-step
    # window.  Now the warm-up's last replay has barely finished when the bracket's synchronize returns - and the warm-up's
    # capture step no longer collects either (with the collector already off the trainer's capture guard has nothing to do:
    # that collection was 66 of the capture step's 76 ms, two replays in front of the driver's 20-step window).
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    import gc
    gc.collect()
    gc.disable()
    last = None
    for i in range(args.warmup):
        last = tr.step(i)
        if world > 1:
            torch.cuda.synchronize()   # (a hang shows up at the step that hangs, not at the end of the warm-up)
            progress(f"warm-up step {i}: {tr.launch_mode()}")
    if last is not None:
        _ = list(last.values())
    progress("timed region")
    sync()
    t0 = time.perf_counter()
    marks[0].record()
    prev = None
    for i in range(args.steps):
        cur = tr.step(i)
        marks[i + 1].record()
        if prev is not None:
            _ = list(prev.values())  # read the previous step's scalars back while this step runs (one-step delay)
        prev = cur
    scal = dict(prev.items())
    sync()
    dt = time.perf_counter() - t0
    gc.enable()
    progress("timed region done")
    if world > 1:
        t = torch.tensor([dt], device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(tr, scal, args.dump_outputs)
    ms = 1e3 * dt / args.steps
    steps_s = args.steps / dt
    imgs = steps_s * args.batch * world
    per = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
    q = lambda f: round(per[min(len(per) - 1, int(f * len(per)))], 4)

    out = {"metric": "G+D train images/sec on 64x1024 LiDAR (steps/sec beside it)", "value": round(imgs, 2),
           "unit": "images/s", "steps_per_sec": round(steps_s, 3), "n_gpus": world, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": args.precision, "data": "synthetic",
           "config": {"workload": f"{'dcgan_eqlr baseline' if arch == 'none' else arch + '_dcgan_eqlr'}, "
                                  f"{args.shape[0]}x{args.shape[1]}, batch {args.batch}/GPU x {world}, "
                                  f"R1 {'on' if args.gp > 0 else 'off'}, {'path-length reg on, ' if args.pl > 0 else ''}DiffAugment {'off' if args.no_augment else 'on'}, "
                                  "Adam+EMA, random-init weights",
                      "global_batch": args.batch * world, "parallelism": f"dp{world}"},
           "step_ms_device": {"p10": q(0.10), "p50": q(0.50), "p90": q(0.90), "min": round(per[0], 4),
                              "max": round(per[-1], 4), "first_steps": [round(marks[i].elapsed_time(marks[i + 1]), 4)
                                              for i in range(min(int(os.environ.get("DUSTY_BENCH_FIRST_STEPS", "5")), args.steps))],
                              "note": "HIP events between consecutive steps, rank 0"},
           "launch_mode": tr.launch_mode(),
           "scalars_last_step": {k: round(v, 5) for k, v in scal.items()}}
    if dist.is_initialized():
        out["distributed"] = {"backend": backend or dist.get_backend(), "world_size": dist.get_world_size(),
                              "devices_visible": torch.cuda.device_count()}
        out["distributed"]["attempt"] = (ATTEMPTS[int(os.environ["DUSTY_BENCH_ATTEMPT"])][0]
                                         if "DUSTY_BENCH_ATTEMPT" in os.environ else "unsupervised")
        try:   # every rank's device identity, gathered: the record itself shows N distinct GPUs (or says that they are shared)
            pr = torch.cuda.get_device_properties(torch.cuda.current_device())
            ident = f"{getattr(pr, 'pci_domain_id', 0):04x}:{getattr(pr, 'pci_bus_id', 0):02x}:{getattr(pr, 'pci_device_id', 0):02x} " \
                    f"uuid={getattr(pr, 'uuid', '?')} {pr.name}"
            idents = [None] * dist.get_world_size()
            dist.all_gather_object(idents, ident)
            out["distributed"]["devices"] = idents
            out["distributed"]["distinct_devices"] = len(set(idents))
        except Exception as e:  # noqa: BLE001
            out["distributed"]["devices"] = f"not gathered ({type(e).__name__}: {e})"
        out["distributed"]["exchanges_per_step"] = 4  # D.hi, D.lo, G.gather (one coalesced pair), G.tail (+ the async scalars)
        try:
            out["distributed"]["bytes_per_step"] = tr.comm_bytes()
        except Exception as e:  # noqa: BLE001
            out["distributed"]["bytes_per_step"] = f"not computed ({type(e).__name__}: {e})"
        try:  # (instrumentation after the timed region: never at the price of the line itself)
            comm = tr.comm_profile(steps=3)
            if comm:
                out["distributed"]["exposed_ms_per_step"] = comm
            elif getattr(tr, "_comm_captured", False):
                out["distributed"]["exposed_ms_per_step"] = ("collectives and their waits are nodes of the step's hipGraph "
                                                             "(no host-side call to time); DUSTY_GAN_GRAPH_COMM=0 measures the segmented form")
        except Exception as e:  # noqa: BLE001
            out["distributed"]["exposed_ms_per_step"] = f"not measured ({type(e).__name__}: {e})"
    if args.soak_steps > 0:
        try:
            progress("soak")
            # (ranks sharing a device over gloo - a functional check, every exchange through the host - take ~0.1 s per step)
            out["soak"] = soak(tr, args.soak_steps if (world == 1 or backend == "nccl") else min(args.soak_steps, 40))
            out["soak"]["vs_timed_region"] = round(out["soak"]["ms_per_step_wall"] / ms, 4)
            progress("soak done")
        except Exception as e:  # noqa: BLE001  (instrumentation behind the timed region: never at the price of the line)
            out["soak"] = {"error": f"{type(e).__name__}: {e}"}
    fl, f_g, f_d = flops_per_sample(args.shape, arch, args.gp)
    out["step_flops_fraction_of_mfma_peak"] = round(fl * args.batch * steps_s / 1e12 / PEAK_TFLOPS[args.precision], 4)

    if not args.no_roofline:
        try:
            fam = roofline_pass(tr)
        except Exception as e:  # noqa: BLE001
            fam = None
            out["roofline"] = {"error": f"{type(e).__name__}: {e}"}
        if rank == 0 and fam:
            name = max(fam, key=lambda k: fam[k]["ms"])
            f = fam[name]
            tf = f["flops"] / (f["ms"] * 1e-3) / 1e12
            traffic, src = pmc_traffic(name, args, arch)
            out["roofline"] = {"kernel": name, "bound": "mfma", "achieved": round(tf, 2),
                               "peak": PEAK_TFLOPS[args.precision], "unit": "TFLOP/s",
                               "frac": round(tf / PEAK_TFLOPS[args.precision], 4), "traffic": traffic,
                               "traffic_unit": "HBM-side bytes per launch (rocprofv3 PMC FETCH_SIZE x2 + WRITE_SIZE)",
                               "traffic_source": src, "kernel_source_sha": kernel_source_sha(),
                               "algorithmic_bytes_per_launch": round(f["bytes"] / f["n"]),
                               "launches": f["n"], "avg_launch_us": round(1e3 * f["ms"] / f["n"], 2),
                               "timing": f"HIP events around every launch of {f['steps']} eager steps behind the timed region, "
                                         "per-launch median, summed per step"}
            if traffic:
                out["roofline"]["traffic_over_algorithmic"] = round(traffic / (f["bytes"] / f["n"]), 3)
            if not args.no_clock and args.precision == "bf16" and name == "conv_mfma_kernel":
                # what the peak is at the clock this chip holds inside this kernel (the 2.5 PFLOP/s of `peak` is 2.4 GHz)
                ghz, info = held_clock()
                out["roofline"]["clock_ghz"] = ghz
                out["roofline"]["clock_source"] = info
                if ghz:
                    out["roofline"]["peak_at_held_clock"] = round(PEAK_TFLOPS[args.precision] * ghz / PEAK_CLOCK_GHZ, 1)
                    out["roofline"]["frac_at_held_clock"] = round(tf / (PEAK_TFLOPS[args.precision] * ghz / PEAK_CLOCK_GHZ), 4)
            out["kernel_families"] = {
                k: {"ms_per_step": round(v["ms"], 3), "launches_per_step": v["n"],
                    "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2),
                    "algorithmic_GBps": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1)} for k, v in fam.items()}
            # the model checks itself: no family can run above either roof on its ALGORITHMIC work - if one does, the
            # FLOP / byte model of engine.conv_algorithmic / wgrad_algorithmic is wrong, not the hardware fast
            bad = [f"{k}: {v['tflops']} TFLOP/s > {PEAK_TFLOPS[args.precision]}" for k, v in out["kernel_families"].items()
                   if v["tflops"] > PEAK_TFLOPS[args.precision]]
            bad += [f"{k}: {v['algorithmic_GBps']} GB/s > {PEAK_HBM_GBS}" for k, v in out["kernel_families"].items()
                    if v["algorithmic_GBps"] > PEAK_HBM_GBS]
            out["roofline"]["model_self_check"] = "ok" if not bad else bad
            if bad:
                print("bench.py: algorithmic work model violates a roof: " + "; ".join(bad), file=sys.stderr)
    if rank == 0:
        # whole-step roofline: max(T_flop, T_bytes) / measured step time, per GPU
        es = 2 if args.precision == "bf16" else 4
        sf, sb = step_model(args.shape, arch, args.gp, args.batch, es, tr.optim_G.store.n, tr.optim_D.store.n)
        t_flop, t_bytes = sf / (PEAK_TFLOPS[args.precision] * 1e12) * 1e3, sb / (PEAK_HBM_GBS * 1e9) * 1e3
        step = {"t_flop_ms": round(t_flop, 4), "t_bytes_ms": round(t_bytes, 4), "flops": sf, "bytes": round(sb),
                "bound": "hbm" if t_bytes > t_flop else "mfma", "frac": round(max(t_flop, t_bytes) / ms, 4),
                "note": "per GPU: executed conv FLOPs / MFMA peak vs minimal parameter + activation bytes / 8 TB/s "
                        "(bench.py step_model), over the measured ms_per_step"}
        meas = pmc_step_traffic(args, arch)
        step["measured_bytes"] = meas["bytes"] if meas else None
        if meas:
            step["measured"] = meas
            step["measured_over_model"] = round(meas["bytes"] / sb, 3)
        out.setdefault("roofline", {})["step"] = step
        # the gradient tolerances of the timed mode are its own (tests/test_gpu_configs.py), not north_star's 1e-3
        out["parity_of_this_mode"] = (
            "bf16 storage, fp32 accumulate.  Anchored to the REFERENCE: at full width the reference's own modules under "
            "torch.autocast(cpu, bfloat16) are 4e-4..7e-3 (outputs) and 7e-2..1.5e-1 (every gradient tensor) from their fp32 "
            "results (tests/golden/full_dusty2_autocast.npz); this mode's step is held to <= 1.5 x that distance per tensor "
            "(tests/test_gpu_configs.py::test_timed_mode_within_the_reference_autocast_yardstick; measured 0.7-1.4 x), and to D "
            "gradients <= 2.1e-2 / G <= 6.6e-2 against the bf16-emulating oracle at batch 32.  The <= 1e-3 north-star tolerance "
            "is met by --precision fp32 (gradients <= 5e-3, cosine >= 0.99999 against the reference digests); two runs from one "
            "seed are bit-identical (tests/test_gpu_timed_path.py)"
            if args.precision == "bf16" else
            ("fp32x3: fp32 parameters and accumulation, the fat layers' feature maps and weight shadows stored as split-bf16 pairs "
             "(hi + lo, 16 mantissa bits; DG_BF16X2) and contracted as three bf16 products on the timed path's own kernels: held to "
             "the fp32 mode's bounds against the reference digests at full width (tests/test_gpu_configs.py, tests/test_gpu_x2.py)"
             if args.precision == "fp32x3" else "fp32 parity mode: <= 1e-3 against the oracle / reference fixtures"))
    if (rank == 0 and world == 1 and not args.no_other_configs and args.arch is None and args.shape == [64, 1024]
            and args.batch == 32 and args.precision == "bf16" and args.pl == 0.0 and args.gp == 1.0 and not args.no_augment):
        del tr
        import gc
        gc.collect()
        torch.cuda.empty_cache()
        # the headline record is safe before anything is appended to it: on stderr and in gpurun_out/ (the ONE JSON line
        # of the contract is printed once, at the end, with the appended entries)
        print("bench.py headline record (extended line follows on stdout): " + json.dumps(out), file=sys.stderr, flush=True)
        try:
            os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
            with open(os.path.join(ROOT, "gpurun_out", "bench_headline_last.json"), "w") as fh:
                json.dump(out, fh)
        except OSError:
            pass
        out["other_configs"] = other_config_lines(args)
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:
            out["cpu_baseline"] = cpu_baseline(args, arch)
        except Exception as e:  # noqa: BLE001
            out["cpu_baseline"] = {"error": f"{type(e).__name__}: {e}"}
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
