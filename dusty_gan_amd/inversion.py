"""GAN inversion: reconstruct LiDAR scans by optimising the latent code of a trained generator -- reference:
evaluate_reconstruction.py:32-164 (the loop) with utils/__init__.py:224-246 (SphericalOptimizer, masked_loss).

Every step is forward (eval mode) -> dg_inv_loss_grad -> the generator's backward-data chain -> grad_z ->
dg_sphere_adam (GEngine.inversion_step).  The reference's demo adds a third loss, "chamfer" (demo.py:508-519): the symmetric
Chamfer distance between the target's points and postprocess(out)["points"], the one term whose gradient reaches the
measurability head - dg_inv_to_xyz -> two dg_chamfer_nn searches -> dg_inv_chamfer_scatter -> dg_inv_chamfer_grad.  The step index, the Adam moments and the latent live on the device, so one
step is captured in a hipGraph and replayed; the scalars are read back once, after the loop."""
import gc
import math

import torch

from . import _lib as L
from . import engine as E

# Philox stream ids of the inversion's own draws (the model's and the trainer's generators use 0-9)
STREAM_LATENT, STREAM_PERTURB, STREAM_GUMBEL = 11, 12, 13


def lr_schedule(k, num_step, lr_rampup_ratio=0.05, lr_rampdown_ratio=0.25):
    """LambdaLR factor of step k (evaluate_reconstruction.py:72-77, stylegan2's schedule); step 0 gives 0"""
    t = k / num_step
    gamma = min(1.0, (1.0 - t) / lr_rampdown_ratio)
    gamma = 0.5 - 0.5 * math.cos(gamma * math.pi)
    return gamma * min(1.0, t / lr_rampup_ratio)


def noise_strength(k, num_step, noise_ratio=0.75, noise_sigma=1.0):
    """strength of step k's latent perturbation (evaluate_reconstruction.py:100-104)"""
    w = max(0.0, 1.0 - (k / num_step) / noise_ratio)
    return 0.05 * noise_sigma * w ** 2


def normalize_rows(latent):
    """latent.div_(latent.pow(2).mean(dim=1, keepdim=True).add(1e-9).sqrt()) (evaluate_reconstruction.py:89)"""
    return latent.div_(latent.pow(2).mean(dim=1, keepdim=True).add(1e-9).sqrt())


def _draw_normal(seed, stream_id, n, device):
    """n standard normals of Philox (seed, stream_id) from counter 0 (dg_philox_fill kind 1).  No device counter: a
    utils.rng.Philox would queue its advance with whatever trainer's counter queue is current."""
    out = torch.empty(n, dtype=torch.float32, device=device)
    L.check(L.lib().dg_philox_fill(seed, stream_id, 0, 1, 0.0, 1.0, 0, 1, n, L.ptr(out), L.stream_ptr()), "dg_philox_fill")
    return out


def _draw_logistic(seed, stream_id, n, eps, device):
    """GumbelSigmoid.logistic_noise from Philox (seed, stream_id): U1, U2 uniform fills at counters 0 and (n + 3) / 4, then
    dg_logistic_noise - the numbers utils.rng.Philox.logistic_noise draws at offset 0"""
    u = torch.empty(2, n, dtype=torch.float32, device=device)
    out = torch.empty(n, dtype=torch.float32, device=device)
    lib = L.lib()
    for i in range(2):
        L.check(lib.dg_philox_fill(seed, stream_id, i * ((n + 3) // 4), 0, 0.0, 1.0, 0, 1, n, L.ptr(u[i]), L.stream_ptr()),
                "dg_philox_fill")
    L.check(lib.dg_logistic_noise(L.ptr(u[0]), L.ptr(u[1]), eps, n, L.ptr(out), L.stream_ptr()), "dg_logistic_noise")
    return out


DISTANCES = ("l1", "l2", "chamfer")   # the order the terms are evaluated and summed in


def check_distance(distance, lidar=None):
    """`distance` of invert - one of DISTANCES or a sequence of them (demo.py:509-519: the loss is their sum) - as a tuple
    in DISTANCES' order.  ValueError for an empty selection or "chamfer" without a LiDAR; needs no device."""
    names = (distance,) if isinstance(distance, str) else tuple(distance)
    if len(names) == 0:
        raise ValueError("no distance selected: give at least one of " + ", ".join(DISTANCES))
    for n in names:
        if n not in DISTANCES:
            raise NotImplementedError(n)
    if "chamfer" in names:
        if lidar is None:
            raise ValueError('distance "chamfer" needs lidar= (dusty_gan_amd.utils.lidar.LiDAR with its angle grid)')
        if getattr(lidar, "angle", None) is None:
            raise ValueError('distance "chamfer" needs a LiDAR with an angle grid (angles.pt or use_nominal_angles)')
        if float(lidar.drop_const) != 0.0:
            raise ValueError("the Chamfer term is built for the LiDAR's own drop_const of 0 (utils/lidar.py:12)")
    return tuple(n for n in DISTANCES if n in names)


class ChamferState:
    """The Chamfer term's buffers: the target's points R (made once), the generated points, both searches' results and the
    scatter words (zero at rest)."""

    def __init__(self, inv_ref, lidar, tol):
        dev = inv_ref.device
        B, _, H, W = inv_ref.shape
        HW = H * W
        if HW > (1 << 18):
            raise ValueError("the Chamfer term holds at most 2^18 points per scan")
        assert (H, W) == (lidar.H, lidar.W)
        self.tol = float(tol)
        self.min_depth, self.max_depth = lidar.min_depth, lidar.max_depth
        self.angle = lidar.angle.detach().to(dev).float().reshape(2, HW).contiguous()   # (a copy: the caller's LiDAR stays as it is)
        self.R = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
        ref = inv_ref.detach().float().contiguous()
        L.check(L.lib().dg_inv_to_xyz(L.ptr(ref), L.ptr(self.angle), B, H, W, 0, self.min_depth, self.max_depth, 0.0, self.tol,
                                      None, L.ptr(self.R), L.stream_ptr()), "dg_inv_to_xyz")
        self.P = torch.empty_like(self.R)
        self.d1 = torch.empty(B, HW, dtype=torch.float32, device=dev)
        self.d2 = torch.empty_like(self.d1)
        self.idx1 = torch.empty(B, HW, dtype=torch.int32, device=dev)
        self.idx2 = torch.empty_like(self.idx1)
        self.acc = torch.zeros(B, HW, 4, dtype=torch.int64, device=dev)


def _backbone(G):
    return G.backbone if hasattr(G, "backbone") else G


def _fixed_gumbel(G, B, H, W, seed, device, gumbel_noise):
    """the pixel-level logistic noise of G in eval mode with fix_noise (utils/__init__.py:141-149): the noise G already holds
    fixed, else `gumbel_noise` [1,1,H,W], else one draw of the inversion's own Philox stream (G's generators are not advanced)"""
    bb = _backbone(G)
    if bb.masker == "none":
        return None
    gs = G.gumbel_pixel if bb.masker == "dusty2" else G.gumbel
    noise = gumbel_noise if gumbel_noise is not None else gs.fixed_noise
    if noise is None:
        noise = _draw_logistic(int(seed) & (2**64 - 1), STREAM_GUMBEL, H * W, gs.eps, device).view(1, 1, H, W)
    return {"pixel": noise.to(device).float().expand(B, 1, H, W).contiguous()}


class InvState:
    """Everything one inversion's steps read and write, allocated before the loop."""

    NCHUNK = 16   # workgroups per sample of dg_inv_loss_grad

    def __init__(self, inv_ref, mask_ref, latent, gumbel, *, num_step, distance, lr, perturb_latent, noise_ratio,
                 noise_sigma, lr_rampup_ratio, lr_rampdown_ratio, seed, lidar=None, tol=1e-8):
        dev = inv_ref.device
        B, _, H, W = inv_ref.shape
        self.B, self.HW = B, H * W
        self.ref = inv_ref.detach().float().contiguous()
        self.mask = mask_ref.detach().float().contiguous()
        self.msum = self.mask.sum(dim=(1, 2, 3)).contiguous()   # integers: exact in any order
        names = check_distance(distance, lidar)
        self.terms = tuple({"l1": 0, "l2": 1}[n] for n in names if n != "chamfer")   # dg_inv_loss_grad's distance codes
        self.chamfer = ChamferState(inv_ref, lidar, tol) if "chamfer" in names else None
        self.latent = latent
        self.m = torch.zeros_like(latent)
        self.v = torch.zeros_like(latent)
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.nchunk = max(1, min(self.NCHUNK, self.HW // 1024))
        self.parts = torch.zeros(B * self.nchunk, dtype=torch.float32, device=dev)
        self.tickets = torch.zeros(B, dtype=torch.int32, device=dev)
        self.loss = torch.zeros(B, dtype=torch.float32, device=dev)
        self.noise_in = None
        self.gumbel = gumbel
        b1, b2 = 0.9, 0.999   # torch.optim.Adam's defaults
        # the per-step scalars formed the way torch's Adam forms them: LambdaLR's lr a Python float, the step count a float32
        # tensor, so the bias corrections and the step size are float32 tensor arithmetic
        rows = []
        for k in range(num_step + 1):
            t = torch.tensor(float(k + 1))
            step_lr = float(lr) * lr_schedule(k, num_step, lr_rampup_ratio, lr_rampdown_ratio)
            rows.append(torch.stack([step_lr / (1 - b1 ** t), (1 - b2 ** t).sqrt(),
                                     torch.tensor(noise_strength(k, num_step, noise_ratio, noise_sigma))]))
        self.sched = torch.stack(rows).float().contiguous().to(dev)
        self.hp = (int(num_step), b1, b2, 1e-8, int(bool(perturb_latent)), int(seed) & (2**64 - 1), STREAM_PERTURB)

    def optimizer_launch(self, dzT, zT, z_dtype, prime=False):
        """dg_sphere_adam on the gradient dz^T [nz][Bp] (prime: only the first step's generator input into zT)"""
        B, nz = self.latent.shape
        Bp = dzT.shape[1] if dzT is not None else 0
        ns, b1, b2, eps, pert, seed, sid = self.hp
        L.check(L.lib().dg_sphere_adam(L.ptr(dzT), 1, Bp, L.ptr(self.latent), L.ptr(self.m), L.ptr(self.v), L.ptr(self.step),
                                       L.ptr(self.ticket), L.ptr(self.noise_in), L.ptr(zT), z_dtype, B, nz, L.ptr(self.sched),
                                       ns, b1, b2, eps, pert, seed, sid, int(prime), L.stream_ptr()), "dg_sphere_adam")


def invert(G, inv_ref, mask_ref, *, num_step=1000, distance="l1", lr=0.1, perturb_latent=True, noise_ratio=0.75,
           noise_sigma=1.0, lr_rampup_ratio=0.05, lr_rampdown_ratio=0.25, seed=0, latent=None, graph=True,
           noise_fn=None, gumbel_noise=None, on_step=None, lidar=None, tol=1e-8):
    """Reconstruct inv_ref [B,1,H,W] (inverse depth in [0,1]) under mask_ref [B,1,H,W] by optimising G's latent
    (evaluate_reconstruction.py:84-118).  G: what utils.setup returns (the bare 'none' generator or a DUSty1 / DUSty2
    wrapper), run in eval mode at its own precision; nothing of G is modified.
    distance: "l1", "l2", "chamfer" or a sequence of them; the per-sample loss is their sum (demo.py:509-519).  "chamfer"
    needs lidar= (utils.lidar.LiDAR with its angle grid) and takes tol, postprocess's validity threshold.
    latent: the initial latent [B,nz] (default: Philox normal draws of `seed`, rows normalised as the reference does).
    Test hooks: noise_fn(k) -> the perturbation [B,nz] added to the latent at step k (replaces the Philox draws; eager
    loop), gumbel_noise [1,1,H,W] the fixed pixel-level logistic noise of the dusty archs, on_step(k, loss [B],
    d loss / d latent [B,nz], latent [B,nz]) after every step (eager loop).
    graph: capture one step (after two eager ones) and replay it; results equal the eager loop's bit for bit.
    Returns {"latent", "out", "inv_gen", "loss"}: the reference's loop variables after the loop - the optimised latent, the
    last step's generator output and tanh_to_sigmoid of its unmasked depth, and the last step's per-sample loss."""
    from .utils.lidar import unit_map
    check_distance(distance, lidar)
    bb = _backbone(G)
    if not inv_ref.is_cuda:
        raise RuntimeError("invert runs on the GPU only (no CPU fallback)")
    if num_step < 1:
        raise ValueError("num_step must be >= 1")
    dev = inv_ref.device
    B, _, H, W = inv_ref.shape
    assert (H, W) == tuple(bb.shape) and inv_ref.shape == mask_ref.shape
    if hasattr(G, "_sync"):
        G._sync()   # the wrapper's tau / drop_const onto the backbone
    eng, st = bb.engine(), bb.store
    if latent is None:
        latent = _draw_normal(int(seed) & (2**64 - 1), STREAM_LATENT, B * bb.in_ch, dev).view(B, bb.in_ch)
        normalize_rows(latent)
    latent = latent.detach().to(dev).float().clone().contiguous()
    S = InvState(inv_ref, mask_ref, latent, _fixed_gumbel(G, B, H, W, seed, dev, gumbel_noise), num_step=num_step,
                 distance=distance, lr=lr, perturb_latent=perturb_latent, noise_ratio=noise_ratio, noise_sigma=noise_sigma,
                 lr_rampup_ratio=lr_rampup_ratio, lr_rampdown_ratio=lr_rampdown_ratio, seed=seed,
                 lidar=lidar, tol=tol)
    # every buffer of the loop exists before it, allocated on the caller's stream
    eng.alloc(B, dev)
    eng.grad_z_buffers()
    zdt = L.dtype_code(eng.dtype)
    zero = torch.zeros_like(latent)

    def injected(k):
        if not perturb_latent:
            return zero
        return noise_fn(k).to(dev).float().contiguous() if k < num_step else zero

    if noise_fn is not None or on_step is not None:
        graph = False
    # The loop runs on a stream of its own: its split-K weight-gradient workspace (engine.WGRAD_WS is per stream) and its
    # capture are then its own, never the caller's or a trainer's (torch's default capture stream is shared by every
    # torch.cuda.graph without a stream); the workspace is released once the replays have run.
    caller = torch.cuda.current_stream(dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(caller)
    g = None
    try:
        with torch.cuda.stream(s):
            if noise_fn is not None:
                S.noise_in = injected(0)
            S.optimizer_launch(None, eng.zT, zdt, prime=True)
            out = None
            n_eager = min(num_step, 2) if graph else num_step
            for k in range(n_eager):
                if noise_fn is not None:
                    S.noise_in = injected(k + 1)
                out = eng.inversion_step(st, S)
                if on_step is not None:
                    on_step(k, S.loss.clone(), eng._dzw[:, :B].t().clone(), S.latent.clone())
            if num_step > n_eager:
                g = torch.cuda.CUDAGraph()
                was = gc.isenabled()
                gc.disable()   # (no collection inside the capture)
                try:
                    with torch.cuda.graph(g, stream=s):
                        out = eng.inversion_step(st, S)
                finally:
                    if was:
                        gc.enable()
                for _ in range(num_step - n_eager):
                    g.replay()
        caller.wait_stream(s)
    finally:
        s.synchronize()    # (the one host sync: the graph and the stream's workspace go only after the replays have run)
        E.WGRAD_WS.drop_stream(s)
        del g
    res_out = {key: v.clone() for key, v in out.items()}
    depth = eng.gout[:, 0:1]
    return {"latent": S.latent.clone(), "out": res_out, "inv_gen": unit_map(depth, 0), "loss": S.loss.clone()}
