"""GAN inversion: reconstruct LiDAR scans by optimising the latent code of a trained generator -- reference:
evaluate_reconstruction.py:32-164 (the loop) with utils/__init__.py:224-246 (SphericalOptimizer, masked_loss).

Every step is forward (eval mode) -> dg_inv_loss_grad -> the generator's backward-data chain -> grad_z ->
dg_sphere_adam (GEngine.inversion_step).  The reference's demo adds a third loss, "chamfer" (demo.py:508-519): the symmetric
Chamfer distance between the target's points and postprocess(out)["points"], the one term whose gradient reaches the
measurability head - dg_inv_to_xyz -> two dg_chamfer_nn searches -> dg_inv_chamfer_scatter -> dg_inv_chamfer_grad.  A fourth,
"emd", is this project's: the earth mover's distance of the evaluation on K furthest-point-sampled rays of the target, the
second 3-D term - dg_inv_to_xyz -> dg_points_gather -> dg_emd_grad -> dg_inv_points_grad (EmdState).  The step index, the Adam moments and the latent live on the device, so one
step is captured in a hipGraph and replayed; the scalars are read back once, after the loop.

num_code > 1 is the demo's multi-code mode (mGANprior, demo.py:353-366, 466-488, 523-530): N latents per scan run through the
lower layers, their feature maps at one layer are blended per channel with learnable weights alpha (dg_feat_compose), and the
blend runs through the rest of G as one sample; the latents are stepped by the spherical Adam, alpha by a plain Adam
(dg_alpha_adam).  GEngine._inversion_step_multi, DESIGN.md 7b."""
import gc
import math

import torch

from . import _lib as L
from . import engine as E

# Philox stream ids of the inversion's own draws (the model's and the trainer's generators use 0-9); 14 is the target
# corruptions' (corruption.STREAM_CORRUPT), 15 the ray-drop transfer's (raydrop.STREAM_RAYDROP), 16 the gates of DiffAugment with
# p < 1 (DG_STREAM_AUG_GATE, include/dusty_gan_hip.h: the low word of the gate block's stream, the augmenter's own id the high one)
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


def _draw_normal(seed, stream_id, n, device, offset=0):
    """n standard normals of Philox (seed, stream_id) from counter `offset` (dg_philox_fill kind 1).  No device counter: a
    utils.rng.Philox would queue its advance with whatever trainer's counter queue is current."""
    out = torch.empty(n, dtype=torch.float32, device=device)
    L.check(L.lib().dg_philox_fill(seed, stream_id, int(offset), 1, 0.0, 1.0, 0, 1, n, L.ptr(out), L.stream_ptr()), "dg_philox_fill")
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


DISTANCES = ("l1", "l2", "chamfer", "emd")   # the order the terms are evaluated and summed in
POINT_TERMS = ("chamfer", "emd")             # the 3-D terms: they need the LiDAR's angle grid
EMD_MAX_POINTS = 3200                        # dg_emd_grad holds n + m <= 6400 points per pair


def check_distance(distance, lidar=None):
    """`distance` of invert - one of DISTANCES or a sequence of them (demo.py:509-519: the loss is their sum) - as a tuple
    in DISTANCES' order.  ValueError for an empty selection or a 3-D term ("chamfer", "emd") without a LiDAR; needs no device."""
    names = (distance,) if isinstance(distance, str) else tuple(distance)
    if len(names) == 0:
        raise ValueError("no distance selected: give at least one of " + ", ".join(DISTANCES))
    for n in names:
        if n not in DISTANCES:
            raise NotImplementedError(n)
    for n in POINT_TERMS:
        if n not in names:
            continue
        if lidar is None:
            raise ValueError(f'distance "{n}" needs lidar= (dusty_gan_amd.utils.lidar.LiDAR with its angle grid)')
        if getattr(lidar, "angle", None) is None:
            raise ValueError(f'distance "{n}" needs a LiDAR with an angle grid (angles.pt or use_nominal_angles)')
        if float(lidar.drop_const) != 0.0:
            raise ValueError(f"the {n} term is built for the LiDAR's own drop_const of 0 (utils/lidar.py:12)")
    return tuple(n for n in DISTANCES if n in names)


def check_emd_points(emd_points, HW):
    """K of the earth mover's term: an integer in 1..min(EMD_MAX_POINTS, HW) (ValueError); needs no device"""
    K = int(emd_points)
    if K != emd_points or not 1 <= K <= min(EMD_MAX_POINTS, HW):
        raise ValueError(f"emd_points must be an integer in 1..min({EMD_MAX_POINTS}, H W = {HW}), got {emd_points!r}: "
                         f"dg_emd_grad holds at most {2 * EMD_MAX_POINTS} points per pair")
    return K


class PointMaps:
    """What the 3-D terms share: the angle grid, the target's point map R (made once) and the generated one P (every step)"""

    def __init__(self, inv_ref, lidar, tol):
        dev = inv_ref.device
        B, _, H, W = inv_ref.shape
        HW = H * W
        assert (H, W) == (lidar.H, lidar.W)
        self.tol = float(tol)
        self.min_depth, self.max_depth = lidar.min_depth, lidar.max_depth
        self.angle = lidar.angle.detach().to(dev).float().reshape(2, HW).contiguous()   # (a copy: the caller's LiDAR stays as it is)
        self.R = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
        ref = inv_ref.detach().float().contiguous()
        L.check(L.lib().dg_inv_to_xyz(L.ptr(ref), L.ptr(self.angle), B, H, W, 0, self.min_depth, self.max_depth, 0.0, self.tol,
                                      None, L.ptr(self.R), L.stream_ptr()), "dg_inv_to_xyz")
        self.P = torch.empty_like(self.R)


class ChamferState(PointMaps):
    """The Chamfer term's buffers: the target's points R (made once), the generated points, both searches' results and the
    scatter words (zero at rest)."""

    def __init__(self, inv_ref, lidar, tol):
        dev = inv_ref.device
        B, _, H, W = inv_ref.shape
        HW = H * W
        if HW > (1 << 18):   # csrc/common.h DG_FIX40_MAX_TERMS
            raise ValueError("the Chamfer term holds at most 2^18 points per scan")
        super().__init__(inv_ref, lidar, tol)
        self.d1 = torch.empty(B, HW, dtype=torch.float32, device=dev)
        self.d2 = torch.empty_like(self.d1)
        self.idx1 = torch.empty(B, HW, dtype=torch.int32, device=dev)
        self.idx2 = torch.empty_like(self.idx1)
        self.acc = torch.zeros(B, HW, 4, dtype=torch.int64, device=dev)


class EmdState:
    """The earth mover's term on K rays of the target: the sample T (dg_fps_map on the target's point map, drawn once), its
    inverse `slot` [B,HW] (-1: not a sample), the target's sampled cloud Rs, and per step the generated cloud on the same rays
    Ps, dg_emd_grad's cost, gradA (the point gradient) and gradB (scratch).  maps: the PointMaps whose R and P it reads.
    ValueError - after ONE host read, before any step - for a scan with fewer than K furthest-point candidates (pixels with
    |R|^2 >= 1e-3 in unit space: the reference's sampler never selects the others) or with a repeated index."""

    def __init__(self, maps, K):
        from .utils.sampling import _run_map
        self.maps = maps
        R = maps.R
        dev = R.device
        B, HW = R.shape[0], R.shape[2] * R.shape[3]
        self.K = K = check_emd_points(K, HW)
        self.idx, self.Rs = _run_map(R, K, True)
        self.slot = torch.full((B, HW), -1, dtype=torch.int32, device=dev)
        order = torch.arange(K, dtype=torch.int32, device=dev).expand(B, K)
        self.slot.scatter_(1, self.idx.long(), order)
        flat = R.flatten(2)
        mag = (flat[:, 0] * flat[:, 0]) + (flat[:, 1] * flat[:, 1]) + (flat[:, 2] * flat[:, 2])
        cand = (mag >= 1e-3).sum(dim=1)   # (float32(1e-3) itself is a candidate: csrc/point_fps.hip fps_skipped)
        distinct = (self.slot.gather(1, self.idx.long()) == order).all(dim=1)
        cand, distinct = torch.stack([cand, distinct.long()]).tolist()   # the one host read
        short = [b for b in range(B) if cand[b] < K]
        if short:
            raise ValueError(f"emd_points = {K}: scan(s) {short} of the batch have only {[cand[b] for b in short]} furthest-point "
                             "candidates (points at 1e-3 or more of squared unit range): lower emd_points")
        twice = [b for b in range(B) if not distinct[b]]
        if twice:
            raise ValueError(f"emd_points = {K}: the sample of scan(s) {twice} repeats a pixel")
        self.Ps = torch.empty_like(self.Rs)
        self.gradA = torch.empty_like(self.Rs)
        self.gradB = torch.empty_like(self.Rs)
        self.cost = torch.empty(B, dtype=torch.float32, device=dev)
        self.grad_cost = torch.full((B,), 1.0 / K, dtype=torch.float32, device=dev)


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


MAX_LOWER = 4096   # lower-batch samples (scans x codes) of one multi-code call
MAX_CODES = 64     # the demo's slider ends there (demo.py:353-357)


def composition_layers(G):
    """{name: (C, h, w)} of the feature maps a multi-code inversion can compose at - the counterpart of the reference's
    demo.get_feature_shapes, restricted to what is supported: the outputs of Proj, Up1, Up2 and Up3 under the reference's module
    names ("0".."3" for the bare generator, "backbone.0".."backbone.3" for the DUSty wrappers) and, as aliases of the same
    tensors, the last child of each block ("<blk>.1" for Proj, "<blk>.2" for Up)."""
    bb = _backbone(G)
    pre = "backbone." if bb is not G else ""
    h0, w0 = bb.shape[0] >> 4, bb.shape[1] >> 4
    out = {}
    for l in range(4):
        shape = (bb.chs[3 - l], h0 << l, w0 << l)
        out[f"{pre}{l}"] = shape
        out[f"{pre}{l}.{1 if l == 0 else 2}"] = shape
    return out


def parse_composition_layer(layer, wrapped=None):
    """the index 0..3 (a[l]: the output of Proj, Up1, Up2, Up3) of `layer`: that integer, or one of composition_layers' names.
    wrapped: True / False - the generator is a DUSty wrapper / the bare one, whose names carry / lack "backbone." (None: either
    form).  NotImplementedError for any other module of the generator (a Pad's output, a conv's pre-activation, the Head's
    inside); needs no device."""
    accepted = ('0..3, or the module names "0".."3" ("backbone.0".."backbone.3" for the DUSty wrappers) and their last children '
                '"<blk>.1" (Proj: blk 0) / "<blk>.2" (Up: blk 1..3)')
    if isinstance(layer, bool) or layer is None:
        raise ValueError(f"composition_layer: {accepted}")
    if isinstance(layer, int):
        if 0 <= layer <= 3:
            return layer
        raise NotImplementedError(f"composition_layer {layer}: accepted are {accepted}")
    name = str(layer)
    has = name.startswith("backbone.")
    body = name[len("backbone."):] if has else name
    parts = body.split(".")
    ok = not (has and wrapped is False)   # (the bare generator has no "backbone." modules)
    if ok and parts[0] in ("0", "1", "2", "3"):
        l = int(parts[0])
        if len(parts) == 1 or (len(parts) == 2 and parts[1] == ("1" if l == 0 else "2")):
            return l
    raise NotImplementedError(f"composition_layer {name!r}: accepted are {accepted}")


def check_multi_code(num_code, composition_layer, alpha, alpha_lr, B=None, wrapped=None):
    """the multi-code arguments of invert; returns the layer index, or None for num_code == 1.  Needs no device."""
    if int(num_code) != num_code or num_code < 1 or num_code > MAX_CODES:
        raise ValueError(f"num_code must be an integer in 1..{MAX_CODES}")
    if num_code == 1:
        if composition_layer is not None or alpha is not None or alpha_lr != 1e-3:
            raise ValueError("composition_layer, alpha and alpha_lr belong to num_code > 1: leave them at their defaults")
        return None
    if composition_layer is None:
        raise ValueError("num_code > 1 needs composition_layer (dusty_gan_amd.inversion.composition_layers lists them)")
    layer = parse_composition_layer(composition_layer, wrapped)
    if B is not None and B * num_code > MAX_LOWER:
        raise ValueError(f"{B} scans x {num_code} codes = {B * num_code} lower samples: at most {MAX_LOWER} per call")
    return layer


def adam_table(lr, num_step, lr_rampup_ratio, lr_rampdown_ratio, noise=None):
    """[num_step + 1][3] per-step scalars of torch's Adam under the LambdaLR schedule, formed the way torch forms them (LambdaLR's
    lr a Python float, the step count a float32 tensor, so the bias corrections and the step size are float32 tensor
    arithmetic): lr(k) / (1 - beta1^(k+1)), sqrt(1 - beta2^(k+1)), and noise(k) (0 without)"""
    b1, b2 = 0.9, 0.999   # torch.optim.Adam's defaults
    rows = []
    for k in range(num_step + 1):
        t = torch.tensor(float(k + 1))
        step_lr = float(lr) * lr_schedule(k, num_step, lr_rampup_ratio, lr_rampdown_ratio)
        rows.append(torch.stack([step_lr / (1 - b1 ** t), (1 - b2 ** t).sqrt(),
                                 torch.tensor(noise(k) if noise is not None else 0.0)]))
    return torch.stack(rows).float().contiguous()


class InvState:
    """Everything one inversion's steps read and write, allocated before the loop."""

    NCHUNK = 16   # workgroups per sample of dg_inv_loss_grad
    num_code = 1

    def __init__(self, inv_ref, mask_ref, latent, gumbel, *, num_step, distance, lr, perturb_latent, noise_ratio,
                 noise_sigma, lr_rampup_ratio, lr_rampdown_ratio, seed, lidar=None, tol=1e-8, row0=0, emd_points=2048):
        dev = inv_ref.device
        self.row0 = int(row0)   # the perturbation's row key of latent row 0
        B, _, H, W = inv_ref.shape
        self.B, self.HW = B, H * W
        self.ref = inv_ref.detach().float().contiguous()
        self.mask = mask_ref.detach().float().contiguous()
        self.msum = self.mask.sum(dim=(1, 2, 3)).contiguous()   # integers: exact in any order
        names = check_distance(distance, lidar)
        self.terms = tuple({"l1": 0, "l2": 1}[n] for n in names if n not in POINT_TERMS)   # dg_inv_loss_grad's distance codes
        self.chamfer = ChamferState(inv_ref, lidar, tol) if "chamfer" in names else None
        self.emd = None
        if "emd" in names:   # (R and P are the Chamfer term's where both are selected: one dg_inv_to_xyz per step)
            self.emd = EmdState(self.chamfer if self.chamfer is not None else PointMaps(inv_ref, lidar, tol), emd_points)
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
        self.sched = adam_table(lr, num_step, lr_rampup_ratio, lr_rampdown_ratio,
                                lambda k: noise_strength(k, num_step, noise_ratio, noise_sigma)).to(dev)
        self.hp = (int(num_step), b1, b2, 1e-8, int(bool(perturb_latent)), int(seed) & (2**64 - 1), STREAM_PERTURB)
        self._ramps = (lr_rampup_ratio, lr_rampdown_ratio)

    def multi_code(self, lower, layer, num_code, alpha, alpha_lr):
        """make this a multi-code state: self.latent holds the B N rows (row s N + n: code n of scan s), `lower` is the GEngine of
        the lower layers at batch B N, `alpha` [B,N,C] the composition weights (stepped in place) with their Adam moments, the
        gradient and the fixed-order sum's scratch of dg_feat_compose_bwd"""
        dev = self.latent.device
        self.lower, self.layer, self.num_code = lower, int(layer), int(num_code)
        P, C = lower.compose_geometry(self.layer)
        assert alpha.shape == (self.B, self.num_code, C) and self.latent.shape[0] == self.B * self.num_code
        self.alpha = alpha
        self.m_alpha = torch.zeros_like(alpha)
        self.v_alpha = torch.zeros_like(alpha)
        self.dalpha = torch.zeros_like(alpha)
        # workgroups per (scan, code) of the backward composition: about 64 KB of the feature map each, at most 64
        es = 2 if lower.dtype == torch.bfloat16 else 4
        self.cnchunk = max(1, min(64, P, (P * C * es) // 65536))
        rows = self.B * self.num_code
        self.cparts = torch.zeros(rows * self.cnchunk * C, dtype=torch.float32, device=dev)
        self.ctickets = torch.zeros(rows, dtype=torch.int32, device=dev)
        self.sched_a = adam_table(alpha_lr, self.hp[0], *self._ramps).to(dev)

    def alpha_launch(self):
        """dg_alpha_adam on d loss / d alpha at the device step index, BEFORE the step's dg_sphere_adam advances it"""
        ns, b1, b2, eps = self.hp[:4]
        L.check(L.lib().dg_alpha_adam(L.ptr(self.dalpha), L.ptr(self.alpha), L.ptr(self.m_alpha), L.ptr(self.v_alpha),
                                      L.ptr(self.step), L.ptr(self.sched_a), ns, b1, b2, eps, self.alpha.numel(),
                                      L.stream_ptr()), "dg_alpha_adam")

    def optimizer_launch(self, dzT, zT, z_dtype, prime=False):
        """dg_sphere_adam on the gradient dz^T [nz][Bp] (prime: only the first step's generator input into zT)"""
        B, nz = self.latent.shape
        Bp = dzT.shape[1] if dzT is not None else 0
        ns, b1, b2, eps, pert, seed, sid = self.hp
        L.check(L.lib().dg_sphere_adam_rows(L.ptr(dzT), 1, Bp, L.ptr(self.latent), L.ptr(self.m), L.ptr(self.v), L.ptr(self.step),
                                            L.ptr(self.ticket), L.ptr(self.noise_in), L.ptr(zT), z_dtype, B, nz, L.ptr(self.sched),
                                            ns, b1, b2, eps, pert, seed, sid, int(prime), self.row0, L.stream_ptr()),
                "dg_sphere_adam_rows")


def invert(G, inv_ref, mask_ref, *, num_step=1000, distance="l1", lr=0.1, perturb_latent=True, noise_ratio=0.75,
           noise_sigma=1.0, lr_rampup_ratio=0.05, lr_rampdown_ratio=0.25, seed=0, latent=None, graph=True,
           noise_fn=None, gumbel_noise=None, on_step=None, lidar=None, tol=1e-8, num_code=1, composition_layer=None,
           alpha=None, alpha_lr=1e-3, first_index=0, emd_points=2048):
    """Reconstruct inv_ref [B,1,H,W] (inverse depth in [0,1]) under mask_ref [B,1,H,W] by optimising G's latent
    (evaluate_reconstruction.py:84-118).  G: what utils.setup returns (the bare 'none' generator or a DUSty1 / DUSty2
    wrapper), run in eval mode at its own precision; nothing of G is modified.
    distance: "l1", "l2", "chamfer", "emd" or a sequence of them; the per-sample loss is their sum (demo.py:509-519).  "chamfer"
    and "emd" need lidar= (utils.lidar.LiDAR with its angle grid) and take tol, postprocess's validity threshold.
    "emd" (beyond the reference's demo): the earth mover's distance the evaluation reports (compute_emd), between the target's
    emd_points furthest-point samples - drawn once, by the evaluation's own sampler - and the generated points on the same
    rays, divided by emd_points; 1 <= emd_points <= min(3200, H W), and every scan needs that many points at 1e-3 or more of
    squared unit range (ValueError before the first step).  Without "emd" the argument is not looked at.
    latent: the initial latent [B,nz] (default: Philox normal draws of `seed`, rows normalised as the reference does).
    Test hooks: noise_fn(k) -> the perturbation [B,nz] added to the latent at step k (replaces the Philox draws; eager
    loop), gumbel_noise [1,1,H,W] the fixed pixel-level logistic noise of the dusty archs, on_step(k, loss [B],
    d loss / d latent [B,nz], latent [B,nz]) after every step (eager loop).
    graph: capture one step (after two eager ones) and replay it; results equal the eager loop's bit for bit.
    Returns {"latent", "out", "inv_gen", "loss"}: the reference's loop variables after the loop - the optimised latent, the
    last step's generator output and tanh_to_sigmoid of its unmasked depth, and the last step's per-sample loss.

    num_code = N in 2..64: the demo's multi-code mode (mGANprior, demo.py:353-366, 466-488, 523-530).  N latents per scan run
    through G up to composition_layer - 0..3 or one of composition_layers(G)'s names: the output of Proj, Up1, Up2 or Up3 - where
    their feature maps are blended per channel with the weights alpha [B,N,C] (default 1/N, stepped by a plain Adam of
    lr alpha_lr under the same LambdaLR schedule); the blend runs through the rest of G as one sample.  Then `latent` (given and
    returned) and noise_fn(k) are [B,N,nz] - the default initial latent is the Philox draws of B N rows, row b N + n code n of
    scan b, each normalised; the device-drawn perturbation keeps its per-row keying - the result carries "alpha" [B,N,C], and
    on_step is called as on_step(k, loss [B], dlatent [B,N,nz], latent, dalpha [B,N,C], alpha).  "loss", "out" and "inv_gen" stay
    per scan.  With num_code = 1 the three other arguments must stay at their defaults (ValueError).
    The reference runs ONE scan (B = 1) under torch.manual_seed(0); B > 1 here is B independent such problems in one batch.
    first_index: the dataset index of the batch's first scan.  Scan b draws its default initial latent and its perturbations as
    latent row(s) (first_index + b) N .. of one long batch, so a scan keyed by its index draws the same numbers in whatever
    batch it travels (0: the batch's own rows; above 0 the default latent needs N nz % 4 == 0, a Philox group per 4 elements).
    The lower layers run at batch B N, at most 4096 per call (ValueError): GEngine.alloc holds per lower sample the
    feature maps a0..a3 and their gradients (2 x 1 966 080 elements at 64 x 1024 with 512 / 256 / 128 / 64 channels: 7.9 MB in
    bf16, 15.7 MB in fp32) plus the head's buffers (gout, draw, mask, depth, in bf16 the pixel-major gradient and a3's mask bits:
    2.4 - 3.0 MB with three heads) - roughly 10 MB in bf16 and 17 MB in fp32.  fp32x3 split storage is not built for it."""
    from .utils.lidar import unit_map
    if "emd" in check_distance(distance, lidar):
        check_emd_points(emd_points, inv_ref.shape[2] * inv_ref.shape[3])
    bb = _backbone(G)
    layer = check_multi_code(num_code, composition_layer, alpha, alpha_lr, inv_ref.shape[0], wrapped=bb is not G)
    N = int(num_code)
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
    if N > 1 and eng.x2_asked:
        raise NotImplementedError("multi-code inversion is not built for the fp32x3 split storage (x2)")
    first_index = int(first_index)
    if first_index < 0 or (first_index + B) * N >= 2**31:
        raise ValueError(f"first_index: 0 <= (first_index + B) num_code < 2^31, got {first_index}")
    if latent is None:
        if first_index and (N * bb.in_ch) % 4:
            raise ValueError("first_index > 0 draws the default latent per scan: num_code * nz must be a multiple of 4")
        latent = _draw_normal(int(seed) & (2**64 - 1), STREAM_LATENT, B * N * bb.in_ch, dev,
                              offset=first_index * N * bb.in_ch // 4).view(B * N, bb.in_ch)
        normalize_rows(latent)
    elif N > 1 and tuple(latent.shape) != (B, N, bb.in_ch):
        raise ValueError(f"latent must be [B,N,nz] = {(B, N, bb.in_ch)} with num_code > 1")
    latent = latent.detach().to(dev).float().clone().contiguous().view(B * N, bb.in_ch)
    S = InvState(inv_ref, mask_ref, latent, _fixed_gumbel(G, B, H, W, seed, dev, gumbel_noise), num_step=num_step,
                 distance=distance, lr=lr, perturb_latent=perturb_latent, noise_ratio=noise_ratio, noise_sigma=noise_sigma,
                 lr_rampup_ratio=lr_rampup_ratio, lr_rampdown_ratio=lr_rampdown_ratio, seed=seed,
                 lidar=lidar, tol=tol, row0=first_index * N, emd_points=emd_points)
    # every buffer of the loop exists before it, allocated on the caller's stream
    eng.alloc(B, dev)
    low = eng   # the engine the latents enter: the generator's own, or the lower one of a multi-code inversion
    if N > 1:
        low = E.GEngine(eng.cfg, eng.dtype, x3=eng.ops.x3)
        low.alloc(B * N, dev)
        C = low.chs[layer]
        if alpha is None:
            alpha = torch.full((B, N, C), 1.0 / N)
        elif tuple(alpha.shape) != (B, N, C):
            raise ValueError(f"alpha must be [B,N,C] = {(B, N, C)}")
        S.multi_code(low, layer, N, alpha.detach().to(dev).float().clone().contiguous(), alpha_lr)
    low.grad_z_buffers()
    zdt = L.dtype_code(eng.dtype)
    zero = torch.zeros_like(latent)

    def injected(k):
        if not perturb_latent:
            return zero
        return noise_fn(k).to(dev).float().contiguous().view(B * N, -1) if k < num_step else zero

    def report(k):
        dz = low._dzw[:, :B * N].t()
        if N == 1:
            return on_step(k, S.loss.clone(), dz.clone(), S.latent.clone())
        return on_step(k, S.loss.clone(), dz.reshape(B, N, -1).clone(), S.latent.view(B, N, -1).clone(), S.dalpha.clone(),
                       S.alpha.clone())

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
            S.optimizer_launch(None, low.zT, zdt, prime=True)
            out = None
            n_eager = min(num_step, 2) if graph else num_step
            for k in range(n_eager):
                if noise_fn is not None:
                    S.noise_in = injected(k + 1)
                out = eng.inversion_step(st, S)
                if on_step is not None:
                    report(k)
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
    res = {"latent": S.latent.clone(), "out": res_out, "inv_gen": unit_map(depth, 0), "loss": S.loss.clone()}
    if N > 1:
        res["latent"] = res["latent"].view(B, N, -1)
        res["alpha"] = S.alpha.clone()
    return res
