"""Ray-drop transfer: the drops G infers for a scan, applied to the scan's own points.

The DUSty paper trains the measurability head for this: a simulator's COMPLETE scan is inverted through G's unmasked depth,
the measurability G predicts at the optimised latent is sampled, and the simulated points are dropped with it - geometry and
per-point annotations stay the simulator's, only the drops are G's.  The reference's repository holds no code for the
experiment; the kernels are csrc/raydrop.hip and run on the GPU only.

    pixel_winner   which input point a pixel of the projection stands for (the nearest; the lowest index on a tie)
    sample_keep    K realisations of keep = (a point fell here) and G's masks, from injected or Philox logistic noise
    gather         per realisation the surviving records, labels and point indices, in row-major pixel order
    transfer       cloud -> projection -> inversion -> the three above

Draws: scan i of a dataset, realisation k, pixel p takes element p of the logistic draw of H W elements of Philox (seed, stream
word STREAM_RAYDROP | k << 32) at counter offset i 2 ceil(H W / 4) - as corruption.py keys a scan's draws by its dataset index
(`first_index`: that of the batch's first scan), so neither the batch a scan travels in nor K changes a number."""
import torch

from . import _lib as L
from .utils.render import _workspace   # zero-at-rest u64 words per (device, stream, size)

STREAM_RAYDROP = 15    # Philox stream id (0-14: inversion.py and corruption.py list them)
ARCH = {"dusty1": 1, "dusty2": 2}
EPS = 1e-10            # GumbelSigmoid.eps


def _gpu(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"{what} runs on the GPU only (no CPU fallback)")
    return t


def _records(records, what):
    _gpu(records, what)
    if records.ndim != 3 or records.shape[2] not in (3, 4) or records.shape[0] < 1 or records.shape[1] < 1:
        raise ValueError(f"{what}: expected [B,N,3] or [B,N,4] records, got {tuple(records.shape)}")
    if records.dtype != torch.float32:
        raise ValueError(f"{what}: float32 records, got {records.dtype}")
    return records.contiguous()


def pixel_winner(records, idx, counts, H, W):
    """records [B,N,3|4] and counts [B] (or None) as given to LiDAR.points_to_depth, idx [B,N] as it returned with
    return_index -> win [B,H W] int32: the nearest of the points binned into every pixel (smallest |xyz|, rounded to float32;
    the lowest index on a tie), -1 where none fell (dg_pixel_winner)"""
    x = _records(records, "pixel_winner")
    B, N, stride = x.shape
    if tuple(idx.shape) != (B, N):
        raise ValueError(f"pixel_winner: idx must be [B,N] = {(B, N)}, got {tuple(idx.shape)}")
    idx = _gpu(idx, "pixel_winner").to(torch.int32).contiguous()
    if counts is not None:
        if tuple(counts.shape) != (B,):
            raise ValueError(f"pixel_winner: counts must be [B] = [{B}], got {tuple(counts.shape)}")
        counts = counts.to(device=x.device, dtype=torch.int32).contiguous()
    win = torch.empty(B, H * W, dtype=torch.int32, device=x.device)
    ws = _workspace(x.device, B * H * W)
    try:
        L.check(L.lib().dg_pixel_winner(L.ptr(x), N * stride, stride, L.ptr(counts), L.ptr(idx), B, N, H, W, L.ptr(ws), L.ptr(win),
                                        L.stream_ptr()), "dg_pixel_winner")
    except BaseException:
        ws.zero_()   # (a failure between the two launches must not leave keys behind: the words are zero at rest)
        raise
    return win


def sample_keep(conf, win, masker, tau, *, realisations=1, seed=0, first_index=0, noise=None, return_noise=False):
    """conf [B,C,H,W]: G's RAW confidence logits (C = 1 dusty1, 2 dusty2: inversion.invert's out["confidence"]); win [B,H W];
    tau: the Gumbel sigmoid's temperature -> keep [B,K,H,W] uint8 = win >= 0 and the masks the generator's head forms in eval
    mode (the pixel mask from h1 + noise, dusty2's image mask from the sign of h2).  noise [B,K,1,H,W] injects the logistic
    noise; None draws it (module docstring).  return_noise: also the noise used [B,K,1,H,W] (dg_raydrop_keep)."""
    if masker not in ARCH:
        raise ValueError(f"masker {masker!r} has no measurability head: nothing to transfer")
    _gpu(conf, "sample_keep")
    K = int(realisations)
    if conf.ndim != 4 or conf.shape[1] != ARCH[masker]:
        raise ValueError(f"sample_keep: {masker} logits are [B,{ARCH[masker]},H,W], got {tuple(conf.shape)}")
    if K < 1:
        raise ValueError("sample_keep: realisations must be at least 1")
    if not float(tau) > 0:
        raise ValueError(f"sample_keep: tau must be positive, got {tau}")
    B, C, H, W = conf.shape
    if tuple(win.shape) != (B, H * W):
        raise ValueError(f"sample_keep: win must be [B,H W] = {(B, H * W)}, got {tuple(win.shape)}")
    conf = conf.detach().float().contiguous()
    win = _gpu(win, "sample_keep").to(torch.int32).contiguous()
    if noise is not None:
        if tuple(noise.shape) != (B, K, 1, H, W):
            raise ValueError(f"sample_keep: noise must be [B,K,1,H,W] = {(B, K, 1, H, W)}, got {tuple(noise.shape)}")
        noise = noise.to(device=conf.device, dtype=torch.float32).contiguous()
    keep = torch.empty(B, K, H, W, dtype=torch.uint8, device=conf.device)
    used = torch.empty(B, K, 1, H, W, dtype=torch.float32, device=conf.device) if return_noise else None
    L.check(L.lib().dg_raydrop_keep(L.ptr(conf), C, L.ptr(win), L.ptr(noise), int(seed) & (2**64 - 1), STREAM_RAYDROP,
                                    int(first_index), EPS, float(tau), B, K, H, W, L.ptr(keep), L.ptr(used), L.stream_ptr()),
            "dg_raydrop_keep")
    return (keep, used) if return_noise else keep


def _label_bits(labels):
    """integer labels in [0, 2^32) (or their uint32 bits as int32 already) -> the uint32 bits as int32: torch has no arithmetic
    on uint32, and the kernel only copies them"""
    if labels.dtype == torch.int32:
        return labels
    v = labels.to(torch.int64)
    return torch.where(v >= 2**31, v - 2**32, v).to(torch.int32)


def gather(records, win, keep, labels=None, *, out=None):
    """records [B,N,3|4] float32 - ANY buffer of the cloud's layout; a command passes the records in metres as read from the
    file, so what comes out is what went in, bit for bit - win [B,H W], keep [B,K,H,W], labels [B,N] (integers below 2^32,
    optional) -> (out_records [B,K,H W,4], out_labels [B,K,H W] int32 holding the labels' uint32 bits - on the host
    `.numpy().view(np.uint32)` - or None, out_index [B,K,H W] int32, out_counts [B,K] int32): per (b, k) the kept pixels'
    winners in row-major pixel order; rows at and beyond the count are not written.  out: (out_records, out_labels or None,
    out_index) to write into instead of fresh tensors (dg_raydrop_gather)."""
    x = _records(records, "gather")
    B, N, stride = x.shape
    _gpu(keep, "gather")
    if keep.ndim != 4 or keep.shape[0] != B or keep.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"gather: keep must be uint8 [B,K,H,W] with B = {B}, got {keep.dtype} {tuple(keep.shape)}")
    _, K, H, W = keep.shape
    HW = H * W
    if tuple(win.shape) != (B, HW):
        raise ValueError(f"gather: win must be [B,H W] = {(B, HW)}, got {tuple(win.shape)}")
    keep = keep.contiguous().view(torch.uint8)
    win = _gpu(win, "gather").to(torch.int32).contiguous()
    lab = None
    if labels is not None:
        if tuple(labels.shape) != (B, N):
            raise ValueError(f"gather: labels must be [B,N] = {(B, N)}, one per record, got {tuple(labels.shape)}")
        lab = _label_bits(labels.to(device=x.device)).contiguous()
    dev = x.device
    if out is None:
        out = (torch.empty(B, K, HW, 4, dtype=torch.float32, device=dev),
               torch.empty(B, K, HW, dtype=torch.int32, device=dev) if lab is not None else None,
               torch.empty(B, K, HW, dtype=torch.int32, device=dev))
    out_rec, out_lab, out_idx = out
    for t, shape, dt in ((out_rec, (B, K, HW, 4), torch.float32), (out_lab, (B, K, HW), torch.int32), (out_idx, (B, K, HW), torch.int32)):
        if t is not None and not (tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous() and t.device == dev):
            raise ValueError(f"gather: out tensors are contiguous {dt} {shape} on {dev}")
    if (out_lab is None) != (lab is None):
        raise ValueError("gather: out_labels goes with labels")
    counts = torch.empty(B, K, dtype=torch.int32, device=dev)
    chunks = torch.empty(B * K * ((HW + L.EXPORT_CHUNK - 1) // L.EXPORT_CHUNK), dtype=torch.int32, device=dev)
    L.check(L.lib().dg_raydrop_gather(L.ptr(x), N * stride, stride, N, L.ptr(win), L.ptr(keep), L.ptr(lab), B, K, H, W,
                                      L.ptr(chunks), L.ptr(out_rec), L.ptr(out_lab), L.ptr(out_idx), L.ptr(counts),
                                      L.stream_ptr()), "dg_raydrop_gather")
    return out_rec, out_lab, out_idx, counts


def transfer(G, lidar, records_unit, counts, *, records_raw=None, labels=None, realisations=1, noise="sample", seed=0,
             first_index=0, tau=2, corruption=None, corruption_seed=0, **invert_kwargs):
    """The paper's transfer for B clouds.  records_unit [B,N,3|4]: the clouds in unit space (metres / max_depth) with counts
    [B], as datasets.raw.read_clouds returns them; records_raw: the buffer the output records are copied from (default
    records_unit; the command passes the records in metres); labels [B,N] optional.
      1. LiDAR.points_to_depth(tau=tau, return_index=True) -> the inversion's target, mask = the pixels a point fell in
         (corruption: one of corruption.CORRUPTIONS applied to it first - "closing" pre-fills a sparse simulator frame);
      2. inversion.invert against it (invert_kwargs: num_step, distance, num_code ... - "chamfer" and "emd" get lidar=) and the raw
         confidence logits of the optimised latent;
      3. pixel_winner -> sample_keep -> gather.  noise="sample": `realisations` Philox draws keyed by (seed, first_index + b,
         k); "fixed": the inversion's own fixed Gumbel noise (what G's head applied in the last step; realisations == 1).
    Returns a dict: "records" [B,K,H W,4], "labels" (or None), "index", "counts" [B,K] (gather's), "keep" [B,K,H,W] uint8,
    "win" [B,H W], "target" [B,1,H,W] normalised depth, "valid" [B,1,H,W] bool, "confidence" [B,1,H,W] the pixel
    confidence's sigmoid, "loss" [B] the inversion's final loss, "out" the generator's raw outputs at the optimised latent."""
    from .corruption import apply_corruption
    from .inversion import _backbone, _fixed_gumbel, invert
    from .utils.lidar import unit_map
    bb = _backbone(G)
    if bb.masker not in ARCH:
        raise ValueError(f"a generator without a measurability head (masker {bb.masker!r}) has nothing to transfer")
    if noise not in ("sample", "fixed"):
        raise ValueError(f"noise: 'sample' or 'fixed', got {noise!r}")
    K = int(realisations)
    if noise == "fixed" and K != 1:
        raise ValueError("noise='fixed' is one realisation: the inversion's own fixed Gumbel noise")
    x = _records(records_unit, "transfer")
    B, N, _ = x.shape
    raw = x if records_raw is None else _records(records_raw, "transfer")
    if raw.shape[:2] != (B, N):
        raise ValueError(f"transfer: records_raw must hold the same [B,N] = {(B, N)} records, got {tuple(raw.shape)}")
    if labels is not None and tuple(labels.shape) != (B, N):
        raise ValueError(f"transfer: labels must be [B,N] = {(B, N)}, one per record, got {tuple(labels.shape)}")
    H, W = lidar.H, lidar.W
    depth, valid, idx = lidar.points_to_depth(x, drop_value=1, tau=tau, counts=counts, return_index=True)
    mask = valid.float()
    dep_t, mask_t = apply_corruption(depth, mask, corruption, seed=corruption_seed, first_index=first_index)
    inv_ref = mask_t * lidar.invert_depth(dep_t)
    if hasattr(G, "_sync"):
        G._sync()
    fixed = _fixed_gumbel(G, 1, H, W, seed, x.device, invert_kwargs.pop("gumbel_noise", None))["pixel"]
    names = invert_kwargs.get("distance", "l1")
    names = (names,) if isinstance(names, str) else tuple(names)
    if "chamfer" in names or "emd" in names:
        invert_kwargs.setdefault("lidar", lidar)
    res = invert(G, inv_ref, mask_t, seed=seed, gumbel_noise=fixed, first_index=first_index, **invert_kwargs)
    conf = res["out"]["confidence"]
    win = pixel_winner(x, idx, counts, H, W)
    injected = fixed.view(1, 1, 1, H, W).expand(B, 1, 1, H, W) if noise == "fixed" else None
    keep = sample_keep(conf, win, bb.masker, bb.tau, realisations=K, seed=seed, first_index=first_index, noise=injected)
    rec, lab, index, cnt = gather(raw, win, keep, labels)
    return {"records": rec, "labels": lab, "index": index, "counts": cnt, "keep": keep, "win": win, "target": depth,
            "valid": valid, "confidence": unit_map(conf[:, 0:1], 1), "loss": res["loss"], "out": res["out"]}
