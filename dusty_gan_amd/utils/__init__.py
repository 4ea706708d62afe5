"""Host-side helpers mirrored from the reference's utils/__init__.py (only the four on the hot path,
SURVEY.md §2, and masked_loss of the reconstruction evaluation) plus the engine's Philox stream."""


def set_requires_grad(net, requires_grad: bool = True):
    """reference: utils/__init__.py:59-61.  The engine has no autograd; kept so callers need not change."""
    for param in net.parameters():
        param.requires_grad = requires_grad


def sigmoid_to_tanh(x):
    """[0,1] -> [-1,+1]  (reference: utils/__init__.py:70-73)"""
    return x * 2.0 - 1.0


def tanh_to_sigmoid(x):
    """[-1,+1] -> [0,1]  (reference: utils/__init__.py:76-79)"""
    return (x + 1.0) / 2.0


def cycle(iterable):
    """reference: utils/__init__.py:110-113"""
    while True:
        for i in iterable:
            yield i


def setup(model_path, config_path, ema=True, fix_noise=True, cuda=True):
    """reference: utils/__init__.py:116-160 -- what evaluate_*.py / demo.py call to get a generator back from a
    checkpoint: (cfg, G, lidar, device).  `cuda=False` is refused: this engine has no CPU path."""
    import os.path as osp

    import torch

    from ..models import define_G
    from ..models.dusty import GumbelSigmoid
    from .config import load_config_file
    from .lidar import LiDAR
    if not (cuda and torch.cuda.is_available()):
        raise RuntimeError("dusty_gan_amd.utils.setup needs an MI355X (no CPU path)")
    device = torch.device("cuda")
    cfg = load_config_file(config_path)
    cfg.model.gen.shape = cfg.dataset.shape
    cfg.model.dis.shape = cfg.dataset.shape
    assert ".pth" in model_path
    checkpoint = torch.load(model_path, map_location="cpu")
    G_state_dict = checkpoint["G_ema"] if ema else checkpoint["G"]
    print("#iterations:", checkpoint["step"])
    G = define_G(cfg)
    G.eval()
    G.load_state_dict(G_state_dict)
    G.to(device)
    if hasattr(G, "_sync"):
        G._sync()   # (a learnable temperature: the by-value tau of the inference paths, one host read of the loaded weight)
    if fix_noise:
        for m in G.modules():
            if isinstance(m, GumbelSigmoid):
                m.fix_on_first_use = True
    root = cfg.dataset.get("root")
    lidar = LiDAR(num_ring=cfg.dataset.shape[0], num_points=cfg.dataset.shape[1], min_depth=cfg.dataset.min_depth,
                  max_depth=cfg.dataset.max_depth, angle_file=osp.join(root, "angles.pt") if root else None)
    if str(cfg.dataset.name) == "synthetic":
        lidar.use_nominal_angles()
    lidar.to(device)
    return cfg, G, lidar, device


def masked_loss(img_ref, img_gen, mask, distance="l1"):
    """reference: utils/__init__.py:237-246 -> per-sample [B] sum(|ref - gen| or (ref - gen)^2) mask / sum(mask) for
    [B,1,H,W] images, on the kernel GAN inversion uses (csrc/inversion.hip dg_inv_loss_grad, forward only)"""
    import torch

    from .. import _lib as L
    if distance not in ("l1", "l2"):
        raise NotImplementedError
    if not img_gen.is_cuda:
        raise RuntimeError("masked_loss runs on the GPU only (no CPU fallback)")
    ref, gen, m = (t.contiguous().float() for t in (img_ref, img_gen, mask))
    assert ref.shape == gen.shape == m.shape and ref.ndim == 4 and ref.shape[1] == 1
    B, HW = ref.shape[0], ref.shape[2] * ref.shape[3]
    msum = m.sum(dim=(1, 2, 3)).contiguous()
    nchunk = max(1, min(16, HW // 1024))
    parts = torch.zeros(B * nchunk, dtype=torch.float32, device=gen.device)
    tickets = torch.zeros(B, dtype=torch.int32, device=gen.device)
    loss = torch.empty(B, dtype=torch.float32, device=gen.device)
    L.check(L.lib().dg_inv_loss_grad(L.ptr(gen), HW, 0, L.ptr(ref), L.ptr(m), L.ptr(msum), int(distance == "l2"), B, HW,
                                     1.0, None, 1, None, 1, L.ptr(parts), L.ptr(tickets), nchunk, L.ptr(loss),
                                     L.stream_ptr()), "dg_inv_loss_grad")
    return loss
