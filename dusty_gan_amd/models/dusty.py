"""DUSty measurability wrappers -- reference: models/dusty.py.

The Gumbel-sigmoid sampling and the mask-out are fused into the generator's head kernels
(csrc/head_post.hip head_post_fwd/bwd); these classes keep the reference's module names, buffers and the
`GumbelSigmoid.fixed_noise` / `logistic_noise` hooks that utils.setup relies on (utils/__init__.py:141-149).

Learnable temperature (`model.gen.tau: null`, reference models/dusty.py:25-26, 38-43): every GumbelSigmoid owns a scalar
`weight` and the sigmoid's slope is softplus(weight) + 1 / tau_max.  The weights live in one trailing segment `tau_w` of the
backbone's flat ParamStore (pixel, then image), so zeroing, Adam, the EMA into G_ema, the gradient exchange and resume treat
them like every other parameter; the head kernels read the fp32 master weights from memory (dg_head_post_*_lt) and add their
gradients into the segment's slice of the flat gradient.  The paths that take tau by value (GAN inversion, ray-drop
sampling) get it from `_DUSty._sync`: one host read of the pixel weight, never inside a graph capture.
"""
import math

import torch
from torch import nn

from ..utils.rng import Philox


class GumbelSigmoid(nn.Module):
    """reference: models/dusty.py:6-62 (hard=True; tau fixed, or None = learnable: a scalar `weight`, which the DUSty
    wrapper rebinds to a view of the backbone's flat store).  Holds the noise policy; the arithmetic is fused."""

    def __init__(self, tau: float = 1.0, tau_max: float = 1.0, hard: bool = True, eps: float = 1e-10,
                 pixelwise: bool = True):
        super().__init__()
        if not hard:
            raise NotImplementedError("GumbelSigmoid(hard=False): soft masks are not implemented - the fused head kernels form "
                                      "the hard mask with the straight-through gradient, the only form models.define_G builds "
                                      "(reference models/dusty.py:69, 98-99)")
        if tau is None:
            if not float(tau_max) > 0:
                raise ValueError(f"GumbelSigmoid: tau_max must be positive, got {tau_max}")
            self.weight = nn.Parameter(torch.tensor(0.0))
        self.tau, self.tau_max, self.hard, self.eps, self.pixelwise = tau, tau_max, hard, eps, pixelwise
        self.fixed_noise = None
        self.fix_on_first_use = False  # utils.setup(fix_noise=True): what the reference's forward-pre-hook does
        self._rng = None

    def rng(self, device):
        if self._rng is None or self._rng.device != device:
            self._rng = Philox(torch.initial_seed() + (17 if self.pixelwise else 29), device, stream_id=3)
        return self._rng

    def logistic_noise(self, logits):
        B, _, H, W = logits.shape
        shape = (B, 1, H, W) if self.pixelwise else (B, 1, 1, 1)
        return self.rng(logits.device).logistic_noise(shape, self.eps)

    def noise_for(self, B, H, W, device):
        if self.fixed_noise is not None:
            shape = (-1, -1, -1) if self.pixelwise else (-1, -1, -1)
            return self.fixed_noise.to(device).expand(B, *shape).contiguous()
        shape = (B, 1, H, W) if self.pixelwise else (B, 1, 1, 1)
        noise = self.rng(device).logistic_noise(shape, self.eps)
        if self.fix_on_first_use:
            # utils/__init__.py:141-149: `m.fixed_noise = m.logistic_noise(i[0])[[0]]` on the first call, reused after
            self.fixed_noise = noise[[0]].clone()
            return self.fixed_noise.expand(B, -1, -1, -1).contiguous()
        return noise

    def forward(self, logits, threshold: float = 0.5):
        raise RuntimeError("GumbelSigmoid is fused into the generator head kernels; call the DUSty wrapper")

    def extra_repr(self):
        return f"hard={self.hard}, eps={self.eps}"


class _DUSty(nn.Module):
    def __init__(self, backbone, tau, drop_const=-1):
        super().__init__()
        self.backbone = backbone
        self.register_buffer("drop_const", torch.tensor(drop_const).float())
        self._tau = None if tau is None else float(tau)
        self._drop = float(drop_const)
        self._gumbels = []   # the wrapper's GumbelSigmoids in parameter order: pixel[, image]

    TAU_MAX = 1.0   # GumbelSigmoid's default, which the reference's wrappers never override (models/dusty.py:69, 98-99)

    def _own_gumbels(self, *gumbels):
        """called by the subclass once its GumbelSigmoids exist.  Learnable temperature: one trailing segment `tau_w` of the
        backbone's store, a float per sigmoid, zero like the reference's init; `weight` becomes a view of it"""
        self._gumbels = list(gumbels)
        if self._tau is None:
            bb = self.backbone
            bb.store.extend([("tau_w", (len(self._gumbels),), "scalar")])
            bb._rebind()
            bb.tau_learn, bb.inv_tau_min = True, 1.0 / self.TAU_MAX
            self._rebind_tau()

    def _tau_pairs(self):
        return [(g.weight, lambda st, k=k: st.view("tau_w")[k]) for k, g in enumerate(self._gumbels)] if self._tau is None else []

    def _bind_pairs(self):
        """the backbone's (Parameter, view factory) pairs, then the temperature weights': named_parameters() order"""
        return self.backbone._bind_pairs() + self._tau_pairs()

    def _rebind_tau(self):
        with torch.no_grad():
            for p, mk in self._tau_pairs():
                p.data = mk(self.backbone.store)

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)   # (the backbone moves its store; a GumbelSigmoid would leave with a copy of its weight)
        self._rebind_tau()
        return self

    def _sync(self, latent=None):
        """the wrapper's tau / drop_const onto the backbone.  Learnable temperature: the by-value tau of the inference paths
        (inversion kernels, raydrop.sample_keep) is 1 / (softplus(w_pixel) + 1 / tau_max) from ONE host read of the master
        weight - a device synchronisation, made by an explicit call (utils.setup, inversion.invert, raydrop.transfer) or an
        eval-mode forward, not by a training forward (the step's kernels read the weights from memory) and never while a graph
        is being captured.  Only the pixel sigmoid's slope matters there: eval mode thresholds the
        image logit."""
        if latent is not None:
            self.backbone._require_gpu(latent)
        if self._tau is not None:
            self.backbone.tau = self._tau
        elif (latent is None or not self.training) and not (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()):
            w = float(self.backbone.store.view("tau_w")[0])
            self.backbone.tau = 1.0 / (_softplus(w) + 1.0 / self.TAU_MAX)
        self.backbone.drop_const = self._drop

    def set_precision(self, dtype):
        self.backbone.set_precision(dtype)

    @property
    def store(self):
        return self.backbone.store


def _softplus(w):
    return w + math.log1p(math.exp(-w)) if w > 0 else math.log1p(math.exp(w))


class DUSty1(_DUSty):
    """reference: models/dusty.py:65-91"""

    def __init__(self, backbone, tau, drop_const=-1):
        super().__init__(backbone, tau, drop_const)
        self.gumbel = GumbelSigmoid(hard=True, tau=tau, pixelwise=True)
        assert backbone.masker == "dusty1", "DUSty1 needs a generator with a 1-channel confidence head"
        self._own_gumbels(self.gumbel)

    def forward(self, latent, noise=None, **kwargs):
        self._sync(latent)
        H, W = self.backbone.shape
        if noise is None:
            noise = {"pixel": self.gumbel.noise_for(latent.shape[0], H, W, latent.device)}
        return self.backbone.run(latent, noise, self.training)


class DUSty2(_DUSty):
    """reference: models/dusty.py:94-127 (eval mode thresholds the image-level logit, still samples pixel noise)"""

    def __init__(self, backbone, tau, drop_const=-1):
        super().__init__(backbone, tau, drop_const)
        self.gumbel_pixel = GumbelSigmoid(hard=True, tau=tau, pixelwise=True)
        self.gumbel_image = GumbelSigmoid(hard=True, tau=tau, pixelwise=False)
        assert backbone.masker == "dusty2", "DUSty2 needs a generator with a 2-channel confidence head"
        self._own_gumbels(self.gumbel_pixel, self.gumbel_image)

    def forward(self, latent, noise=None, **kwargs):
        self._sync(latent)
        H, W = self.backbone.shape
        B = latent.shape[0]
        if noise is None:
            noise = {"pixel": self.gumbel_pixel.noise_for(B, H, W, latent.device)}
            if self.training:
                noise["image"] = self.gumbel_image.noise_for(B, H, W, latent.device)
        return self.backbone.run(latent, noise, self.training)
