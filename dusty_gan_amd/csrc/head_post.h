// Head post-processing, the arithmetic of ONE pixel written once: Generator.forward's tanh (models/gans/dcgan_eqlr.py:71) and the
// DUSty maskout with its Gumbel-sigmoid masks (models/dusty.py:45-59, 77-91, 107-127), their first derivatives, the sigmoid
// derivatives the second-order pass builds its Hessian rows from, and the pixel-major bf16 packing of a pixel's head gradients.
// Everything works on scalars in registers; arch: 0 none, 1 dusty1, 2 dusty2 (head outputs h0 raw depth, h1 / h2 confidence
// logits).  Used by head_post.hip (forward, backward, second-order backward).
#pragma once
#include "pointwise.h"

// PX = 4 consecutive floats as one 16-byte access, or one float
template <int PX>
__device__ __forceinline__ void ld_px(const float* p, float (&v)[PX]) {
  if constexpr (PX == 4) Vec16<float>::load(p, v); else v[0] = p[0];
}
template <int PX>
__device__ __forceinline__ void st_px(float* p, const float (&v)[PX]) {
  if constexpr (PX == 4) Vec16<float>::store(p, v); else p[0] = v[0];
}
// a thread's contribution to a sum: one pixel, or a quad added pairwise
template <int PX>
__device__ __forceinline__ float px_sum(const float (&v)[PX]) {
  if constexpr (PX == 4) return (v[0] + v[1]) + (v[2] + v[3]); else return v[0];
}

// ---- the Gumbel sigmoid of a noisy logit l (= logit + logistic noise) and its derivatives in l.  The hard mask carries the
//      straight-through derivative sp' = sp (1 - sp) / tau, which is itself differentiable: sp'' = sp' (1 - 2 sp) / tau.
// d tanh / d h0 from the saved t = tanh h0
__device__ __forceinline__ float hp_dtanh(float t) { return 1.f - t * t; }
__device__ __forceinline__ float hp_sigmoid(float l, float inv_tau) { return 1.f / (1.f + __expf(-l * inv_tau)); }
// pre * sp' - the factor in front is multiplied in FIRST (the order every caller rounds in; pre = 1 is exact)
__device__ __forceinline__ float hp_dsigmoid(float pre, float s, float inv_tau) { return pre * s * (1.f - s) * inv_tau; }
__device__ __forceinline__ float hp_d2sigmoid(float s, float s1, float inv_tau) { return s1 * (1.f - 2.f * s) * inv_tau; }

// ---- the forward pixel.  raw: h0; l1 = h1 + the pixel's noise; g2 = h2, ni = the sample's image noise (read when training:
//      the eval branch of dusty2's image mask is the sign of the logit).  t = tanh h0, the masks (1 where the arch has none)
//      and the output depth m t + (1 - m) drop_const, m = mp mi.
struct HeadPx { float t, mp, mi, depth; };
template <int arch>
__device__ __forceinline__ HeadPx head_px_fwd(float raw, float l1, float g2, float ni, int training, float inv_tau,
                                              float drop_const) {
  HeadPx o;
  o.t = dg_tanh(raw);
  o.mp = 1.f; o.mi = 1.f; o.depth = o.t;
  if (arch == 0) return o;
  o.mp = hp_sigmoid(l1, inv_tau) > 0.5f ? 1.f : 0.f;
  if (arch == 2) {
    if (training) o.mi = hp_sigmoid(g2 + ni, inv_tau) > 0.5f ? 1.f : 0.f;
    else o.mi = g2 > 0.f ? 1.f : 0.f;
  }
  const float m = arch == 2 ? o.mp * o.mi : o.mp;
  o.depth = m * o.t + (1.f - m) * drop_const;
  return o;
}

// ---- the first-order gradient pixel: unscaled gradients w.r.t. the head outputs (= the head-bias gradients) from the saved
//      t, the upstream go, the noisy logits l1 and l2 = h2 + ni, and the saved masks.  Channels the arch lacks are 0.
template <int arch>
__device__ __forceinline__ void head_px_bwd(float t, float go, float l1, float l2, float mp, float mi, float inv_tau,
                                            float drop_const, float& d0, float& d1, float& d2) {
  const float dt = hp_dtanh(t);
  d1 = 0.f; d2 = 0.f;
  if (arch == 0) { d0 = go * dt; return; }
  const float sp = hp_sigmoid(l1, inv_tau);
  const float dmask = go * (t - drop_const);
  if (arch == 1) {
    d0 = mp * go * dt;
    d1 = hp_dsigmoid(dmask, sp, inv_tau);
  } else {
    const float si = hp_sigmoid(l2, inv_tau);
    d0 = mp * mi * go * dt;
    d1 = hp_dsigmoid(dmask * mi, sp, inv_tau);
    d2 = hp_dsigmoid(dmask * mp, si, inv_tau);
  }
}

// ---- the learnable temperature (models/dusty.py:25-26, 38-43: tau = None).  Each Gumbel sigmoid k owns a scalar weight w_k and
//      its slope is inv_k = softplus(w_k) + 1 / tau_max, formed in the kernel from the fp32 MASTER weight (a replayed step graph
//      follows the training).  HeadTau<false> is the by-value slope of the fixed-tau kernels - one float, their argument as before;
//      HeadTau<true> carries the weights (pixel, image), 1 / tau_max and the weights' gradient accumulators.
//      d loss / d w_k = sigma(w_k) G_k with G_k = sum over pixels of pre_k s_k (1 - s_k) l_k: the term is taken from the
//      intermediate ((pre s)(1 - s)) hp_dsigmoid forms before its last multiply, so d1 / d2 round as in the fixed-tau form.
template <bool LT> struct HeadTau;
template <> struct HeadTau<false> { float inv_tau; };
template <> struct HeadTau<true> { const float* w; float inv_min; float* dw; };
__device__ __forceinline__ float hp_inv_tau_lt(float w, float inv_min) { return log1pf(__expf(w)) + inv_min; }
__device__ __forceinline__ float hp_dinv_tau_lt(float w) { return 1.f / (1.f + __expf(-w)); }   // d inv / d w = sigma(w)

// head_px_fwd with a slope per sigmoid (dusty2's eval-mode image mask stays the sign of the logit)
template <int arch>
__device__ __forceinline__ HeadPx head_px_fwd_lt(float raw, float l1, float g2, float ni, int training, float inv_p, float inv_i,
                                                 float drop_const) {
  HeadPx o;
  o.t = dg_tanh(raw);
  o.mp = 1.f; o.mi = 1.f; o.depth = o.t;
  if (arch == 0) return o;
  o.mp = hp_sigmoid(l1, inv_p) > 0.5f ? 1.f : 0.f;
  if (arch == 2) {
    if (training) o.mi = hp_sigmoid(g2 + ni, inv_i) > 0.5f ? 1.f : 0.f;
    else o.mi = g2 > 0.f ? 1.f : 0.f;
  }
  const float m = arch == 2 ? o.mp * o.mi : o.mp;
  o.depth = m * o.t + (1.f - m) * drop_const;
  return o;
}

// head_px_bwd with a slope per sigmoid, plus the pixel's terms of G_pixel (g1) and G_image (g2): 0 where the arch has none
template <int arch>
__device__ __forceinline__ void head_px_bwd_lt(float t, float go, float l1, float l2, float mp, float mi, float inv_p, float inv_i,
                                               float drop_const, float& d0, float& d1, float& d2, float& g1, float& g2) {
  const float dt = hp_dtanh(t);
  d1 = 0.f; d2 = 0.f; g1 = 0.f; g2 = 0.f;
  if (arch == 0) { d0 = go * dt; return; }
  const float sp = hp_sigmoid(l1, inv_p);
  const float dmask = go * (t - drop_const);
  if (arch == 1) {
    d0 = mp * go * dt;
    const float q1 = dmask * sp * (1.f - sp);
    d1 = q1 * inv_p;
    g1 = q1 * l1;
  } else {
    const float si = hp_sigmoid(l2, inv_i);
    d0 = mp * mi * go * dt;
    const float q1 = dmask * mi * sp * (1.f - sp), q2 = dmask * mp * si * (1.f - si);
    d1 = q1 * inv_p;
    d2 = q2 * inv_i;
    g1 = q1 * l1;
    g2 = q2 * l2;
  }
}

// ---- the pixel-major / channel-minor bf16 copy [B,H,W,cp] of the scaled gradients, channels zero-padded: the operand layout
//      of the MFMA backward-data kernel (thin_s2_mfma).  A pixel is two 32-bit words: (d0 s_depth | d1 s_conf << 16, d2 s_conf).
__device__ __forceinline__ uint2 head_pm_words(int arch, float d0, float d1, float d2, float s_depth, float s_conf) {
  const unsigned short h0 = __builtin_bit_cast(unsigned short, (bf16)(d0 * s_depth));
  const unsigned short h1 = __builtin_bit_cast(unsigned short, (bf16)(arch >= 1 ? d1 * s_conf : 0.f));
  const unsigned short h2 = __builtin_bit_cast(unsigned short, (bf16)(arch >= 2 ? d2 * s_conf : 0.f));
  return make_uint2((unsigned)h0 | ((unsigned)h1 << 16), (unsigned)h2);
}
// PX consecutive pixels from pixel `idx`.  CP: 2 / 4 that padded channel count (one store per pixel, 16-byte stores per quad),
// anything else: `cp` channels, element by element.
template <int CP, int PX>
__device__ __forceinline__ void head_pm_store(bf16* __restrict__ draw_pm, long idx, int cp, const uint2 (&w)[PX]) {
  if constexpr (CP == 2 && PX == 4) {
    *(uint4*)(draw_pm + idx * 2) = make_uint4(w[0].x, w[1].x, w[2].x, w[3].x);
  } else if constexpr (CP == 4 && PX == 4) {
    *(uint4*)(draw_pm + idx * 4) = make_uint4(w[0].x, w[0].y, w[1].x, w[1].y);
    *(uint4*)(draw_pm + idx * 4 + 8) = make_uint4(w[2].x, w[2].y, w[3].x, w[3].y);
  } else {
#pragma unroll
    for (int q = 0; q < PX; ++q) {
      if constexpr (CP == 2) {
        *(unsigned*)(draw_pm + (idx + q) * 2) = w[q].x;
      } else if constexpr (CP == 4) {
        *(uint2*)(draw_pm + (idx + q) * 4) = w[q];
      } else {
        bf16* o = draw_pm + (idx + q) * cp;
        o[0] = __builtin_bit_cast(bf16, (unsigned short)w[q].x);
        if (cp > 1) o[1] = __builtin_bit_cast(bf16, (unsigned short)(w[q].x >> 16));
        if (cp > 2) o[2] = __builtin_bit_cast(bf16, (unsigned short)w[q].y);
        for (int c = 3; c < cp; ++c) o[c] = (bf16)0.f;
      }
    }
  }
}
