// The optimizers' arithmetic, written once: every kernel that applies Adam forms its gradient and moves its streams itself and
// calls these on registers.  Held per element to a float64 reference by tests/test_gpu_optim.py (criteria: tests/optim_ref.py).
#pragma once
#include "common.h"

// torch.optim.Adam (no weight decay / amsgrad) as configured at trainers/dcgan_amp.py:116-125 with the bias corrections folded
// into two factors, lr_bc1 = lr / (1 - b1^t) and inv_sqrt_bc2 = 1 / sqrt(1 - b2^t), and ema_inplace (:30-35) behind it
struct AdamCoef { float lr_bc1, inv_sqrt_bc2, b2, eps, ema_decay; };

// the factors at step t = *stepp + 1 from a step count in device memory (graph replay)
__device__ __forceinline__ float adam_step_t(const unsigned long long* stepp) { return (float)(*stepp + 1ull); }
__device__ __forceinline__ float adam_inv_sqrt_bc2(float b2, float t) { return rsqrtf(1.f - powf(b2, t)); }
__device__ __forceinline__ float adam_lr_bc1(float lr, float b1, float t) { return lr / (1.f - (b1 > 0.f ? powf(b1, t) : 0.f)); }

//   v <- b2 v + (1-b2) g^2 ; p <- p - lr_bc1 mi / (sqrt(v) inv_sqrt_bc2 + eps) ; e <- d e + (1-d) p
// mi is the new first moment: b1 m + (1-b1) g formed by the caller, or g itself where beta1 = 0 (exp_avg IS the gradient)
__device__ __forceinline__ void adam_ema_apply(float mi, float g, float& v, float& p, float& e, const AdamCoef& c) {
  const float vi = c.b2 * v + (1.f - c.b2) * g * g;
  v = vi;
  p = p - c.lr_bc1 * (mi / (sqrtf(vi) * c.inv_sqrt_bc2 + c.eps));
  e = c.ema_decay * e + (1.f - c.ema_decay) * p;
}

// four consecutive updated parameters -> dst[i .. i + 3] of the ST-typed shadow the conv kernels read, as one 8- or 16-byte
// store per lane (four 2-byte stores were a quarter of adam_ema_kernel's store instructions)
template <typename ST>
__device__ __forceinline__ void shadow_store4(ST* dst, long i, const float (&x)[4]) {
  if constexpr (sizeof(ST) == 2) {
    const ST h[4] = {(ST)x[0], (ST)x[1], (ST)x[2], (ST)x[3]};
    uint2 pk;
    pk.x = (unsigned)__builtin_bit_cast(unsigned short, h[0]) | ((unsigned)__builtin_bit_cast(unsigned short, h[1]) << 16);
    pk.y = (unsigned)__builtin_bit_cast(unsigned short, h[2]) | ((unsigned)__builtin_bit_cast(unsigned short, h[3]) << 16);
    *(uint2*)(dst + i) = pk;
  } else {
    *(float4*)(dst + i) = make_float4(x[0], x[1], x[2], x[3]);
  }
}

// torch.optim.Adam's single-tensor form (defaults), as the inversion optimizers step their latents and blend weights, with
// w1 = 1 - beta1, w2 = 1 - beta2 and, from a host-made table, step_size = lr / (1 - beta1^t) and bc2s = sqrt(1 - beta2^t).
// m and v are the state elements themselves: written before x is formed, as torch does
__device__ __forceinline__ void adam_torch_apply(float g, float& m, float& v, float& x, float step_size, float bc2s, float w1,
                                                 float beta2, float w2, float eps) {
  const float mi = m + w1 * (g - m);          // exp_avg.lerp_(grad, 1 - beta1)
  const float vi = v * beta2 + w2 * g * g;    // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
  m = mi;
  v = vi;
  x = x - step_size * (mi / (sqrtf(vi) / bc2s + eps));
}
