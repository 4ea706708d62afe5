// The adaptive controller of DiffAugment's probability p (StyleGAN2-ADA's rule on E[sign(D(real))]; the reference has none:
// its p is a constructor argument, utils/diff_augment.py:114-122).  ONE small launch per D phase, only when the controller is on:
// it counts the signs of the real logits in integers - two runs give the same bits whatever the order - and, every `interval`
// iterations, moves p by a fixed step towards the target.  p lives in device memory, where the step's draw reads it
// (dg_aug_draw_p_dev / DgDraw.p_dev): a captured step follows it without a host round trip.
#include "common.h"

// sign of a logit as torch.sign has it for +-0; a logit that is not finite counts as 0
__device__ __forceinline__ int ada_sign(float v) { return isfinite(v) ? (int)(v > 0.f) - (int)(v < 0.f) : 0; }

// One block.  y != nullptr: pend += {sum of sign(y[0..B)), B} and rt_slot[0] += rt_scale * (that sum / B) (a float the step's
// arena zeroed: rt_scale = 1 / micro-batches, so the slot ends as the iteration's mean of the calls' mean signs).
// advance: the iteration ends here - the window takes `pend` (which, with several ranks, the caller has summed over the ranks in
// between), steps += 1, and at steps % interval == 0:  r_t = sign_sum / count,
// p = clamp(p + sign(r_t - target) (batch_size interval) / (kimg 1000), 0, 1) in float32, in this order; the window restarts.
// p_slot[0] = p as it stands behind this call.
__global__ __launch_bounds__(256) void ada_update_kernel(const float* __restrict__ y, int B, DgAdaState* __restrict__ st,
                                                         long long* __restrict__ pend, int advance, float target, int interval,
                                                         int batch_size, float kimg, float rt_scale, float* __restrict__ rt_slot,
                                                         float* __restrict__ p_slot) {
  __shared__ int red[256];
  int acc = 0;
  if (y)
    for (int i = threadIdx.x; i < B; i += 256) acc += ada_sign(y[i]);
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  if (y) {
    pend[0] += (long long)red[0];
    pend[1] += (long long)B;
    // (three roundings, as stated: the quotient, the product, the sum - no contraction into a fused multiply-add)
    if (rt_slot) rt_slot[0] = __fadd_rn(rt_slot[0], __fmul_rn(rt_scale, (float)red[0] / (float)B));
  }
  float p = st->p;
  if (advance) {
    long long ssum = st->sign_sum + pend[0], cnt = st->count + pend[1];
    pend[0] = 0;
    pend[1] = 0;
    const int steps = st->steps + 1;
    if (steps % interval == 0) {
      const float rt = cnt > 0 ? (float)ssum / (float)cnt : target;
      const float d = rt - target;
      const float sg = (float)((int)(d > 0.f) - (int)(d < 0.f));
      const float adj = __fdiv_rn(__fmul_rn(sg, (float)(batch_size * interval)), __fmul_rn(kimg, 1000.f));
      p = fminf(fmaxf(__fadd_rn(p, adj), 0.f), 1.f);
      ssum = 0;
      cnt = 0;
    }
    st->p = p;
    st->sign_sum = ssum;
    st->count = cnt;
    st->steps = steps;
  }
  if (p_slot) p_slot[0] = p;
}

extern "C" {

int dg_ada_update(const float* y_real, int B, void* state, long long* pend, int advance, float target, int interval,
                  int batch_size, float kimg, float rt_scale, float* rt_slot, float* p_slot, void* s_) {
  if (!state || !pend || (y_real && B <= 0) || (!y_real && !advance) || interval < 1 || batch_size < 1 || !(kimg > 0.f) ||
      !(target >= -1.f && target <= 1.f) || (long)batch_size * interval > 0x7fffffffL)
    return DG_EINVAL;
  ada_update_kernel<<<1, 256, 0, (hipStream_t)s_>>>(y_real, B, (DgAdaState*)state, pend, advance, target, interval, batch_size, kimg, rt_scale,
                                                    rt_slot, p_slot);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

}  // extern "C"
