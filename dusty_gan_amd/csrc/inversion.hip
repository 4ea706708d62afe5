// GAN inversion (reference: evaluate_reconstruction.py:32-164 with utils/__init__.py:224-246), gfx950:
//   * inv_loss_grad_kernel : the masked L1 / L2 loss between the reference inverse depth and tanh_to_sigmoid of the head's
//                            depth channel, per sample, and in the same pass its gradient w.r.t. the head's depth
//                            pre-activation in the layout dg_head_post_bwd writes (planar fp32 `draw` and / or the
//                            pixel-major bf16 `draw_pm`), confidence channels zero: the generator's backward-data chain
//                            runs unchanged below it.
//   * sphere_adam_kernel   : SphericalOptimizer.step (Adam, then every latent row renormalised to unit RMS) with the
//                            LambdaLR schedule looked up by the step index in device memory, plus the NEXT step's
//                            perturbed latent written straight into the generator's compute-dtype latent buffer.
//   * depth_metrics_kernel : compute_depth_error / compute_depth_accuracy (utils/metrics/depth.py) on revert_depth of both
//                            inverse-depth maps, and the drop ratios of the evaluation CSV.
//   * inv_chamfer_scatter_kernel / inv_chamfer_grad_kernel : the Chamfer term of the reference's inversion loop (demo.py:508-519
//                            with chamfer_distance.cpp:82-140): the target-to-generated matches of dg_chamfer_nn scattered
//                            onto the generated pixels in 24.40 fixed point, then per sample the loss and, chained through
//                            inv_to_xyz and the EVAL-mode head post-processing, the head gradient.
//   * points_gather_kernel / inv_points_grad_kernel : the earth mover's term on K furthest-point-sampled rays of the target:
//                            the generated points read at the sampled pixels (the cloud dg_emd_grad matches against the
//                            target's sample), and dg_emd_grad's gradA taken from those K pixels through the same pixel chain
//                            (inv_chain.h) into the head gradient.
// Every per-sample sum is a fixed-order reduction (block sums, then the partials of a sample in chunk order): an inversion
// is bit-reproducible run to run.
#include "adam.h"
#include "head_post.h"
#include "inv_chain.h"

namespace {

constexpr int IL_THREADS = 256;

// gen = tanh_to_sigmoid(t) (from_tanh) or x; l1: |ref - gen|, l2: (ref - gen)^2, both times the mask.
// d loss_b / d gen = sign(gen - ref) (sign(0) = 0, torch's l1_loss gradient) or 2 (gen - ref), times mask / msum_b;
// through tanh_to_sigmoid (1/2) and tanh (1 - t^2), times the head's EqualLR scale.
// ADD: a further term of the loss (its own instantiation: the single-term kernel is the code it was)
template <bool ADD>
__global__ __launch_bounds__(IL_THREADS) void inv_loss_grad_kernel(const float* __restrict__ gen, int gen_sb, int from_tanh,
                                                                   const float* __restrict__ ref, const float* __restrict__ mask,
                                                                   const float* __restrict__ msum, int l2, long HW,
                                                                   float s_depth, float* __restrict__ draw, int nheads,
                                                                   bf16* __restrict__ draw_pm, int cp, float* __restrict__ parts,
                                                                   unsigned* __restrict__ tickets, float* __restrict__ loss) {
  __shared__ float red[16];
  const int b = blockIdx.y, nch = gridDim.x;
  const long chunk = (HW + nch - 1) / nch;
  const long p0 = blockIdx.x * chunk, p1 = min(HW, p0 + chunk);
  const float* g = gen + (long)b * gen_sb;
  const float* r = ref + (long)b * HW;
  const float* mk = mask + (long)b * HW;
  const float inv_m = 1.f / msum[b];
  float acc = 0.f;
#pragma unroll 4
  for (long p = p0 + threadIdx.x; p < p1; p += IL_THREADS) {
    const float t = g[p];
    const float x = from_tanh ? (t + 1.f) / 2.f : t;
    const float m = mk[p];
    const float d = r[p] - x;
    acc += (l2 ? d * d : fabsf(d)) * m;
    if (draw || draw_pm) {
      const float e = x - r[p];
      const float dl = (l2 ? 2.f * e : (float)((e > 0.f) - (e < 0.f))) * (m * inv_m);
      const float d0 = dl * 0.5f * (1.f - t * t) * s_depth;
      if constexpr (ADD) {   // a further term of the loss: the planar fp32 gradient is the running sum, the bf16 copy its rounding
        float* q = draw + (long)b * nheads * HW + p;
        const float v0 = q[0] + d0;
        q[0] = v0;
        if (draw_pm) {
          bf16* o = draw_pm + ((long)b * HW + p) * cp;
          o[0] = (bf16)v0;
          for (int c = 1; c < cp; ++c) o[c] = (bf16)(c < nheads ? q[c * HW] : 0.f);
        }
        continue;
      }
      if (draw) {
        float* q = draw + (long)b * nheads * HW + p;
        q[0] = d0;
        for (int c = 1; c < nheads; ++c) q[c * HW] = 0.f;
      }
      if (draw_pm) {
        bf16* q = draw_pm + ((long)b * HW + p) * cp;
        q[0] = (bf16)d0;
        for (int c = 1; c < cp; ++c) q[c] = (bf16)0.f;
      }
    }
  }
  const float s = dg_block_sum(acc, red);
  if (threadIdx.x != 0) return;
  if (nch == 1) {
    loss[b] = ADD ? loss[b] + s / msum[b] : s / msum[b];
    return;
  }
  // the partial goes to memory-side (atomic exchange); the last block of the sample adds the partials in chunk order
  atomicExch(&parts[(long)b * nch + blockIdx.x], s);
  if (!dg_ticket_last(&tickets[b], nch)) return;
  float tot = 0.f;
  for (int c = 0; c < nch; ++c) tot += atomicExch(&parts[(long)b * nch + c], 0.f);
  loss[b] = ADD ? loss[b] + tot / msum[b] : tot / msum[b];
}

// ---- the Chamfer term.  R [B,3,HW]: the target's points, P [B,3,HW]: postprocess(out)["points"], both planar.
// Scatter of the target-to-generated matches: acc [B,HW,4] u64 words (dg_fix40: |R| <= 1 and at most 2^18 matches per pixel keep a
// total below 2^59), word 3 the match count.  Integer atomics: the sums do not depend on the arrival order.  ZERO AT REST:
// inv_chamfer_grad_kernel zeroes what it reads.
__global__ __launch_bounds__(256) void inv_chamfer_scatter_kernel(const float* __restrict__ R, const int* __restrict__ idx1,
                                                                  int B, long HW, unsigned long long* __restrict__ acc) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * HW) return;
  const long b = i / HW, j = i - b * HW;
  const int k = idx1[i];
  if (k < 0 || k >= HW) return;
  unsigned long long* cell = acc + (b * HW + k) * 4;
#pragma unroll
  for (int c = 0; c < 3; ++c) dg_fix40_add(cell + c, (double)R[(b * 3 + c) * HW + j]);
  atomicAdd(cell + 3, 1ull);
}

struct ChamferGradArgs {
  const float *P, *R, *d1, *d2;
  const int* idx2;
  unsigned long long* acc;
  const float *depth, *angle, *gout, *noise_pixel, *mask;
  int arch, nheads, cp, add;
  float inv_tau, drop_const, min_d, max_d, tol, s_depth, s_conf;
  long HW;
  float* draw;
  bf16* draw_pm;
  float* parts;
  unsigned* tickets;
  float* loss;
};

// loss[b] (+)= mean_j d1 + mean_k d2 (N = M = HW points either side) and, per generated pixel k,
//   gP = (2/M)(P_k - R_idx2[k]) + (2/N)(c_k P_k - S_k)                       chamfer_distance.cpp:105-139
//   g  = <gP, direction> d(depth/max)/d inv * valid * 1/2                     utils/lidar.py:61-68, utils/__init__.py:168
// = d loss_b / d (masked depth); then the head gradient of the eval-mode graph (models/dusty.py:45-59,77-91,107-127): the depth
// channel through mask and tanh, the pixel confidence through the straight-through Gumbel sigmoid, dusty2's image channel 0
// (eval: a plain threshold).  add: the gradient is added to what `draw` holds (an L1 / L2 term written before).
__global__ __launch_bounds__(IL_THREADS) void inv_chamfer_grad_kernel(const ChamferGradArgs a) {
  __shared__ float red[16];
  const int b = blockIdx.y, nch = gridDim.x;
  const long HW = a.HW;
  const long chunk = (HW + nch - 1) / nch;
  const long p0 = blockIdx.x * chunk, p1 = min(HW, p0 + chunk);
  const float* Pb = a.P + (long)b * 3 * HW;
  const float* Rb = a.R + (long)b * 3 * HW;
  const float span = 1.f / a.min_d - 1.f / a.max_d;
  const float w = 2.f / (float)HW;
  float acc = 0.f;
  for (long p = p0 + threadIdx.x; p < p1; p += IL_THREADS) {
    const long bp = (long)b * HW + p;
    acc += a.d1[bp] + a.d2[bp];
    const float x = Pb[p], y = Pb[HW + p], z = Pb[2 * HW + p];
    int k2 = a.idx2[bp];
    k2 = k2 < 0 ? 0 : (k2 >= HW ? (int)(HW - 1) : k2);
    unsigned long long* cell = a.acc + bp * 4;
    const float sx = (float)dg_fix40_value((long long)cell[0]), sy = (float)dg_fix40_value((long long)cell[1]),
                sz = (float)dg_fix40_value((long long)cell[2]), cnt = (float)cell[3];
    cell[0] = 0ull; cell[1] = 0ull; cell[2] = 0ull; cell[3] = 0ull;
    const float gx = w * (x - Rb[k2]) + w * (cnt * x - sx);
    const float gy = w * (y - Rb[HW + k2]) + w * (cnt * y - sy);
    const float gz = w * (z - Rb[2 * HW + k2]) + w * (cnt * z - sz);
    inv_point_chain(a, b, p, bp, span, gx, gy, gz);
  }
  const float s = dg_block_sum(acc, red);
  if (threadIdx.x != 0) return;
  float tot = s;
  if (nch > 1) {
    atomicExch(&a.parts[(long)b * nch + blockIdx.x], s);
    if (!dg_ticket_last(&a.tickets[b], nch)) return;
    tot = 0.f;
    for (int c = 0; c < nch; ++c) tot += atomicExch(&a.parts[(long)b * nch + c], 0.f);
  }
  const float val = tot / (float)HW;
  a.loss[b] = a.add ? a.loss[b] + val : val;
}

// ---- the earth mover's term on K sampled rays.  out[b][s][c] = X[b x_sb + idx[b][s] x_sp + c x_sc] (strides as
// dg_chamfer_nn's); an index outside [0, n) gives the origin.
__global__ __launch_bounds__(256) void points_gather_kernel(const float* __restrict__ X, long x_sb, long x_sp, long x_sc, int n,
                                                            const int* __restrict__ idx, long BK, int K, float* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= BK) return;
  const long b = i / K;
  const int k = idx[i];
  const bool in = k >= 0 && k < n;
  const float* x = X + b * x_sb + (in ? k : 0) * x_sp;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[i * 3 + c] = in ? x[c * x_sc] : 0.f;
}

struct PointsGradArgs {
  const float* gP;
  const int* slot;
  const float* term;
  float scale;
  int K;
  const float *depth, *angle, *gout, *noise_pixel, *mask;
  int arch, nheads, cp, add;
  float inv_tau, drop_const, min_d, max_d, tol, s_depth, s_conf;
  long HW;
  float* draw;
  bf16* draw_pm;
  float* loss;
};

// The dense pixel pass of a term whose point gradient lives on K sampled pixels: gP [B,K,3] = d loss_b / d P at the sampled
// pixels (dg_emd_grad's gradA), slot [B,HW] the sample a pixel is (-1: none, its gP is 0), then the chain of inv_chain.h on
// EVERY pixel (one writer each).  loss[b] (+)= term[b] scale: the cost is a per-sample scalar already, so one thread writes it.
__global__ __launch_bounds__(IL_THREADS) void inv_points_grad_kernel(const PointsGradArgs a) {
  const int b = blockIdx.y, nch = gridDim.x;
  const long HW = a.HW;
  const long chunk = (HW + nch - 1) / nch;
  const long p0 = blockIdx.x * chunk, p1 = min(HW, p0 + chunk);
  const float span = 1.f / a.min_d - 1.f / a.max_d;
  for (long p = p0 + threadIdx.x; p < p1; p += IL_THREADS) {
    const long bp = (long)b * HW + p;
    const int s = a.slot[bp];
    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (s >= 0 && s < a.K) {
      const float* q = a.gP + ((long)b * a.K + s) * 3;
      gx = q[0]; gy = q[1]; gz = q[2];
    }
    inv_point_chain(a, b, p, bp, span, gx, gy, gz);
  }
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const float val = __fmul_rn(a.term[b], a.scale);   // (rounded on its own: the sum below is prior + val exactly)
  a.loss[b] = a.add ? a.loss[b] + val : val;
}

constexpr int SA_THREADS = 256;
constexpr int SA_PER = 4;  // latent elements per thread: nz <= 1024

// standard normal of latent element (b, j) for step k: Box-Muller on the Philox words of counter
// (k ceil(nz / 4) + j / 4, stream | b << 32) - the same word pairing as dg_philox_fill's kind 1, one counter stream per row
// (a row draws the same perturbations whatever batch it is inverted in)
__device__ __forceinline__ float latent_normal(uint64_t seed, uint64_t stream, int k, int b, int j, int nz) {
  uint32_t r[4];
  const uint64_t n4 = (uint64_t)(nz + 3) / 4;
  philox4x32_10(seed, (uint64_t)k * n4 + (uint64_t)(j >> 2), stream | ((uint64_t)b << 32), r);
  const float s24 = 1.f / 16777216.f;
  const int a = j & 2;
  const float u1 = 1.f - (float)(r[a] >> 8) * s24, u2 = (float)(r[a + 1] >> 8) * s24;
  const float rad = sqrtf(-2.f * logf(u1));
  return (j & 1) ? rad * sinf(6.283185307179586f * u2) : rad * cosf(6.283185307179586f * u2);
}

struct SphereArgs {
  const float* grad; long g_sb, g_sk;
  float *latent, *m, *v;
  unsigned long long* step;
  unsigned* ticket;
  const float* noise_in;
  void* zT; int z_bf16;
  int B, nz;
  const float* sched;   // [num_step + 1][3]: Adam's step size and sqrt(bias correction 2) at step k, noise strength of step k
  float beta1, beta2, eps;
  int num_step;
  int perturb;
  uint64_t seed, stream;
  int prime;
  int row0;   // the perturbation's row key of row 0 (dg_sphere_adam_rows: a scan's dataset index; 0 otherwise)
};

__global__ __launch_bounds__(SA_THREADS) void sphere_adam_kernel(SphereArgs a) {
  __shared__ float red[16];
  __shared__ float s_scale;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int k = (int)*(volatile unsigned long long*)a.step;
  float* p = a.latent + (long)b * a.nz;
  float x[SA_PER];
#pragma unroll
  for (int e = 0; e < SA_PER; ++e) {
    const int j = tid + e * SA_THREADS;
    x[e] = j < a.nz ? p[j] : 0.f;
  }
  int kz = k;   // the step whose perturbed latent is written below
  // the step's scalars from the host's table (evaluate_reconstruction.py:72-77,100-104; formed as torch's Adam forms them):
  // Adam at step count k + 1 with lr = base lr * lr_lambda(k); row num_step (lr 0, no noise) for a replay past the last step
  const float* sk = a.sched + 3 * min(k, a.num_step);
  const float str = a.sched[3 * min(a.prime ? k : k + 1, a.num_step) + 2];
  if (!a.prime) {
    const float step_size = sk[0], bc2s = sk[1];
    const float w1 = 1.f - a.beta1, w2 = 1.f - a.beta2;
    float* m = a.m + (long)b * a.nz;
    float* v = a.v + (long)b * a.nz;
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < SA_PER; ++e) {
      const int j = tid + e * SA_THREADS;
      if (j >= a.nz) break;
      const float g = a.grad[(long)b * a.g_sb + (long)j * a.g_sk];
      adam_torch_apply(g, m[j], v[j], x[e], step_size, bc2s, w1, a.beta2, w2, a.eps);
      ss += x[e] * x[e];
    }
    // SphericalOptimizer (utils/__init__.py:229-234): row / sqrt(mean(row^2) + 1e-9), one fixed-order block sum
    const float tot = dg_block_sum(ss, red);
    if (tid == 0) s_scale = sqrtf(tot / (float)a.nz + 1e-9f);
    __syncthreads();
    const float sc = s_scale;
#pragma unroll
    for (int e = 0; e < SA_PER; ++e) {
      const int j = tid + e * SA_THREADS;
      if (j < a.nz) {
        x[e] = x[e] / sc;
        p[j] = x[e];
      }
    }
    kz = k + 1;
  }
  // the generator's input of step kz: latent + 0.05 sigma w^2 randn (or the injected noise), in the compute dtype
#pragma unroll
  for (int e = 0; e < SA_PER; ++e) {
    const int j = tid + e * SA_THREADS;
    if (j >= a.nz) break;
    float z = x[e];
    if (a.perturb) {
      const float n = a.noise_in ? a.noise_in[(long)b * a.nz + j]
                                 : str * latent_normal(a.seed, a.stream, kz, a.row0 + b, j, a.nz);
      z = z + n;
    }
    if (a.z_bf16) ((bf16*)a.zT)[(long)b * a.nz + j] = (bf16)z;
    else ((float*)a.zT)[(long)b * a.nz + j] = z;
  }
  if (a.prime) return;
  // the step index advances once every row has read it: the last row's workgroup to finish (ticket) adds one
  if (tid == 0 && dg_ticket_last(a.ticket, a.B)) atomicAdd(a.step, 1ull);
}

constexpr int DM_THREADS = 1024;

__device__ __forceinline__ float revert_depth(float inv, float lo, float span) {
  return 1.f / (inv * span + lo);   // Coordinate.revert_depth(norm = False), utils/lidar.py:38-47
}

// one workgroup per sample.  out[b][0..8] = abs_rel, sq_rel, rmse, rmse_log, accuracy_1..3, drop_gen, drop_ref.
// keep: the generator's keep mask [B,kc,HW] (drop_gen = sum(1 - keep) / HW, evaluate_reconstruction.py:140-142) or, with
// keep_is_depth, its depth image [B,1,HW] whose |x| > tol marks kept points (:144-146).
__global__ __launch_bounds__(DM_THREADS) void depth_metrics_kernel(const float* __restrict__ inv_ref,
                                                                   const float* __restrict__ inv_gen,
                                                                   const float* __restrict__ mask,
                                                                   const float* __restrict__ keep, int kc, int keep_is_depth,
                                                                   float tol, long HW, float min_depth, float max_depth,
                                                                   float* __restrict__ out) {
  __shared__ float red[16];
  const int b = blockIdx.x;
  const bool rev = max_depth > 0.f;   // else the maps are depths already
  const float lo = rev ? 1.f / max_depth : 0.f, span = rev ? 1.f / min_depth - 1.f / max_depth : 0.f;
  float s[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const float* ir = inv_ref + (long)b * HW;
  const float* ig = inv_gen + (long)b * HW;
  const float* mk = mask + (long)b * HW;
  for (long p = threadIdx.x; p < HW; p += DM_THREADS) {
    const float dr = rev ? revert_depth(ir[p], lo, span) : ir[p], dg = rev ? revert_depth(ig[p], lo, span) : ig[p];
    const float m = mk[p];
    const float d = dr - dg;
    s[0] += fabsf(d) / dr * m;
    s[1] += d * d / dr * m;
    s[2] += d * d * m;
    const float dl = logf(dr) - logf(dg);
    s[3] += dl * dl * m;
    const float delta = fmaxf(dr / dg, dg / dr);
    s[4] += (delta < 1.25f ? 1.f : 0.f) * m;
    s[5] += (delta < 1.5625f ? 1.f : 0.f) * m;
    s[6] += (delta < 1.953125f ? 1.f : 0.f) * m;
    s[7] += m;
    s[8] += 1.f - m;
    if (keep_is_depth) {
      s[9] += fabsf(keep[(long)b * HW + p]) > tol ? 0.f : 1.f;
    } else {
      for (int c = 0; c < kc; ++c) s[9] += 1.f - keep[((long)b * kc + c) * HW + p];
    }
  }
  float t[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) t[i] = dg_block_sum(s[i], red);
  if (threadIdx.x != 0) return;
  float* o = out + (long)b * 9;
  const float ms = t[7];
  o[0] = t[0] / ms;
  o[1] = t[1] / ms;
  o[2] = sqrtf(t[2] / ms);
  o[3] = sqrtf(t[3] / ms);
  o[4] = t[4] / ms;
  o[5] = t[5] / ms;
  o[6] = t[6] / ms;
  o[7] = t[9] / (float)HW;
  o[8] = t[8] / (float)HW;
}

}  // namespace

extern "C" {

static int inv_loss_grad_launch(const float* gen, long gen_sb, int from_tanh, const float* ref, const float* mask,
                                const float* msum, int distance, int B, long HW, float s_depth, float* draw, int nheads,
                                void* draw_pm, int cp, float* parts, unsigned* tickets, int nchunk, float* loss, int add,
                                void* s_) {
  if (!gen || !ref || !mask || !msum || !loss || B <= 0 || HW <= 0 || (distance != 0 && distance != 1)) return DG_EINVAL;
  if (draw && nheads < 1) return DG_EINVAL;
  if (draw_pm && cp < 1) return DG_EINVAL;
  if (nchunk < 1 || nchunk > 65535 || B > 65535) return DG_EINVAL;
  if (nchunk > 1 && (!parts || !tickets)) return DG_EINVAL;
  if (gen_sb > 0x7fffffffL) return DG_EUNSUPPORTED;
  const dim3 grid(nchunk, B);
  if (add)
    inv_loss_grad_kernel<true><<<grid, IL_THREADS, 0, (hipStream_t)s_>>>(gen, (int)gen_sb, from_tanh, ref, mask, msum, distance,
                                                                         HW, s_depth, draw, nheads, (bf16*)draw_pm, cp, parts,
                                                                         tickets, loss);
  else
    inv_loss_grad_kernel<false><<<grid, IL_THREADS, 0, (hipStream_t)s_>>>(gen, (int)gen_sb, from_tanh, ref, mask, msum, distance,
                                                                          HW, s_depth, draw, nheads, (bf16*)draw_pm, cp, parts,
                                                                          tickets, loss);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_inv_loss_grad(const float* gen, long gen_sb, int from_tanh, const float* ref, const float* mask, const float* msum,
                     int distance, int B, long HW, float s_depth, float* draw, int nheads, void* draw_pm, int cp,
                     float* parts, unsigned* tickets, int nchunk, float* loss, void* s_) {
  return inv_loss_grad_launch(gen, gen_sb, from_tanh, ref, mask, msum, distance, B, HW, s_depth, draw, nheads, draw_pm, cp,
                              parts, tickets, nchunk, loss, 0, s_);
}

int dg_inv_loss_grad_add(const float* gen, long gen_sb, int from_tanh, const float* ref, const float* mask, const float* msum,
                         int distance, int B, long HW, float s_depth, float* draw, int nheads, void* draw_pm, int cp,
                         float* parts, unsigned* tickets, int nchunk, float* loss, void* s_) {
  if (!draw) return DG_EINVAL;   // the running sum lives in the planar gradient
  return inv_loss_grad_launch(gen, gen_sb, from_tanh, ref, mask, msum, distance, B, HW, s_depth, draw, nheads, draw_pm, cp,
                              parts, tickets, nchunk, loss, 1, s_);
}

int dg_inv_chamfer_scatter(const float* R, const int* idx1, int B, long HW, unsigned long long* acc, void* s_) {
  if (!R || !idx1 || !acc || B <= 0 || HW <= 0) return DG_EINVAL;
  if (HW > DG_FIX40_MAX_TERMS) return DG_EUNSUPPORTED;
  const long n = (long)B * HW;
  inv_chamfer_scatter_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)s_>>>(R, idx1, B, HW, acc);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_inv_chamfer_grad(const float* P, const float* R, const float* d1, const float* d2, const int* idx2,
                        unsigned long long* acc, const float* depth, const float* angle, const float* gout,
                        const float* noise_pixel, const float* mask, int arch, float tau, float drop_const, float min_depth,
                        float max_depth, float tol, int B, long HW, float s_depth, float s_conf, int add, float* draw,
                        int nheads, void* draw_pm, int cp, float* parts, unsigned* tickets, int nchunk, float* loss,
                        void* s_) {
  if (!P || !R || !d1 || !d2 || !idx2 || !acc || !depth || !angle || !gout || !loss || B <= 0 || HW <= 0) return DG_EINVAL;
  if (arch < 0 || arch > 2 || nheads != arch + 1 || (arch && (!noise_pixel || !mask)) || !(tau > 0.f)) return DG_EINVAL;
  if (!(min_depth > 0.f && min_depth < max_depth)) return DG_EINVAL;
  if (!draw && !draw_pm) return DG_EINVAL;
  if (add && !draw) return DG_EINVAL;
  if (draw_pm && cp < nheads) return DG_EINVAL;
  if (nchunk < 1 || nchunk > 65535 || B > 65535) return DG_EINVAL;
  if (nchunk > 1 && (!parts || !tickets)) return DG_EINVAL;
  if (HW > DG_FIX40_MAX_TERMS) return DG_EUNSUPPORTED;
  ChamferGradArgs a;
  a.P = P; a.R = R; a.d1 = d1; a.d2 = d2; a.idx2 = idx2; a.acc = acc; a.depth = depth; a.angle = angle; a.gout = gout;
  a.noise_pixel = noise_pixel; a.mask = mask; a.arch = arch; a.nheads = nheads; a.cp = cp; a.add = add;
  a.inv_tau = 1.f / tau; a.drop_const = drop_const; a.min_d = min_depth; a.max_d = max_depth; a.tol = tol;
  a.s_depth = s_depth; a.s_conf = s_conf; a.HW = HW; a.draw = draw; a.draw_pm = (bf16*)draw_pm; a.parts = parts;
  a.tickets = tickets; a.loss = loss;
  inv_chamfer_grad_kernel<<<dim3(nchunk, B), IL_THREADS, 0, (hipStream_t)s_>>>(a);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_points_gather(const float* X, long x_sb, long x_sp, long x_sc, int n, const int* idx, int B, int K, float* out,
                     void* s_) {
  if (!X || !idx || !out || n <= 0 || B <= 0 || K <= 0 || x_sb < 0 || x_sp <= 0 || x_sc <= 0) return DG_EINVAL;
  const long BK = (long)B * K;
  if ((BK + 255) / 256 > 0x7fffffffL) return DG_EUNSUPPORTED;
  points_gather_kernel<<<(unsigned)((BK + 255) / 256), 256, 0, (hipStream_t)s_>>>(X, x_sb, x_sp, x_sc, n, idx, BK, K, out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_inv_points_grad(const float* gP, const int* slot, const float* term, float scale, int K, const float* depth,
                       const float* angle, const float* gout, const float* noise_pixel, const float* mask, int arch, float tau,
                       float drop_const, float min_depth, float max_depth, float tol, int B, long HW, float s_depth, float s_conf,
                       int add, float* draw, int nheads, void* draw_pm, int cp, int nchunk, float* loss, void* s_) {
  if (!gP || !slot || !term || !depth || !angle || !gout || !loss || B <= 0 || HW <= 0 || K <= 0) return DG_EINVAL;
  if (arch < 0 || arch > 2 || nheads != arch + 1 || (arch && (!noise_pixel || !mask)) || !(tau > 0.f)) return DG_EINVAL;
  if (!(min_depth > 0.f && min_depth < max_depth)) return DG_EINVAL;
  if (!draw && !draw_pm) return DG_EINVAL;
  if (add && !draw) return DG_EINVAL;
  if (draw_pm && cp < nheads) return DG_EINVAL;
  if (nchunk < 1 || nchunk > 65535 || B > 65535) return DG_EINVAL;
  PointsGradArgs a;
  a.gP = gP; a.slot = slot; a.term = term; a.scale = scale; a.K = K; a.depth = depth; a.angle = angle; a.gout = gout;
  a.noise_pixel = noise_pixel; a.mask = mask; a.arch = arch; a.nheads = nheads; a.cp = cp; a.add = add;
  a.inv_tau = 1.f / tau; a.drop_const = drop_const; a.min_d = min_depth; a.max_d = max_depth; a.tol = tol;
  a.s_depth = s_depth; a.s_conf = s_conf; a.HW = HW; a.draw = draw; a.draw_pm = (bf16*)draw_pm; a.loss = loss;
  inv_points_grad_kernel<<<dim3(nchunk, B), IL_THREADS, 0, (hipStream_t)s_>>>(a);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

// row b's perturbation is keyed as row row0 + b (dg_sphere_adam: row0 = 0)
int dg_sphere_adam_rows(const float* grad, long g_sb, long g_sk, float* latent, float* m, float* v, unsigned long long* step_dev,
                        unsigned* ticket, const float* noise_in, void* zT, int z_dtype, int B, int nz, const float* sched,
                        int num_step, float beta1, float beta2, float eps, int perturb, uint64_t seed, uint64_t stream_id,
                        int prime, int row0, void* s_) {
  if (row0 < 0 || !latent || !step_dev || !zT || !sched || B <= 0 || nz <= 0 || num_step <= 0) return DG_EINVAL;
  if (!prime && (!grad || !m || !v || !ticket)) return DG_EINVAL;
  if (z_dtype != DG_F32 && z_dtype != DG_BF16) return DG_EINVAL;
  if (nz > SA_THREADS * SA_PER) return DG_EUNSUPPORTED;
  SphereArgs a;
  a.grad = grad; a.g_sb = g_sb; a.g_sk = g_sk;
  a.latent = latent; a.m = m; a.v = v; a.step = step_dev; a.ticket = ticket; a.noise_in = noise_in;
  a.zT = zT; a.z_bf16 = z_dtype == DG_BF16; a.B = B; a.nz = nz;
  a.sched = sched; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.num_step = num_step;
  a.perturb = perturb; a.seed = seed; a.stream = stream_id; a.prime = prime; a.row0 = row0;
  sphere_adam_kernel<<<B, SA_THREADS, 0, (hipStream_t)s_>>>(a);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_sphere_adam(const float* grad, long g_sb, long g_sk, float* latent, float* m, float* v, unsigned long long* step_dev,
                   unsigned* ticket, const float* noise_in, void* zT, int z_dtype, int B, int nz, const float* sched,
                   int num_step, float beta1, float beta2, float eps, int perturb, uint64_t seed, uint64_t stream_id, int prime,
                   void* s_) {
  return dg_sphere_adam_rows(grad, g_sb, g_sk, latent, m, v, step_dev, ticket, noise_in, zT, z_dtype, B, nz, sched, num_step, beta1,
                             beta2, eps, perturb, seed, stream_id, prime, 0, s_);
}

int dg_depth_metrics(const float* inv_ref, const float* inv_gen, const float* mask, const float* keep, int kc,
                     int keep_is_depth, float tol, int B, long HW, float min_depth, float max_depth, float* out, void* s_) {
  if (!inv_ref || !inv_gen || !mask || !keep || !out || B <= 0 || HW <= 0) return DG_EINVAL;
  if (max_depth > 0.f && !(min_depth > 0.f && min_depth < max_depth)) return DG_EINVAL;
  if (!keep_is_depth && kc < 1) return DG_EINVAL;
  depth_metrics_kernel<<<B, DM_THREADS, 0, (hipStream_t)s_>>>(inv_ref, inv_gen, mask, keep, kc, keep_is_depth, tol, HW,
                                                              min_depth, max_depth, out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

}  // extern "C"
