// Head post-processing (tanh + Gumbel point-drop) between the generator's head convs and the image: forward (with the
// per-sample sums DiffAugment's contrast needs), backward (from d loss / d depth, or from the BlurVH adjoint's output through
// DiffAugment's adjoint gather), and the second-order backward of the path-length penalty.  The pixel arithmetic: head_post.h.
// gout [B,1+k,H,W] planar fp32: ch0 raw depth -> tanh in place (depth_orig), ch1.. confidence logits (kept).
// arch: 0 none, 1 dusty1, 2 dusty2.  noise_pixel [B,H,W], noise_image [B]; mask [B,k,H,W] (pixel mask, image mask).
#include "head_post.h"
#include "diffaug.h"   // (HeadGradAug: DiffAugment's adjoint gather inside the backward)

// ----------------------------------------------------------------------------------------------------------
// Forward.  PX = 1: one pixel per thread; PX = 4: four consecutive pixels per thread (HW % 1024 == 0, sums wanted), 16-byte
// loads / stores of every plane.
// dsum != nullptr: dsum[b] += sum of depth[b] - the per-sample sum DiffAugment's contrast needs of its input, produced where
// the image is produced.  A block then owns `chunk` consecutive pixels of ONE sample (HW % chunk == 0) and issues one atomic:
// with one block per 256 pixels the 8192 atomics on 32 addresses cost 80 us (round 1 met the same in head_post_bwd).

// PX pixels whose head outputs are in registers: stores tanh (in place: g), the masks (m: the pixel mask's plane, the image
// mask's one plane further) and the depth; returns the pixels' depth sum
// LT (the learnable temperature, head_post.h): inv_tau is the pixel sigmoid's slope, inv_i the image sigmoid's
template <int arch, int PX, bool LT = false>
__device__ __forceinline__ float head_fwd_store(const float (&g0)[PX], const float (&g1)[PX], const float (&np)[PX],
                                                const float (&g2)[PX], float ni, int training, float inv_tau, float inv_i,
                                                float drop_const, long HW, float* __restrict__ g, float* __restrict__ m,
                                                float* __restrict__ depth) {
  float t[PX], mp[PX], mi[PX], dv[PX];
#pragma unroll
  for (int q = 0; q < PX; ++q) {
    const HeadPx o = LT ? head_px_fwd_lt<arch>(g0[q], arch >= 1 ? g1[q] + np[q] : 0.f, arch == 2 ? g2[q] : 0.f, ni, training,
                                               inv_tau, inv_i, drop_const)
                        : head_px_fwd<arch>(g0[q], arch >= 1 ? g1[q] + np[q] : 0.f, arch == 2 ? g2[q] : 0.f, ni, training,
                                            inv_tau, drop_const);
    t[q] = o.t; mp[q] = o.mp; mi[q] = o.mi; dv[q] = o.depth;
  }
  st_px<PX>(g, t);
  if (arch >= 1) st_px<PX>(m, mp);
  if (arch == 2) st_px<PX>(m + HW, mi);
  st_px<PX>(depth, dv);
  return px_sum<PX>(dv);
}

// the slopes of a launch: the by-value one, or (LT) formed from the master weights - one load per thread, uniform
template <int arch, bool LT>
__device__ __forceinline__ void head_slopes(const HeadTau<LT>& tau, float& inv_p, float& inv_i) {
  if constexpr (LT) {
    inv_p = arch >= 1 ? hp_inv_tau_lt(tau.w[0], tau.inv_min) : tau.inv_min;
    inv_i = arch == 2 ? hp_inv_tau_lt(tau.w[1], tau.inv_min) : inv_p;
  } else {
    inv_p = inv_i = tau.inv_tau;
  }
}

// compile-time: the pixel function is then straight-line code and the unrolled trips batch their loads.  LT: the learnable temperature
template <int arch, int PX, bool LT = false>
__global__ __launch_bounds__(256) void head_post_fwd_kernel(float* __restrict__ gout, const float* __restrict__ noise_pixel,
                                     const float* __restrict__ noise_image, int training, const HeadTau<LT> tau,
                                     float drop_const, int B, long HW, float* __restrict__ mask,
                                     float* __restrict__ depth, float* __restrict__ dsum, int chunk, const DgDet det) {
  __shared__ float red[16];
  constexpr int nch = 1 + arch;
  float inv_tau, inv_i;
  head_slopes<arch, LT>(tau, inv_tau, inv_i);
  // the head outputs of PX pixels: g = the first one's raw depth, np = its noise
  auto load = [&](const float* g, const float* np_, float (&g0)[PX], float (&g1)[PX], float (&np)[PX], float (&g2)[PX]) {
    ld_px<PX>(g, g0);
    if (arch >= 1) { ld_px<PX>(g + HW, g1); ld_px<PX>(np_, np); }
    if (arch == 2) ld_px<PX>(g + 2 * HW, g2);
  };
  if (PX == 1 && !dsum) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < (long)B * HW) {
      const int b = (int)(idx / HW);
      const long p = idx - (long)b * HW;
      float* g = gout + (long)b * nch * HW + p;
      float g0[PX], g1[PX], np[PX], g2[PX];
      load(g, noise_pixel + idx, g0, g1, np, g2);
      head_fwd_store<arch, PX, LT>(g0, g1, np, g2, (arch == 2 && training) ? noise_image[b] : 0.f, training, inv_tau, inv_i,
                                   drop_const, HW, g, arch >= 1 ? mask + (long)b * arch * HW + p : nullptr, depth + idx);
    }
    return;
  }
  // the block's pixels belong to ONE sample (HW % chunk == 0): the sample index is block-uniform (a 64-bit division per
  // pixel and one round trip per pixel made this 15 us for 25 MB)
  const long i0 = (long)blockIdx.x * chunk;
  const int b = (int)(i0 / HW);
  const long p0 = i0 - (long)b * HW;
  float* g = gout + (long)b * nch * HW + p0;
  float* m = arch >= 1 ? mask + (long)b * arch * HW + p0 : nullptr;   // (arch 0 has no mask: the pointer may be null)
  const float ni = (arch == 2 && training) ? noise_image[b] : 0.f;
  float acc = 0.f;
  // PX = 4: the loads of U = 4 trips issued before the first store (gout is rewritten in place: the compiler cannot hoist a
  // later trip's loads over an earlier trip's stores, and one load in flight per wave left the launch at a third of the HBM
  // rate).  PX = 1: the four pixels a thread handles per unrolled trip are independent.
  constexpr int U = PX == 4 ? 4 : 1, STEP = 256 * PX;
  auto trips = [&](int k0) {
    float g0[U][PX], g1[U][PX], np[U][PX], g2[U][PX];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + u * STEP;
      if (k < chunk) load(g + k, noise_pixel + i0 + k, g0[u], g1[u], np[u], g2[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + u * STEP;
      if (k >= chunk) break;
      acc += head_fwd_store<arch, PX, LT>(g0[u], g1[u], np[u], g2[u], ni, training, inv_tau, inv_i, drop_const, HW, g + k,
                                          m + k, depth + i0 + k);
    }
  };
  if constexpr (PX == 1) {
#pragma unroll 4
    for (int k0 = threadIdx.x; k0 < chunk; k0 += 256) trips(k0);
  } else {
    for (int k0 = threadIdx.x * PX; k0 < chunk; k0 += U * STEP) trips(k0);
  }
  const float sblk = dg_block_sum(acc, red);
  if (threadIdx.x == 0) dg_acc_add(&dsum[b], sblk, (unsigned)(HW / chunk), det);
}

// ----------------------------------------------------------------------------------------------------------
// Backward of the above: d loss / d depth [B,H,W] -> draw [B,1+k,H,W] planar (gradient w.r.t. the head conv outputs, times
// the heads' EqualLR scales), its pixel-major bf16 copy draw_pm, and the head-bias gradient sums.
// Where d loss / d depth of PX pixels comes from: the tensor itself, or - HeadGradAug, diffaug.h - DiffAugment's adjoint
// gather applied on the fly to the BlurVH adjoint's output.
struct HeadGradPlain {
  const float* ddepth;
  template <int PX>
  __device__ __forceinline__ void operator()(int b, long p, long HW, float (&go)[PX]) const { ld_px<PX>(ddepth + (long)b * HW + p, go); }
};

// grid = (blocks per sample, B): blockIdx.y = sample (no 64-bit division per pixel), grid-stride over the sample so that
// the bias-gradient sums cost one atomic per block per head (one pixel per thread meant 8192 atomics on the same address:
// 100 us of the 108 us this kernel took at B = 32); straight-line body (arch and the copy's layout are compile-time).
// PX = 1: any HW and any padded channel count (CP = 1: `cp`), planar copy mandatory, four independent pixels per unrolled
// trip, plain float atomics into dbias.
// PX = 4: four consecutive pixels per thread (HW % 4 == 0): 16-byte loads of every plane, 16-byte stores; `draw` may be
// null - the bf16 path consumes only the pixel-major copy, and three 8 MB planes were written for nobody.
// LT: the learnable temperature (head_post.h) - the slopes come from the master weights, and the two temperature sums G_pixel,
// G_image travel exactly as the head-bias sums do (block sum; then the fixed-point slots and tickets, or float atomics) into
// tau.dw[k] += sigma(w_k) G_k, the factor applied once where the total is converted.  The launch sums them with or without dbias.
template <int arch, int CP, int PX, typename DD, bool LT = false>   // CP: 0 no pixel-major copy, 2 / 4 that padded channel count, 1 any other
__global__ __launch_bounds__(256) void head_post_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ noise_pixel,
                                     const float* __restrict__ noise_image, const float* __restrict__ mask,
                                     DD ddepth, const HeadTau<LT> tau, float drop_const, int B, long HW,
                                     float s_depth, float s_conf, float* __restrict__ draw, float* __restrict__ dbias,
                                     bf16* __restrict__ draw_pm, int cp, float* __restrict__ bias_ws) {
  __shared__ float red[16];
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  float at1 = 0.f, at2 = 0.f;   // (LT) this thread's part of G_pixel, G_image
  float inv_tau, inv_i;
  head_slopes<arch, LT>(tau, inv_tau, inv_i);
  const int b = blockIdx.y;
  constexpr int nch = 1 + arch;
  const float* g = gout + (long)b * nch * HW;
  const float* mk = arch >= 1 ? mask + (long)b * arch * HW : nullptr;
  const float ni = arch == 2 ? noise_image[b] : 0.f;
  auto pixels = [&](long p) {
    const long idx = (long)b * HW + p;
    float t[PX], go[PX], g1[PX], np[PX], g2[PX], mp[PX], mi[PX];
    ld_px<PX>(g + p, t);
    ddepth.template operator()<PX>(b, p, HW, go);
    if (arch >= 1) { ld_px<PX>(g + HW + p, g1); ld_px<PX>(noise_pixel + idx, np); ld_px<PX>(mk + p, mp); }
    if (arch == 2) { ld_px<PX>(mk + HW + p, mi); ld_px<PX>(g + 2 * HW + p, g2); }
    float d0[PX], d1[PX], d2[PX];   // unscaled gradients w.r.t. the head outputs (= the head bias gradients)
    if constexpr (LT) {
      float e1[PX], e2[PX];
#pragma unroll
      for (int q = 0; q < PX; ++q)
        head_px_bwd_lt<arch>(t[q], go[q], arch >= 1 ? g1[q] + np[q] : 0.f, arch == 2 ? g2[q] + ni : 0.f, arch >= 1 ? mp[q] : 1.f,
                             arch == 2 ? mi[q] : 1.f, inv_tau, inv_i, drop_const, d0[q], d1[q], d2[q], e1[q], e2[q]);
      at1 += px_sum<PX>(e1); at2 += px_sum<PX>(e2);
    } else {
#pragma unroll
      for (int q = 0; q < PX; ++q)
        head_px_bwd<arch>(t[q], go[q], arch >= 1 ? g1[q] + np[q] : 0.f, arch == 2 ? g2[q] + ni : 0.f, arch >= 1 ? mp[q] : 1.f,
                          arch == 2 ? mi[q] : 1.f, inv_tau, drop_const, d0[q], d1[q], d2[q]);
    }
    if (PX == 1 || draw) {
      float* d = draw + (long)b * nch * HW + p;
      float v[PX];
#pragma unroll
      for (int q = 0; q < PX; ++q) v[q] = d0[q] * s_depth;
      st_px<PX>(d, v);
      if (arch >= 1) {
#pragma unroll
        for (int q = 0; q < PX; ++q) v[q] = d1[q] * s_conf;
        st_px<PX>(d + HW, v);
      }
      if (arch == 2) {
#pragma unroll
        for (int q = 0; q < PX; ++q) v[q] = d2[q] * s_conf;
        st_px<PX>(d + 2 * HW, v);
      }
    }
    if (CP != 0) {
      uint2 w[PX];
#pragma unroll
      for (int q = 0; q < PX; ++q) w[q] = head_pm_words(arch, d0[q], d1[q], d2[q], s_depth, s_conf);
      head_pm_store<CP, PX>(draw_pm, idx, cp, w);
    }
    a0 += px_sum<PX>(d0); a1 += px_sum<PX>(d1); a2 += px_sum<PX>(d2);
  };
  const long p_first = ((long)blockIdx.x * blockDim.x + threadIdx.x) * PX, p_step = (long)gridDim.x * blockDim.x * PX;
  if constexpr (PX == 1) {
#pragma unroll 4
    for (long p = p_first; p < HW; p += p_step) pixels(p);
  } else {
    for (long p = p_first; p < HW; p += p_step) pixels(p);
  }
  if (LT || dbias) {  // head biases are outside EqualLR's input scaling: their gradient is the unscaled sum
    // Atomics on ONE address retire at ~10 ns each (they execute memory-side): a thousand blocks adding straight into
    // dbias[n] cost 10 us per head - more than the pass over the data.  With `bias_ws` (PX = 4; 4 KB per sample, zero on entry
    // and left zero) the blocks of a sample add into that sample's slot - B independent addresses - and the last one to
    // arrive (a ticket in the slot) folds the slot into dbias: gridDim.x adds per slot, B per dbias[n].
    const float s0 = dg_block_sum(a0, red);
    const float s1 = arch >= 1 ? dg_block_sum(a1, red) : 0.f;
    const float s2 = arch >= 2 ? dg_block_sum(a2, red) : 0.f;
    const float st1 = (LT && arch >= 1) ? dg_block_sum(at1, red) : 0.f;
    const float st2 = (LT && arch >= 2) ? dg_block_sum(at2, red) : 0.f;
    const bool heads = !LT || dbias;   // (LT: the temperature sums do not wait for a dbias)
    // (LT) adds sigma(w_k) v onto the gradient of temperature weight k
    auto dtau_add = [&](int k, float v) {
      if constexpr (LT) atomicAdd(&tau.dw[k], hp_dinv_tau_lt(tau.w[k]) * v);
    };
    if (threadIdx.x == 0) {
      if (PX == 4 && bias_ws && gridDim.x > 1) {
        // Round 5: the staged sums are 32.32 FIXED POINT (integer adds commute: the total no longer depends on the order in
        // which blocks and samples arrive - common.h has the protocol and its argument).  Two levels, as before: the blocks of a
        // sample add into that sample's slot; the last block of a sample (ticket) moves the slot's totals, still integers,
        // into the launch's accumulators (upper half of slot 0) and takes a second ticket; the last SAMPLE converts and adds
        // each head's total to dbias once.  Everything is left zero.
        unsigned long long* w = (unsigned long long*)(bias_ws + (long)b * DG_BIAS_WS_SAMPLE_FLOATS);
        unsigned long long* gacc = (unsigned long long*)(bias_ws + DG_BIAS_WS_ACC);
        const float sv[3] = {s0, s1, s2};
        if (heads) {
#pragma unroll
          for (int h = 0; h <= arch; ++h) {
            long long q;
            if (dg_fix1(sv[h], q)) atomicAdd(&w[h], (unsigned long long)q);
            else atomicAdd(&dbias[h], sv[h]);
          }
        }
        if constexpr (LT) {   // the temperature sums: words DG_BIAS_WS_TAU, + 1 of the same slots, the same two tickets
          const float tv[2] = {st1, st2};
#pragma unroll
          for (int k = 0; k < arch; ++k) {
            long long q;
            if (dg_fix1(tv[k], q)) atomicAdd(&w[DG_BIAS_WS_TAU + k], (unsigned long long)q);
            else dtau_add(k, tv[k]);
          }
        }
        if (dg_ticket_last(dg_bias_ws_ticket(w), gridDim.x)) {
          if (heads) {
#pragma unroll
            for (int h = 0; h <= arch; ++h) atomicAdd(&gacc[h], atomicExch(&w[h], 0ull));
          }
          if constexpr (LT) {
#pragma unroll
            for (int k = 0; k < arch; ++k) atomicAdd(&gacc[DG_BIAS_WS_TAU + k], atomicExch(&w[DG_BIAS_WS_TAU + k], 0ull));
          }
          if (dg_ticket_last(dg_bias_ws_ticket(gacc), gridDim.y)) {
            if (heads) {
#pragma unroll
              for (int h = 0; h <= arch; ++h) atomicAdd(&dbias[h], dg_fix1_value((long long)atomicExch(&gacc[h], 0ull)));
            }
            if constexpr (LT) {
#pragma unroll
              for (int k = 0; k < arch; ++k) dtau_add(k, dg_fix1_value((long long)atomicExch(&gacc[DG_BIAS_WS_TAU + k], 0ull)));
            }
          }
        }
      } else {
        if (heads) {
          atomicAdd(&dbias[0], s0);
          if (arch >= 1) atomicAdd(&dbias[1], s1);
          if (arch >= 2) atomicAdd(&dbias[2], s2);
        }
        if (arch >= 1) dtau_add(0, st1);
        if (arch >= 2) dtau_add(1, st2);
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------------------
// The SECOND-order part of the head post-processing (path-length regularisation, trainers/dcgan_amp.py:268-306).  With
// x = depth output, h = the head conv outputs, y the upstream of x and th the forward-mode tangent of h along the latent
// direction v, the tangent of the first-order backward d x / d h_i * y is  y * sum_j H_ij th_j  with H the Hessian of x in h
// as autograd sees it (hard masks carry the straight-through derivative, head_post.h):
//   H00 = m (-2 t)(1 - t^2)   H01 = mi sp' (1 - t^2)   H02 = mp si' (1 - t^2)
//   H11 = (t - c) mi sp''     H12 = (t - c) sp' si'    H22 = (t - c) mp si''        (t = tanh h0, c = drop_const)
// Outputs as head_post_bwd_kernel: draw2 (scaled by the head's EqualLR scale), the pixel-major bf16 copy, and the
// head-bias gradient sums.
__global__ void head_post_bwd2_kernel(const float* __restrict__ gout, const float* __restrict__ noise_pixel,
                                      const float* __restrict__ noise_image, const float* __restrict__ mask,
                                      const float* __restrict__ ddepth, const float* __restrict__ thead, int arch,
                                      float inv_tau, float drop_const, int B, long HW, float s_depth, float s_conf,
                                      float* __restrict__ draw, float* __restrict__ dbias, bf16* __restrict__ draw_pm,
                                      int cp) {
  __shared__ float red[16];
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < (long)B * HW; idx += (long)gridDim.x * blockDim.x) {
    const int b = (int)(idx / HW);
    const long p = idx - (long)b * HW;
    const int nch = 1 + arch;
    const float* g = gout + (long)b * nch * HW + p;
    const float* th = thead + (long)b * nch * HW + p;
    float* d = draw + (long)b * nch * HW + p;
    const float t = g[0], dt = hp_dtanh(t), y = ddepth[idx];
    const float t0 = th[0];
    float d0, d1 = 0.f, d2 = 0.f;
    if (arch == 0) {
      d0 = y * (-2.f * t * dt) * t0;
    } else {
      const float sp = hp_sigmoid(g[HW] + noise_pixel[idx], inv_tau);
      const float sp1 = hp_dsigmoid(1.f, sp, inv_tau), sp2 = hp_d2sigmoid(sp, sp1, inv_tau);
      const float t1 = th[HW], tc = t - drop_const;
      if (arch == 1) {
        const float mp = mask[idx];
        d0 = y * (mp * (-2.f * t * dt) * t0 + sp1 * dt * t1);
        d1 = y * (sp1 * dt * t0 + tc * sp2 * t1);
      } else {
        const float mp = mask[(long)b * 2 * HW + p], mi = mask[(long)b * 2 * HW + HW + p];
        const float si = hp_sigmoid(g[2 * HW] + noise_image[b], inv_tau);
        const float si1 = hp_dsigmoid(1.f, si, inv_tau), si2 = hp_d2sigmoid(si, si1, inv_tau);
        const float t2 = th[2 * HW];
        d0 = y * (mp * mi * (-2.f * t * dt) * t0 + mi * sp1 * dt * t1 + mp * si1 * dt * t2);
        d1 = y * (mi * sp1 * dt * t0 + tc * mi * sp2 * t1 + tc * sp1 * si1 * t2);
        d2 = y * (mp * si1 * dt * t0 + tc * sp1 * si1 * t1 + tc * mp * si2 * t2);
        d[2 * HW] = d2 * s_conf;
      }
      d[HW] = d1 * s_conf;
    }
    d[0] = d0 * s_depth;
    if (draw_pm) {   // (its own element-wise store, cp <= 4: through head_pm_words / head_pm_store the arch-0 launch measured 5 % slower)
      bf16* q = draw_pm + idx * cp;
      q[0] = (bf16)(d0 * s_depth);
      if (cp > 1) q[1] = (bf16)(arch >= 1 ? d1 * s_conf : 0.f);
      if (cp > 2) q[2] = (bf16)(arch >= 2 ? d2 * s_conf : 0.f);
      if (cp > 3) q[3] = (bf16)0.f;
    }
    a0 += d0; a1 += d1; a2 += d2;
  }
  if (dbias) {
    const float s0 = dg_block_sum(a0, red);
    if (threadIdx.x == 0) atomicAdd(&dbias[0], s0);
    if (arch >= 1) { const float s1 = dg_block_sum(a1, red); if (threadIdx.x == 0) atomicAdd(&dbias[1], s1); }
    if (arch >= 2) { const float s2 = dg_block_sum(a2, red); if (threadIdx.x == 0) atomicAdd(&dbias[2], s2); }
  }
}

// ----------------------------------------------------------------------------------------------------------
// grid: ~1024 blocks in all, each one atomic per head
// LT: `tau` holds the learnable temperature's pointers (arch 1 / 2 only: the callers have checked)
template <int PX, typename DD, bool LT = false>
static int head_post_bwd_launch(DD dd, const float* gout, const float* noise_pixel, const float* noise_image,
                                const float* mask, int arch, const HeadTau<LT> tau, float drop_const, int B, long HW, float s_depth,
                                float s_conf, float* draw, float* dbias, void* draw_pm, int cpk, int cp, float* bias_ws,
                                hipStream_t s) {
  const unsigned per = B >= 1024 ? 1u : (unsigned)(1024 / B);
  unsigned hb = nblk(HW / PX);
  if (hb > per) hb = per;
  const dim3 grid(hb, B);
#define DG_HPB(A, C)                                                                                                     \
  head_post_bwd_kernel<A, C, PX, DD, LT><<<grid, 256, 0, s>>>(gout, noise_pixel, noise_image, mask, dd, tau, drop_const, \
                                                              B, HW, s_depth, s_conf, draw, dbias, (bf16*)draw_pm, cp, bias_ws)
#define DG_HPB_A(A)                                                                            \
  do {                                                                                         \
    if (cpk == 0) DG_HPB(A, 0); else if (cpk == 2) DG_HPB(A, 2); else if (cpk == 4) DG_HPB(A, 4); \
    else if constexpr (PX == 1) DG_HPB(A, 1);   /* (any other `cp`: the callers send it to the scalar form only) */ \
  } while (0)
  if (arch == 0) { if constexpr (!LT) DG_HPB_A(0); } else if (arch == 1) DG_HPB_A(1); else DG_HPB_A(2);
#undef DG_HPB_A
#undef DG_HPB
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

template <bool LT = false>
static int head_post_fwd_impl(float* gout, const float* noise_pixel, const float* noise_image, int arch, int training,
                              const HeadTau<LT> tau, float drop_const, int B, long HW, float* mask, float* depth, float* dsum,
                              void* s_) {
  hipStream_t s = (hipStream_t)s_;
  if (arch < 0 || arch > 2) return DG_EINVAL;
  if (dsum && HW % 256 != 0) return DG_EUNSUPPORTED;
  const int chunk = dsum ? sum_chunk(HW) : 256;
  const DgDet det = dg_det_current();
  const unsigned nb = nblk((long)B * HW, chunk);
  const bool quad = dsum && chunk % 1024 == 0 && ((size_t)gout & 15) == 0 && ((size_t)depth & 15) == 0 && ((size_t)mask & 15) == 0 &&
                    ((size_t)noise_pixel & 15) == 0;
#define DG_HPF(A, PX)                                                                                                      \
  head_post_fwd_kernel<A, PX, LT><<<nb, 256, 0, s>>>(gout, noise_pixel, noise_image, training, tau, drop_const, B, HW, mask, \
                                                     depth, dsum, chunk, det)
#define DG_HPF_A(A) do { if (quad) DG_HPF(A, 4); else DG_HPF(A, 1); } while (0)
  if (arch == 0) { if constexpr (!LT) DG_HPF_A(0); } else if (arch == 1) DG_HPF_A(1); else DG_HPF_A(2);
#undef DG_HPF_A
#undef DG_HPF
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

// the two backward entry points' bodies, shared by the fixed-tau and the learnable-temperature forms
template <bool LT>
static int head_post_bwd_impl(const float* gout, const float* noise_pixel, const float* noise_image, const float* mask,
                              const float* ddepth, int arch, const HeadTau<LT> tau, float drop_const, int B, long HW,
                              float s_depth, float s_conf, float* draw, float* dbias, void* draw_pm, int cp, float* bias_ws,
                              void* s_) {
  hipStream_t s = (hipStream_t)s_;
  if (arch < 0 || arch > 2) return DG_EINVAL;
  const int cpk = !draw_pm ? 0 : (cp == 2 ? 2 : (cp == 4 ? 4 : 1));
  if (!draw && !draw_pm) return DG_EINVAL;
  auto al = [](const void* q) { return ((size_t)q & 15) == 0; };
  if (HW % 4 == 0 && cpk != 1 && al(gout) && al(ddepth) && al(draw) && al(draw_pm) && al(noise_pixel) && al(mask))
    return head_post_bwd_launch<4, HeadGradPlain, LT>(HeadGradPlain{ddepth}, gout, noise_pixel, noise_image, mask, arch, tau,
                                                      drop_const, B, HW, s_depth, s_conf, draw, dbias, draw_pm, cpk, cp, bias_ws, s);
  if (!draw) return DG_EUNSUPPORTED;   // (the scalar form always writes the planar copy)
  return head_post_bwd_launch<1, HeadGradPlain, LT>(HeadGradPlain{ddepth}, gout, noise_pixel, noise_image, mask, arch, tau,
                                                    drop_const, B, HW, s_depth, s_conf, draw, dbias, draw_pm, cpk, cp, bias_ws, s);
}

template <bool LT>
static int head_post_bwd_aug_impl(const float* gout, const float* noise_pixel, const float* noise_image, const float* mask,
                                  const float* gy, const float* u_b, const float* u_c, const int* t_h, const int* t_w,
                                  const int* o_x, const int* o_y, int policy, const float* gsum, int arch, const HeadTau<LT> tau,
                                  float drop_const, int B, int H, int W, float s_depth, float s_conf, float* draw, float* dbias,
                                  void* draw_pm, int cp, float* bias_ws, void* s_) {
  if (arch < 0 || arch > 2 || !gy || B <= 0 || H <= 0 || W <= 1) return DG_EINVAL;
  if (!draw && !draw_pm) return DG_EINVAL;
  if ((policy & 4) && !gsum) return DG_EINVAL;
  const int cpk = !draw_pm ? 0 : (cp == 2 ? 2 : (cp == 4 ? 4 : 1));
  auto al = [](const void* q) { return ((size_t)q & 15) == 0; };
  if (!(W % 4 == 0 && cpk != 1 && al(gout) && al(draw) && al(draw_pm) && al(noise_pixel) && al(mask))) return DG_EUNSUPPORTED;
  HeadGradAug dd{make_aug(u_b, u_c, t_h, t_w, o_x, o_y, policy, B, H, W), gy, gsum};
  return head_post_bwd_launch<4, HeadGradAug, LT>(dd, gout, noise_pixel, noise_image, mask, arch, tau, drop_const, B, (long)H * W,
                                                  s_depth, s_conf, draw, dbias, draw_pm, cpk, cp, bias_ws, (hipStream_t)s_);
}

// the learnable-temperature entry points' own argument checks: a dusty arch, the weights, a positive 1 / tau_max
static bool head_lt_ok(int arch, const float* tau_w, float inv_tau_min) {
  return (arch == 1 || arch == 2) && tau_w != nullptr && inv_tau_min > 0.f;
}

extern "C" {

int dg_head_post_fwd(float* gout, const float* noise_pixel, const float* noise_image, int arch, int training,
                     float tau, float drop_const, int B, long HW, float* mask, float* depth, void* s_) {
  return head_post_fwd_impl(gout, noise_pixel, noise_image, arch, training, HeadTau<false>{1.f / tau}, drop_const, B, HW, mask,
                            depth, nullptr, s_);
}
// ... + dsum[b] += sum of depth[b] (dsum zeroed by the caller; HW % 256 == 0 or DG_EUNSUPPORTED): the per-sample sums
// that dg_diffaug_fwd_pre takes instead of making its own pass over the image
int dg_head_post_fwd_sum(float* gout, const float* noise_pixel, const float* noise_image, int arch, int training,
                         float tau, float drop_const, int B, long HW, float* mask, float* depth, float* dsum, void* s_) {
  if (!dsum) return DG_EINVAL;
  return head_post_fwd_impl(gout, noise_pixel, noise_image, arch, training, HeadTau<false>{1.f / tau}, drop_const, B, HW, mask,
                            depth, dsum, s_);
}

int dg_head_post_bwd(const float* gout, const float* noise_pixel, const float* noise_image, const float* mask,
                     const float* ddepth, int arch, float tau, float drop_const, int B, long HW, float s_depth,
                     float s_conf, float* draw, float* dbias, void* draw_pm, int cp, float* bias_ws,
                     void* s_) {
  return head_post_bwd_impl<false>(gout, noise_pixel, noise_image, mask, ddepth, arch, HeadTau<false>{1.f / tau}, drop_const, B, HW,
                                   s_depth, s_conf, draw, dbias, draw_pm, cp, bias_ws, s_);
}

// dg_diffaug_bwd_pre + dg_head_post_bwd in one launch: d loss / d depth is DiffAugment's adjoint gather of gy (the BlurVH
// adjoint's output; gsum from dg_blur_bwd_augsum), evaluated per pixel quad where the head post-processing's backward
// needs it - the generator's upstream gradient [B,1,H,W] is never written.  DG_EUNSUPPORTED (nothing launched) unless the
// four-pixel form applies (W % 4 == 0, 16-byte aligned planes, cp 2 / 4 or no pixel-major copy).
int dg_head_post_bwd_aug(const float* gout, const float* noise_pixel, const float* noise_image, const float* mask,
                         const float* gy, const float* u_b, const float* u_c, const int* t_h, const int* t_w,
                         const int* o_x, const int* o_y, int policy, const float* gsum, int arch, float tau,
                         float drop_const, int B, int H, int W, float s_depth, float s_conf, float* draw, float* dbias,
                         void* draw_pm, int cp, float* bias_ws, void* s_) {
  return head_post_bwd_aug_impl<false>(gout, noise_pixel, noise_image, mask, gy, u_b, u_c, t_h, t_w, o_x, o_y, policy, gsum, arch,
                                       HeadTau<false>{1.f / tau}, drop_const, B, H, W, s_depth, s_conf, draw, dbias, draw_pm, cp,
                                       bias_ws, s_);
}

// ---- the learnable temperature (tau = None): the four entry points above with `float tau` replaced by tau_w (device pointer to
// the `arch` fp32 MASTER weights, pixel then image - never a bf16 shadow) and inv_tau_min = 1 / tau_max; the backward forms also
// take dtau_w (`arch` accumulators, added to like dbias).  arch 1 / 2; a null tau_w / dtau_w or inv_tau_min <= 0: DG_EINVAL.
int dg_head_post_fwd_lt(float* gout, const float* noise_pixel, const float* noise_image, int arch, int training,
                        const float* tau_w, float inv_tau_min, float drop_const, int B, long HW, float* mask, float* depth,
                        void* s_) {
  if (!head_lt_ok(arch, tau_w, inv_tau_min)) return DG_EINVAL;
  return head_post_fwd_impl<true>(gout, noise_pixel, noise_image, arch, training, HeadTau<true>{tau_w, inv_tau_min, nullptr},
                                  drop_const, B, HW, mask, depth, nullptr, s_);
}
int dg_head_post_fwd_sum_lt(float* gout, const float* noise_pixel, const float* noise_image, int arch, int training,
                            const float* tau_w, float inv_tau_min, float drop_const, int B, long HW, float* mask, float* depth,
                            float* dsum, void* s_) {
  if (!dsum || !head_lt_ok(arch, tau_w, inv_tau_min)) return DG_EINVAL;
  return head_post_fwd_impl<true>(gout, noise_pixel, noise_image, arch, training, HeadTau<true>{tau_w, inv_tau_min, nullptr},
                                  drop_const, B, HW, mask, depth, dsum, s_);
}
int dg_head_post_bwd_lt(const float* gout, const float* noise_pixel, const float* noise_image, const float* mask,
                        const float* ddepth, int arch, const float* tau_w, float inv_tau_min, float* dtau_w, float drop_const,
                        int B, long HW, float s_depth, float s_conf, float* draw, float* dbias, void* draw_pm, int cp,
                        float* bias_ws, void* s_) {
  if (!head_lt_ok(arch, tau_w, inv_tau_min) || !dtau_w) return DG_EINVAL;
  return head_post_bwd_impl<true>(gout, noise_pixel, noise_image, mask, ddepth, arch, HeadTau<true>{tau_w, inv_tau_min, dtau_w},
                                  drop_const, B, HW, s_depth, s_conf, draw, dbias, draw_pm, cp, bias_ws, s_);
}
int dg_head_post_bwd_aug_lt(const float* gout, const float* noise_pixel, const float* noise_image, const float* mask,
                            const float* gy, const float* u_b, const float* u_c, const int* t_h, const int* t_w,
                            const int* o_x, const int* o_y, int policy, const float* gsum, int arch, const float* tau_w,
                            float inv_tau_min, float* dtau_w, float drop_const, int B, int H, int W, float s_depth, float s_conf,
                            float* draw, float* dbias, void* draw_pm, int cp, float* bias_ws, void* s_) {
  if (!head_lt_ok(arch, tau_w, inv_tau_min) || !dtau_w) return DG_EINVAL;
  return head_post_bwd_aug_impl<true>(gout, noise_pixel, noise_image, mask, gy, u_b, u_c, t_h, t_w, o_x, o_y, policy, gsum, arch,
                                      HeadTau<true>{tau_w, inv_tau_min, dtau_w}, drop_const, B, H, W, s_depth, s_conf, draw, dbias,
                                      draw_pm, cp, bias_ws, s_);
}

int dg_head_post_bwd2(const float* gout, const float* noise_pixel, const float* noise_image, const float* mask,
                      const float* ddepth, const float* thead, int arch, float tau, float drop_const, int B, long HW,
                      float s_depth, float s_conf, float* draw, float* dbias, void* draw_pm, int cp, void* s_) {
  if (!gout || !ddepth || !thead || !draw || B <= 0 || HW <= 0 || arch < 0 || arch > 2) return DG_EINVAL;
  if (arch >= 1 && (!noise_pixel || !mask)) return DG_EINVAL;
  if (arch == 2 && !noise_image) return DG_EINVAL;
  if (draw_pm && (cp < 1 || cp > 4)) return DG_EINVAL;   // (the kernel's element-wise store writes channels 0..3)
  const long n = (long)B * HW;
  const int hb = (int)min((long)1024, (n + 255) / 256);
  head_post_bwd2_kernel<<<hb, 256, 0, (hipStream_t)s_>>>(gout, noise_pixel, noise_image, mask, ddepth, thead, arch,
                                                         1.f / tau, drop_const, B, HW, s_depth, s_conf, draw, dbias,
                                                         (bf16*)draw_pm, cp);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

}  // extern "C"
