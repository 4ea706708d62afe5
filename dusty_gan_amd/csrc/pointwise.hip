// HBM-bound kernels of the step's network end: the final (4 x w0) dot, head post-processing (tanh + Gumbel point-drop), the GAN
// losses, the path-length penalty, small reductions and zero-fills; and the registration of the accumulator arena.  (BlurVH,
// DiffAugment and sample_sum: blur_aug.hip; fetch_reals: step_inputs.hip.)  Images are fp32 [B,1,H,W]; feature maps are T.
#include "pointwise.h"
#include "diffaug.h"   // (HeadGradAug: DiffAugment's adjoint gather inside the head post-processing's backward)

// ----------------------------------------------------------------------------------------------------------
// Final EqualLR(Conv2d(C,1,(h0,w0))) (models/gans/dcgan_eqlr.py:95): y[b] = scale * <d4[b], wf> + bias.
template <typename T>
__global__ __launch_bounds__(256) void final_fwd_kernel(const T* __restrict__ d4, const float* __restrict__ wf,
                                                        const float* __restrict__ bias, float scale, long n,
                                                        float* __restrict__ y, const DgDet det) {
  // grid = (slabs, B): each block reduces one slab of one sample and adds it to y[b] (zeroed by the launcher);
  // slab 0 also adds the bias.  One block per sample left 7/8 of the chip idle (0.18 ms per call at B = 64).
  // 16-byte accesses (n % V == 0, checked by the launcher; else the scalar kernel below).
  __shared__ float red[16];
  constexpr int V = Vec16<T>::V;
  const int b = blockIdx.y;
  const T* row = d4 + (long)b * n;
  float acc = 0.f;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * V; i < n; i += (long)gridDim.x * blockDim.x * V) {
    float a[V];
    Vec16<T>::load(row + i, a);
#pragma unroll
    for (int k = 0; k < V; k += 4) {
      const float4 w4 = *(const float4*)(wf + i + k);
      acc += a[k] * w4.x + a[k + 1] * w4.y + a[k + 2] * w4.z + a[k + 3] * w4.w;
    }
  }
  const float s = dg_block_sum(acc, red);
  if (threadIdx.x == 0) dg_acc_add(&y[b], s * scale + ((bias && blockIdx.x == 0) ? bias[0] : 0.f), gridDim.x, det);
}
template <typename T>
__global__ __launch_bounds__(256) void final_fwd_scalar_kernel(const T* __restrict__ d4, const float* __restrict__ wf,
                                                               const float* __restrict__ bias, float scale, long n,
                                                               float* __restrict__ y, const DgDet det) {
  __shared__ float red[16];
  const int b = blockIdx.y;
  const T* row = d4 + (long)b * n;
  float acc = 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    acc += (float)row[i] * wf[i];
  const float s = dg_block_sum(acc, red);
  if (threadIdx.x == 0) dg_acc_add(&y[b], s * scale + ((bias && blockIdx.x == 0) ? bias[0] : 0.f), gridDim.x, det);
}

// dd4[b][i] = up[b] * scale * wf[i] * lrelu'(d4[b][i]) * sqrt2 ; dbias4[i % C] += rowscale[b] * dd4[b][i]
// A block owns 64 V consecutive elements; its four waves split the samples (wave w: b = w, w + 4, ...), a lane owns V
// consecutive elements (V consecutive channels: C % V == 0): 16-byte loads and stores, four samples in flight per
// element tile, the waves' bias-gradient partials meet in LDS and leave as ONE atomic per element per block.  (One
// element per thread over all samples in turn: 2-byte accesses, 15 us for 34 MB.)
template <typename T>
__global__ __launch_bounds__(256) void final_bwd_data_kernel(const T* __restrict__ d4, const float* __restrict__ wf,
                                                             const float* __restrict__ up,
                                                             const float* __restrict__ rowscale, float scale, int B,
                                                             long n, int C, T* __restrict__ dd4,
                                                             float* __restrict__ dbias) {
  constexpr int V = Vec16<T>::V;
  __shared__ float part[4][64 * V];
  __shared__ float s_u[256], s_r[256];          // per-sample factors (B <= 256, checked by the launcher): LDS reads inside
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;   // the loop keep its global loads free of other waits
  for (int b = threadIdx.x; b < B; b += 256) { s_u[b] = up ? up[b] : 1.f; s_r[b] = rowscale ? rowscale[b] : 1.f; }
  const long i = ((long)blockIdx.x * 64 + lane) * V;
  float w[V], db[V];
#pragma unroll
  for (int k = 0; k < V; ++k) { w[k] = 0.f; db[k] = 0.f; }
  if (i < n) {                                  // (n % V == 0: a thread's V elements are all inside)
#pragma unroll
    for (int k4 = 0; k4 < V; k4 += 4) {         // (wf 16-byte aligned: checked by the launcher)
      const float4 r = *(const float4*)(wf + i + k4);
      w[k4] = r.x * scale; w[k4 + 1] = r.y * scale; w[k4 + 2] = r.z * scale; w[k4 + 3] = r.w * scale;
    }
  }
  __syncthreads();
  if (i < n) {
#pragma unroll 4
    for (int b = wave; b < B; b += 4) {
      float a[V], g[V];
      Vec16<T>::load(d4 + (long)b * n + i, a);
      const float u = s_u[b], rs = s_r[b];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        g[k] = u * w[k] * (a[k] > 0.f ? SQRT2 : LRELU_SLOPE * SQRT2);
        db[k] += rs * g[k];
      }
      Vec16<T>::store(dd4 + (long)b * n + i, g);
    }
  }
  if (!dbias) return;
#pragma unroll
  for (int k = 0; k < V; ++k) part[wave][lane * V + k] = db[k];
  __syncthreads();
  for (int e = threadIdx.x; e < 64 * V; e += 256) {
    const long ie = (long)blockIdx.x * 64 * V + e;
    if (ie < n) atomicAdd(&dbias[ie % C], part[0][e] + part[1][e] + part[2][e] + part[3][e]);
  }
}
template <typename T>
__global__ __launch_bounds__(256) void final_bwd_data_scalar_kernel(const T* __restrict__ d4, const float* __restrict__ wf,
                                                                    const float* __restrict__ up,
                                                                    const float* __restrict__ rowscale, float scale,
                                                                    int B, long n, int C, T* __restrict__ dd4,
                                                                    float* __restrict__ dbias) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float w = wf[i] * scale;
  float db = 0.f;
  for (int b = 0; b < B; ++b) {
    const float a = (float)d4[(long)b * n + i];
    const float g = (up ? up[b] : 1.f) * w * (a > 0.f ? SQRT2 : LRELU_SLOPE * SQRT2);
    dd4[(long)b * n + i] = (T)g;
    db += (rowscale ? rowscale[b] : 1.f) * g;
  }
  if (dbias) atomicAdd(&dbias[i % C], db);
}

// out[i] += scale * sum_b coef[b] * src[b][i]   (coef null -> 1).  Vector form: a block owns 64 V consecutive elements,
// its four waves split the samples, partials meet in LDS, plain read-modify-write of out (no atomics).
template <typename T>
__global__ __launch_bounds__(256) void batch_wsum_kernel(const T* __restrict__ src, const float* __restrict__ coef,
                                                         float scale, int B, long n, float* __restrict__ out) {
  constexpr int V = Vec16<T>::V;
  __shared__ float part[4][64 * V];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long i = ((long)blockIdx.x * 64 + lane) * V;
  float acc[V];
#pragma unroll
  for (int k = 0; k < V; ++k) acc[k] = 0.f;
  if (i < n) {
#pragma unroll 8
    for (int b = wave; b < B; b += 4) {
      float a[V];
      Vec16<T>::load(src + (long)b * n + i, a);
      const float c = coef ? coef[b] : 1.f;
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] += c * a[k];
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) part[wave][lane * V + k] = acc[k];
  __syncthreads();
  for (int e = threadIdx.x; e < 64 * V; e += 256) {
    const long ie = (long)blockIdx.x * 64 * V + e;
    if (ie < n) out[ie] += (part[0][e] + part[1][e] + part[2][e] + part[3][e]) * scale;
  }
}
template <typename T>
__global__ void batch_wsum_scalar_kernel(const T* __restrict__ src, const float* __restrict__ coef, float scale, int B,
                                         long n, float* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float acc = 0.f;
  for (int b = 0; b < B; ++b) acc += (coef ? coef[b] : 1.f) * (float)src[(long)b * n + i];
  out[i] += acc * scale;
}

// ----------------------------------------------------------------------------------------------------------
// Head post-processing: Generator.forward's tanh (models/gans/dcgan_eqlr.py:71) + DUSty maskout
// (models/dusty.py:77-91, 107-127).  gout [B,1+k,H,W] planar fp32: ch0 raw depth -> tanh in place (depth_orig),
// ch1.. confidence logits (kept).  arch: 0 none, 1 dusty1, 2 dusty2.  noise_pixel [B,H,W], noise_image [B].
// dsum != nullptr: dsum[b] += sum of depth[b] - the per-sample sum DiffAugment's contrast needs of its input, produced where
// the image is produced.  A block then owns `chunk` consecutive pixels of ONE sample (HW % chunk == 0) and issues one atomic:
// with one block per 256 pixels the 8192 atomics on 32 addresses cost 80 us (round 1 met the same in head_post_bwd).
template <int arch>
__device__ __forceinline__ float head_post_px(float* __restrict__ gout, const float* __restrict__ noise_pixel,
                                              const float* __restrict__ noise_image, int training,
                                              float inv_tau, float drop_const, long HW, float* __restrict__ mask,
                                              int b, long p) {
  const long idx = (long)b * HW + p;
  const int nch = 1 + (arch == 0 ? 0 : arch);
  float* g = gout + (long)b * nch * HW + p;
  const float t = dg_tanh(g[0]);
  g[0] = t;
  if (arch == 0) return t;
  const float sp = 1.f / (1.f + __expf(-(g[HW] + noise_pixel[idx]) * inv_tau));
  const float mp = sp > 0.5f ? 1.f : 0.f;
  float m = mp;
  if (arch == 1) {
    mask[idx] = mp;
  } else {
    float mi;
    if (training) {
      const float si = 1.f / (1.f + __expf(-(g[2 * HW] + noise_image[b]) * inv_tau));
      mi = si > 0.5f ? 1.f : 0.f;
    } else {
      mi = g[2 * HW] > 0.f ? 1.f : 0.f;
    }
    mask[(long)b * 2 * HW + p] = mp;
    mask[(long)b * 2 * HW + HW + p] = mi;
    m = mp * mi;
  }
  return m * t + (1.f - m) * drop_const;
}
// Four consecutive pixels per thread (HW % 1024 == 0, sums wanted): 16-byte loads / stores of every plane; same arithmetic
// as head_post_px (which remains for other sizes).
template <int arch>
__global__ __launch_bounds__(256) void head_post_fwd4_kernel(float* __restrict__ gout, const float* __restrict__ noise_pixel,
                                      const float* __restrict__ noise_image, int training, float inv_tau,
                                      float drop_const, int B, long HW, float* __restrict__ mask,
                                      float* __restrict__ depth, float* __restrict__ dsum, int chunk, const DgDet det) {
  __shared__ float red[16];
  const long i0 = (long)blockIdx.x * chunk;
  const int b = (int)(i0 / HW);
  const long p0 = i0 - (long)b * HW;
  constexpr int nch = 1 + (arch == 0 ? 0 : arch);
  float* g = gout + (long)b * nch * HW + p0;
  const float ni = (arch == 2 && training) ? noise_image[b] : 0.f;
  float acc = 0.f;
  // the loads of four trips issued before the first store (gout is rewritten in place: the compiler cannot hoist a later
  // trip's loads over an earlier trip's stores, and one load in flight per wave left the launch at a third of the HBM rate)
  constexpr int U = 4;
  for (int k0 = threadIdx.x * 4; k0 < chunk; k0 += U * 1024) {
    float4 g0u[U], g1u[U], npu[U], g2u[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + u * 1024;
      if (k < chunk) {
        g0u[u] = *(const float4*)(g + k);
        if (arch >= 1) { g1u[u] = *(const float4*)(g + HW + k); npu[u] = *(const float4*)(noise_pixel + (long)b * HW + p0 + k); }
        if (arch == 2) g2u[u] = *(const float4*)(g + 2 * HW + k);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
    const int k = k0 + u * 1024;
    if (k >= chunk) break;
    const float4 g0 = g0u[u];
    float t[4] = {dg_tanh(g0.x), dg_tanh(g0.y), dg_tanh(g0.z), dg_tanh(g0.w)};
    *(float4*)(g + k) = make_float4(t[0], t[1], t[2], t[3]);
    float dv[4] = {t[0], t[1], t[2], t[3]};
    if (arch >= 1) {
      const float4 g1 = g1u[u], np = npu[u];
      const float l1[4] = {g1.x + np.x, g1.y + np.y, g1.z + np.z, g1.w + np.w};
      float mp[4], m[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float sp = 1.f / (1.f + __expf(-l1[q] * inv_tau));
        mp[q] = sp > 0.5f ? 1.f : 0.f;
        m[q] = mp[q];
      }
      if (arch == 1) {
        *(float4*)(mask + (long)b * HW + p0 + k) = make_float4(mp[0], mp[1], mp[2], mp[3]);
      } else {
        const float4 g2 = g2u[u];
        const float l2[4] = {g2.x, g2.y, g2.z, g2.w};
        float mi[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (training) {
            const float si = 1.f / (1.f + __expf(-(l2[q] + ni) * inv_tau));
            mi[q] = si > 0.5f ? 1.f : 0.f;
          } else {
            mi[q] = l2[q] > 0.f ? 1.f : 0.f;
          }
          m[q] = mp[q] * mi[q];
        }
        *(float4*)(mask + (long)b * 2 * HW + p0 + k) = make_float4(mp[0], mp[1], mp[2], mp[3]);
        *(float4*)(mask + (long)b * 2 * HW + HW + p0 + k) = make_float4(mi[0], mi[1], mi[2], mi[3]);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) dv[q] = m[q] * t[q] + (1.f - m[q]) * drop_const;
    }
    *(float4*)(depth + i0 + k) = make_float4(dv[0], dv[1], dv[2], dv[3]);
    acc += (dv[0] + dv[1]) + (dv[2] + dv[3]);
    }
  }
  const float sblk = dg_block_sum(acc, red);
  if (threadIdx.x == 0) dg_acc_add(&dsum[b], sblk, (unsigned)(HW / chunk), det);
}

template <int arch>   // compile-time: the pixel function is then straight-line code and the unrolled trips batch their loads
__global__ __launch_bounds__(256) void head_post_fwd_kernel(float* __restrict__ gout, const float* __restrict__ noise_pixel,
                                     const float* __restrict__ noise_image, int training, float inv_tau,
                                     float drop_const, int B, long HW, float* __restrict__ mask,
                                     float* __restrict__ depth, float* __restrict__ dsum, int chunk, const DgDet det) {
  __shared__ float red[16];
  if (!dsum) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < (long)B * HW) {
      const int b = (int)(idx / HW);
      depth[idx] = head_post_px<arch>(gout, noise_pixel, noise_image, training, inv_tau, drop_const, HW, mask, b, idx - (long)b * HW);
    }
    return;
  }
  // the block's pixels belong to ONE sample (HW % chunk == 0): the sample index is block-uniform, and the four pixels a
  // thread handles per trip are independent - unrolled so that their loads are in flight together (a 64-bit division per
  // pixel and one round trip per pixel made this 15 us for 25 MB)
  const long i0 = (long)blockIdx.x * chunk;
  const int b = (int)(i0 / HW);
  const long p0 = i0 - (long)b * HW;
  float acc = 0.f;
#pragma unroll 4
  for (int k = threadIdx.x; k < chunk; k += 256) {
    const float dv = head_post_px<arch>(gout, noise_pixel, noise_image, training, inv_tau, drop_const, HW, mask, b, p0 + k);
    depth[i0 + k] = dv;
    acc += dv;
  }
  const float sblk = dg_block_sum(acc, red);
  if (threadIdx.x == 0) dg_acc_add(&dsum[b], sblk, (unsigned)(HW / chunk), det);
}

// Backward of the above: ddepth [B,H,W] -> draw [B,1+k,H,W] planar (gradient w.r.t. the head conv outputs).
template <int arch, int CP>   // CP: 0 no pixel-major copy, 2 / 4 that padded channel count, 1 any other (`cp`)
__global__ __launch_bounds__(256) void head_post_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ noise_pixel,
                                     const float* __restrict__ noise_image, const float* __restrict__ mask,
                                     const float* __restrict__ ddepth, float inv_tau, float drop_const,
                                     int B, long HW, float s_depth, float s_conf, float* __restrict__ draw,
                                     float* __restrict__ dbias, bf16* __restrict__ draw_pm, int cp) {
  __shared__ float red[16];
  // grid-stride: a block covers many pixels so that the bias-gradient sums cost one atomic per block per head (one
  // pixel per thread meant 8192 atomics on the same address: 100 us of the 108 us this kernel took at B = 32)
  // blockIdx.y = sample (no 64-bit division per pixel); straight-line body (arch and the copy's layout are compile-time),
  // four independent pixels per trip in flight together
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  const int b = blockIdx.y;
#pragma unroll 4
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += (long)gridDim.x * blockDim.x) {
  const long idx = (long)b * HW + p;
  float d0 = 0.f, d1 = 0.f, d2 = 0.f;  // unscaled gradients w.r.t. the head outputs (= the head bias gradients)
  {
  const int nch = 1 + (arch == 0 ? 0 : arch);
  const float* g = gout + (long)b * nch * HW + p;
  float* d = draw + (long)b * nch * HW + p;
  const float t = g[0];
  const float dt = 1.f - t * t;
  const float go = ddepth[idx];
  if (arch == 0) {
    d0 = go * dt;
  } else {
    const float sp = 1.f / (1.f + __expf(-(g[HW] + noise_pixel[idx]) * inv_tau));
    const float dmask = go * (t - drop_const);
    if (arch == 1) {
      const float mp = mask[idx];
      d0 = mp * go * dt;
      d1 = dmask * sp * (1.f - sp) * inv_tau;
    } else {
      const float mp = mask[(long)b * 2 * HW + p], mi = mask[(long)b * 2 * HW + HW + p];
      const float si = 1.f / (1.f + __expf(-(g[2 * HW] + noise_image[b]) * inv_tau));
      d0 = mp * mi * go * dt;
      d1 = dmask * mi * sp * (1.f - sp) * inv_tau;
      d2 = dmask * mp * si * (1.f - si) * inv_tau;
      d[2 * HW] = d2 * s_conf;
    }
    d[HW] = d1 * s_conf;
  }
  d[0] = d0 * s_depth;
  if (CP != 0) {  // second copy, pixel-major / channel-minor bf16 [B,H,W,cp], channels zero-padded: the operand layout
                  // of the MFMA backward-data kernel (thin_s2_mfma); one store per pixel for cp = 2 / 4
    const unsigned short h0 = __builtin_bit_cast(unsigned short, (bf16)(d0 * s_depth));
    const unsigned short h1 = __builtin_bit_cast(unsigned short, (bf16)(arch >= 1 ? d1 * s_conf : 0.f));
    const unsigned short h2 = __builtin_bit_cast(unsigned short, (bf16)(arch >= 2 ? d2 * s_conf : 0.f));
    if (CP == 2) {
      *(unsigned*)(draw_pm + idx * 2) = (unsigned)h0 | ((unsigned)h1 << 16);
    } else if (CP == 4) {
      *(uint2*)(draw_pm + idx * 4) = make_uint2((unsigned)h0 | ((unsigned)h1 << 16), (unsigned)h2);
    } else {      // any other padded channel count
      bf16* q = draw_pm + idx * cp;
      q[0] = __builtin_bit_cast(bf16, h0);
      if (cp > 1) q[1] = __builtin_bit_cast(bf16, h1);
      if (cp > 2) q[2] = __builtin_bit_cast(bf16, h2);
      for (int c = 3; c < cp; ++c) q[c] = (bf16)0.f;
    }
  }
  }
  a0 += d0; a1 += d1; a2 += d2;
  }
  if (dbias) {  // head biases are outside EqualLR's input scaling: their gradient is the unscaled sum
    const float s0 = dg_block_sum(a0, red);
    if (threadIdx.x == 0) atomicAdd(&dbias[0], s0);
    if (arch >= 1) { const float s1 = dg_block_sum(a1, red); if (threadIdx.x == 0) atomicAdd(&dbias[1], s1); }
    if (arch >= 2) { const float s2 = dg_block_sum(a2, red); if (threadIdx.x == 0) atomicAdd(&dbias[2], s2); }
  }
}

// Where head_post_bwd4_kernel gets d loss / d depth of a pixel quad from: the tensor itself, or - HeadGradAug, diffaug.h -
// DiffAugment's adjoint gather applied on the fly to the BlurVH adjoint's output.
struct HeadGradPlain {
  const float* ddepth;
  __device__ __forceinline__ float4 operator()(int b, long p, long HW) const { return *(const float4*)(ddepth + (long)b * HW + p); }
};

// Four consecutive pixels per thread (HW % 4 == 0): 16-byte loads of every plane, 16-byte stores; `draw` (the planar fp32
// copy) may be null - the bf16 path consumes only the pixel-major copy, and three 8 MB planes were written for nobody.
template <int arch, int CP, typename DD>   // CP: 2 / 4 padded channel count of the pixel-major copy, 0 none
__global__ __launch_bounds__(256) void head_post_bwd4_kernel(const float* __restrict__ gout, const float* __restrict__ noise_pixel,
                                      const float* __restrict__ noise_image, const float* __restrict__ mask,
                                      DD ddepth, float inv_tau, float drop_const, int B, long HW,
                                      float s_depth, float s_conf, float* __restrict__ draw, float* __restrict__ dbias,
                                      bf16* __restrict__ draw_pm, float* __restrict__ bias_ws) {
  __shared__ float red[16];
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  const int b = blockIdx.y;
  constexpr int nch = 1 + (arch == 0 ? 0 : arch);
  const float* g = gout + (long)b * nch * HW;
  const float ni = arch == 2 ? noise_image[b] : 0.f;
  auto ld = [](const float* q) { const float4 v = *(const float4*)q; return v; };
  for (long p = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; p < HW; p += (long)gridDim.x * blockDim.x * 4) {
    const long idx = (long)b * HW + p;
    const float4 t4 = ld(g + p), go4 = ddepth(b, p, HW);
    const float t[4] = {t4.x, t4.y, t4.z, t4.w}, go[4] = {go4.x, go4.y, go4.z, go4.w};
    float d0[4], d1[4] = {0.f, 0.f, 0.f, 0.f}, d2[4] = {0.f, 0.f, 0.f, 0.f};
    if (arch == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) d0[q] = go[q] * (1.f - t[q] * t[q]);
    } else {
      const float4 g14 = ld(g + HW + p), np4 = ld(noise_pixel + idx);
      const float l1[4] = {g14.x + np4.x, g14.y + np4.y, g14.z + np4.z, g14.w + np4.w};
      float mp[4], mi[4] = {1.f, 1.f, 1.f, 1.f}, l2[4] = {0.f, 0.f, 0.f, 0.f};
      if (arch == 1) {
        const float4 m4 = ld(mask + idx);
        mp[0] = m4.x; mp[1] = m4.y; mp[2] = m4.z; mp[3] = m4.w;
      } else {
        const float4 m4 = ld(mask + (long)b * 2 * HW + p), i4 = ld(mask + (long)b * 2 * HW + HW + p), g24 = ld(g + 2 * HW + p);
        mp[0] = m4.x; mp[1] = m4.y; mp[2] = m4.z; mp[3] = m4.w;
        mi[0] = i4.x; mi[1] = i4.y; mi[2] = i4.z; mi[3] = i4.w;
        l2[0] = g24.x; l2[1] = g24.y; l2[2] = g24.z; l2[3] = g24.w;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float dt = 1.f - t[q] * t[q];
        const float sp = 1.f / (1.f + __expf(-l1[q] * inv_tau));
        const float dmask = go[q] * (t[q] - drop_const);
        if (arch == 1) {
          d0[q] = mp[q] * go[q] * dt;
          d1[q] = dmask * sp * (1.f - sp) * inv_tau;
        } else {
          const float si = 1.f / (1.f + __expf(-(l2[q] + ni) * inv_tau));
          d0[q] = mp[q] * mi[q] * go[q] * dt;
          d1[q] = dmask * mi[q] * sp * (1.f - sp) * inv_tau;
          d2[q] = dmask * mp[q] * si * (1.f - si) * inv_tau;
        }
      }
    }
    if (draw) {
      float* d = draw + (long)b * nch * HW + p;
      *(float4*)d = make_float4(d0[0] * s_depth, d0[1] * s_depth, d0[2] * s_depth, d0[3] * s_depth);
      if (arch >= 1) *(float4*)(d + HW) = make_float4(d1[0] * s_conf, d1[1] * s_conf, d1[2] * s_conf, d1[3] * s_conf);
      if (arch >= 2) *(float4*)(d + 2 * HW) = make_float4(d2[0] * s_conf, d2[1] * s_conf, d2[2] * s_conf, d2[3] * s_conf);
    }
    if (CP != 0) {
      unsigned w01[4], w2[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned short h0 = __builtin_bit_cast(unsigned short, (bf16)(d0[q] * s_depth));
        const unsigned short h1 = __builtin_bit_cast(unsigned short, (bf16)(arch >= 1 ? d1[q] * s_conf : 0.f));
        const unsigned short h2 = __builtin_bit_cast(unsigned short, (bf16)(arch >= 2 ? d2[q] * s_conf : 0.f));
        w01[q] = (unsigned)h0 | ((unsigned)h1 << 16);
        w2[q] = (unsigned)h2;
      }
      if (CP == 2) {
        *(uint4*)(draw_pm + idx * 2) = make_uint4(w01[0], w01[1], w01[2], w01[3]);
      } else {
        *(uint4*)(draw_pm + idx * 4) = make_uint4(w01[0], w2[0], w01[1], w2[1]);
        *(uint4*)(draw_pm + idx * 4 + 8) = make_uint4(w01[2], w2[2], w01[3], w2[3]);
      }
    }
    a0 += (d0[0] + d0[1]) + (d0[2] + d0[3]);
    a1 += (d1[0] + d1[1]) + (d1[2] + d1[3]);
    a2 += (d2[0] + d2[1]) + (d2[2] + d2[3]);
  }
  if (dbias) {
    // Atomics on ONE address retire at ~10 ns each (they execute memory-side): a thousand blocks adding straight into
    // dbias[n] cost 10 us per head - more than the pass over the data.  With `bias_ws` (4 KB per sample, zero on entry and
    // left zero) the blocks of a sample add into that sample's slot - B independent addresses - and the last one to
    // arrive (a ticket in the slot) folds the slot into dbias: gridDim.x adds per slot, B per dbias[n].
    const float s0 = dg_block_sum(a0, red);
    const float s1 = arch >= 1 ? dg_block_sum(a1, red) : 0.f;
    const float s2 = arch >= 2 ? dg_block_sum(a2, red) : 0.f;
    if (threadIdx.x == 0) {
      if (bias_ws && gridDim.x > 1) {
        // Round 5: the staged sums are 32.32 FIXED POINT (integer adds commute: the total no longer depends on the order in
        // which blocks and samples arrive - common.h has the protocol and its argument).  Two levels, as before: the blocks of a
        // sample add into that sample's slot; the last block of a sample (ticket) moves the slot's totals, still integers,
        // into the launch's accumulators (upper half of slot 0) and takes a second ticket; the last SAMPLE converts and adds
        // each head's total to dbias once.  Everything is left zero.
        unsigned long long* w = (unsigned long long*)(bias_ws + (long)b * DG_BIAS_WS_SAMPLE_FLOATS);
        unsigned long long* gacc = (unsigned long long*)(bias_ws + DG_BIAS_WS_ACC);
        const float sv[3] = {s0, s1, s2};
#pragma unroll
        for (int h = 0; h <= arch; ++h) {
          long long q;
          if (dg_fix1(sv[h], q)) atomicAdd(&w[h], (unsigned long long)q);
          else atomicAdd(&dbias[h], sv[h]);
        }
        if (dg_ticket_last(dg_bias_ws_ticket(w), gridDim.x)) {
#pragma unroll
          for (int h = 0; h <= arch; ++h) atomicAdd(&gacc[h], atomicExch(&w[h], 0ull));
          if (dg_ticket_last(dg_bias_ws_ticket(gacc), gridDim.y)) {
#pragma unroll
            for (int h = 0; h <= arch; ++h) atomicAdd(&dbias[h], dg_fix1_value((long long)atomicExch(&gacc[h], 0ull)));
          }
        }
      } else {
        atomicAdd(&dbias[0], s0);
        if (arch >= 1) atomicAdd(&dbias[1], s1);
        if (arch >= 2) atomicAdd(&dbias[2], s2);
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------------------
// Path-length regularisation (trainers/dcgan_amp.py:268-306), the pieces that are not convolutions.
//
// head_post_bwd2_kernel: the SECOND-order part of the head post-processing.  With x = depth output, h = the head conv
// outputs (h0 raw depth, h1 / h2 confidence logits), y the upstream of x and th the forward-mode tangent of h along
// the latent direction v, the tangent of the first-order backward d x / d h_i * y is  y * sum_j H_ij th_j  with H the
// Hessian of x in h as autograd sees it (hard masks carry the straight-through derivative sp' = sp (1 - sp) / tau,
// which is itself differentiable: sp'' = sp' (1 - 2 sp) / tau):
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
    const int nch = 1 + (arch == 0 ? 0 : arch);
    const float* g = gout + (long)b * nch * HW + p;
    const float* th = thead + (long)b * nch * HW + p;
    float* d = draw + (long)b * nch * HW + p;
    const float t = g[0], dt = 1.f - t * t, y = ddepth[idx];
    const float t0 = th[0];
    float d0, d1 = 0.f, d2 = 0.f;
    if (arch == 0) {
      d0 = y * (-2.f * t * dt) * t0;
    } else {
      const float sp = 1.f / (1.f + __expf(-(g[HW] + noise_pixel[idx]) * inv_tau));
      const float sp1 = sp * (1.f - sp) * inv_tau, sp2 = sp1 * (1.f - 2.f * sp) * inv_tau;
      const float t1 = th[HW], tc = t - drop_const;
      if (arch == 1) {
        const float mp = mask[idx];
        d0 = y * (mp * (-2.f * t * dt) * t0 + sp1 * dt * t1);
        d1 = y * (sp1 * dt * t0 + tc * sp2 * t1);
      } else {
        const float mp = mask[(long)b * 2 * HW + p], mi = mask[(long)b * 2 * HW + HW + p];
        const float si = 1.f / (1.f + __expf(-(g[2 * HW] + noise_image[b]) * inv_tau));
        const float si1 = si * (1.f - si) * inv_tau, si2 = si1 * (1.f - 2.f * si) * inv_tau;
        const float t2 = th[2 * HW];
        d0 = y * (mp * mi * (-2.f * t * dt) * t0 + mi * sp1 * dt * t1 + mp * si1 * dt * t2);
        d1 = y * (mi * sp1 * dt * t0 + tc * mi * sp2 * t1 + tc * sp1 * si1 * t2);
        d2 = y * (mp * si1 * dt * t0 + tc * sp1 * si1 * t1 + tc * mp * si2 * t2);
        d[2 * HW] = d2 * s_conf;
      }
      d[HW] = d1 * s_conf;
    }
    d[0] = d0 * s_depth;
    if (draw_pm) {
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

// |J^T y| per sample, the running baseline and the penalty (:294-300), and v = w * d penalty / d dz, the direction of
// the forward-over-reverse pass.  pl_ema (device scalar) is updated in place; acc[0] += baseline, acc[1] += penalty.
// The baseline a = ema + 0.01 (mean l - ema) stays in the graph in the reference (lerp of a live mean), hence the
// second term of  dP/dl_b = (2/B) [(l_b - a) - 0.01 mean_c (l_c - a)].
__global__ __launch_bounds__(256) void pl_penalty_kernel(const float* __restrict__ dz, int B, int K, float w,
                                                         float* __restrict__ pl_ema, float* __restrict__ v,
                                                         float* __restrict__ acc) {
  __shared__ float len[256];
  __shared__ float bc[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int b = wave; b < B; b += 4) {  // one wave per sample
    float s = 0.f;
    for (int k = lane; k < K; k += 64) { const float x = dz[(long)b * K + k]; s += x * x; }
    s = dg_wave_sum(s);
    if (lane == 0) len[b] = sqrtf(s);
  }
  __syncthreads();
  if (tid == 0) {
    float mu = 0.f;
    for (int b = 0; b < B; ++b) mu += len[b];
    mu /= (float)B;
    const float ema = pl_ema[0];
    const float a = ema + 0.01f * (mu - ema);
    float pen = 0.f, dev = 0.f;
    for (int b = 0; b < B; ++b) { const float e = len[b] - a; pen += e * e; dev += e; }
    pl_ema[0] = a;
    acc[0] += a;
    acc[1] += pen / (float)B;
    bc[0] = a;
    bc[1] = dev / (float)B;
  }
  __syncthreads();
  const float a = bc[0], mdev = bc[1];
  for (long i = tid; i < (long)B * K; i += 256) {
    const int b = (int)(i / K);
    const float l = len[b];
    const float dl = (2.f / (float)B) * ((l - a) - 0.01f * mdev);
    v[i] = l > 0.f ? w * dl * dz[i] / l : 0.f;
  }
}

// ----------------------------------------------------------------------------------------------------------
// NSGAN losses (models/loss.py:39-41, 68-69) + their gradients w.r.t. the logits; one block.
// scal[0]=mean(y_real) scal[1]=mean(y_fake) scal[2]=loss_D ; dy_* = d(w_gan*loss_D)/dy
__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(__expf(x)); }
__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + __expf(-x)); }

__global__ __launch_bounds__(256) void nsgan_d_kernel(const float* __restrict__ y_real,
                                                      const float* __restrict__ y_fake, int B, float w_gan,
                                                      float* __restrict__ dy_real, float* __restrict__ dy_fake,
                                                      float* __restrict__ scal) {
  __shared__ float red[16];
  float sr = 0.f, sf = 0.f, lr = 0.f, lf = 0.f;
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    const float r = y_real[i], f = y_fake[i];
    sr += r; sf += f;
    lr += softplus_f(-r); lf += softplus_f(f);
    dy_real[i] = -w_gan * sigmoid_f(-r) / (float)B;
    dy_fake[i] = w_gan * sigmoid_f(f) / (float)B;
  }
  const float a = dg_block_sum(sr, red), b = dg_block_sum(sf, red);
  const float c = dg_block_sum(lr, red), d = dg_block_sum(lf, red);
  if (threadIdx.x == 0) {
    scal[0] = a / B; scal[1] = b / B; scal[2] = c / B + d / B;
  }
}

// scal[0] = loss_G ; dy = d(w_gan*loss_G)/dy_fake
__global__ __launch_bounds__(256) void nsgan_g_kernel(const float* __restrict__ y_fake, int B, float w_gan,
                                                      float* __restrict__ dy, float* __restrict__ scal) {
  __shared__ float red[16];
  float l = 0.f;
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    const float f = y_fake[i];
    l += softplus_f(-f);
    dy[i] = -w_gan * sigmoid_f(-f) / (float)B;
  }
  const float s = dg_block_sum(l, red);
  if (threadIdx.x == 0) scal[0] = s / B;
}

// The D-phase bookkeeping around the loss in one launch (trainers/dcgan_amp.py:203-238): loss + dLoss/dy as
// nsgan_d_kernel, plus the two per-sample vectors the R1 schedule feeds the backward with (up = [1 .. 1 | dy_fake],
// rs = [dy_real | 1 .. 1]; either may be null), the running sums of the logged scalars (acc[0..2] +=) and the
// final bias gradient (dfinal_b += sum dy).  Replaces eight tiny torch kernels per step.
__global__ __launch_bounds__(256) void nsgan_d_step_kernel(const float* __restrict__ y_real,
                                                           const float* __restrict__ y_fake, int B, float w_gan,
                                                           float* __restrict__ dy, float* __restrict__ up,
                                                           float* __restrict__ rs, float* __restrict__ acc,
                                                           float* __restrict__ dfinal_b) {
  __shared__ float red[16];
  float sr = 0.f, sf = 0.f, lr = 0.f, lf = 0.f, sd = 0.f;
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    const float r = y_real[i], f = y_fake[i];
    sr += r; sf += f;
    lr += softplus_f(-r); lf += softplus_f(f);
    const float dr = -w_gan * sigmoid_f(-r) / (float)B, df = w_gan * sigmoid_f(f) / (float)B;
    dy[i] = dr; dy[B + i] = df;
    if (up) { up[i] = 1.f; up[B + i] = df; }
    if (rs) { rs[i] = dr; rs[B + i] = 1.f; }
    sd += dr + df;
  }
  const float a = dg_block_sum(sr, red), b = dg_block_sum(sf, red);
  const float c = dg_block_sum(lr, red), d = dg_block_sum(lf, red), e = dg_block_sum(sd, red);
  if (threadIdx.x == 0) {
    acc[0] += a / B; acc[1] += b / B; acc[2] += c / B + d / B;
    if (dfinal_b) dfinal_b[0] += e;
  }
}

// acc[0] += loss_G ; dy = d(w_gan*loss_G)/dy_fake
__global__ __launch_bounds__(256) void nsgan_g_step_kernel(const float* __restrict__ y_fake, int B, float w_gan,
                                                           float* __restrict__ dy, float* __restrict__ acc) {
  __shared__ float red[16];
  float l = 0.f;
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    const float f = y_fake[i];
    l += softplus_f(-f);
    dy[i] = -w_gan * sigmoid_f(-f) / (float)B;
  }
  const float s = dg_block_sum(l, red);
  if (threadIdx.x == 0) acc[0] += s / B;
}

// ----------------------------------------------------------------------------------------------------------
// All seven GANLoss metrics (models/loss.py:39-61 loss_D, :66-85 loss_G) as one kernel.  Every metric is
//   loss = mean_i phi_r(a_i) + mean_i phi_f(b_i),   a = y_real - [rel] mean(y_fake),  b = y_fake - [rel] mean(y_real)
// with phi from a small family; `rel` marks the relativistic-average metrics (average_diff, loss.py:11-18).
//   d loss / d y_real_i = phi_r'(a_i)/B - [rel] mean_j phi_f'(b_j) / B      (and symmetrically for y_fake)
enum { PHI_NONE = 0, PHI_SOFTPLUS = 1, PHI_LINEAR = 2, PHI_SQUARE = 3, PHI_HINGE = 4 };
struct GanForm {
  int kr, kf;        // phi family of the real / fake term
  float sr, sf;      // sign applied to the argument: softplus(s x), s x, relu(1 + s x)
  float cr, cf;      // target of the square: (x - c)^2
  int rel;
};

// value and derivative of phi(kind, s, c) at x
__device__ __forceinline__ void gan_phi(int kind, float s, float c, float x, float& v, float& d) {
  switch (kind) {
    case PHI_SOFTPLUS: v = softplus_f(s * x); d = s * sigmoid_f(s * x); break;
    case PHI_LINEAR: v = s * x; d = s; break;
    case PHI_SQUARE: v = (x - c) * (x - c); d = 2.f * (x - c); break;
    case PHI_HINGE: { const float t = 1.f + s * x; v = t > 0.f ? t : 0.f; d = t > 0.f ? s : 0.f; } break;
    default: v = 0.f; d = 0.f;
  }
}

static int gan_form(int metric, int mode_g, float smoothing, GanForm* f) {
  // rows follow models/loss.py:39-61 (D) and :66-85 (G)
  const GanForm D[7] = {
      {PHI_SOFTPLUS, PHI_SOFTPLUS, -1.f, 1.f, 0.f, 0.f, 0},      // nsgan
      {PHI_LINEAR, PHI_LINEAR, -1.f, 1.f, 0.f, 0.f, 0},          // wgan
      {PHI_SQUARE, PHI_SQUARE, 0.f, 0.f, smoothing, 0.f, 0},     // lsgan (label_real * smoothing, label_fake = 0)
      {PHI_HINGE, PHI_HINGE, -1.f, 1.f, 0.f, 0.f, 0},            // hinge
      {PHI_SOFTPLUS, PHI_SOFTPLUS, -1.f, 1.f, 0.f, 0.f, 1},      // ragan
      {PHI_HINGE, PHI_HINGE, -1.f, 1.f, 0.f, 0.f, 1},            // rahinge
      {PHI_SQUARE, PHI_SQUARE, 0.f, 0.f, 1.f, -1.f, 1}};         // ralsgan
  const GanForm G[7] = {
      {PHI_NONE, PHI_SOFTPLUS, 0.f, -1.f, 0.f, 0.f, 0},          // nsgan
      {PHI_NONE, PHI_LINEAR, 0.f, -1.f, 0.f, 0.f, 0},            // wgan
      {PHI_NONE, PHI_SQUARE, 0.f, 0.f, 0.f, 1.f, 0},             // lsgan (target 1, not smoothed: loss.py:71-72)
      {PHI_NONE, PHI_LINEAR, 0.f, -1.f, 0.f, 0.f, 0},            // hinge
      {PHI_SOFTPLUS, PHI_SOFTPLUS, 1.f, -1.f, 0.f, 0.f, 1},      // ragan
      {PHI_HINGE, PHI_HINGE, 1.f, -1.f, 0.f, 0.f, 1},            // rahinge
      {PHI_SQUARE, PHI_SQUARE, 0.f, 0.f, -1.f, 1.f, 1}};         // ralsgan
  if (metric < 0 || metric > 6) return DG_EUNSUPPORTED;
  *f = mode_g ? G[metric] : D[metric];
  return DG_OK;
}

// One block.  D mode (mode_g = 0): dy = [d/dy_real | d/dy_fake] of w_gan * loss, up / rs / dfinal_b / acc[0..2] as in
// nsgan_d_step_kernel.  G mode: only the fake half carries a gradient (D(real) is data, trainers/dcgan_amp.py:259);
// dy = d(w_gan * loss)/dy_fake, acc[0] += loss; y_real may be null unless the metric is relativistic.
// `red` >= 17 floats of LDS.  dy / up / rs may be LDS (the fused final-layer kernel: every block evaluates the step for
// itself) or global memory; `write_acc`: add the scalars / the final bias gradient (one block only).
__device__ __forceinline__ void gan_step_body(const GanForm& fm, int mode_g, const float* __restrict__ y_real,
                                              const float* __restrict__ y_fake, int B, float w_gan, float* dy, float* up,
                                              float* rs, bool write_acc, float* __restrict__ acc,
                                              float* __restrict__ dfinal_b, float* red) {
  auto bsum = [&](float v) {  // block sum, broadcast to every thread
    const float r = dg_block_sum(v, red);
    __syncthreads();
    if (threadIdx.x == 0) red[16] = r;
    __syncthreads();
    return red[16];
  };
  const bool has_r = (fm.kr != PHI_NONE) || !mode_g;
  float sr = 0.f, sf = 0.f;
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    if (has_r) sr += y_real[i];
    sf += y_fake[i];
  }
  const float mr = bsum(sr) / B, mf = bsum(sf) / B;
  const float offr = fm.rel ? mf : 0.f, offf = fm.rel ? mr : 0.f;
  float lsum = 0.f, dsr = 0.f, dsf = 0.f;
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    float v, d;
    if (fm.kr != PHI_NONE) {
      gan_phi(fm.kr, fm.sr, fm.cr, y_real[i] - offr, v, d);
      lsum += v; dsr += d;
    }
    gan_phi(fm.kf, fm.sf, fm.cf, y_fake[i] - offf, v, d);
    lsum += v; dsf += d;
  }
  const float loss = bsum(lsum) / B;
  const float mdr = bsum(dsr) / B, mdf = bsum(dsf) / B;
  const float k = w_gan / (float)B;
  float sd = 0.f;
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    float v, d, dr = 0.f;
    if (fm.kr != PHI_NONE) {
      gan_phi(fm.kr, fm.sr, fm.cr, y_real[i] - offr, v, d);
      dr = k * (d - (fm.rel ? mdf : 0.f));
    }
    gan_phi(fm.kf, fm.sf, fm.cf, y_fake[i] - offf, v, d);
    const float df = k * (d - (fm.rel ? mdr : 0.f));
    if (mode_g) {
      dy[i] = df;
    } else {
      dy[i] = dr; dy[B + i] = df;
      if (up) { up[i] = 1.f; up[B + i] = df; }
      if (rs) { rs[i] = dr; rs[B + i] = 1.f; }
      sd += dr + df;
    }
  }
  const float e = dg_block_sum(sd, red);
  if (threadIdx.x == 0 && write_acc) {
    if (mode_g) {
      acc[0] += loss;
    } else {
      acc[0] += mr; acc[1] += mf; acc[2] += loss;
      if (dfinal_b) dfinal_b[0] += e;
    }
  }
}
__global__ __launch_bounds__(256) void gan_step_kernel(GanForm fm, int mode_g, const float* __restrict__ y_real,
                                                       const float* __restrict__ y_fake, int B, float w_gan,
                                                       float* __restrict__ dy, float* __restrict__ up,
                                                       float* __restrict__ rs, float* __restrict__ acc,
                                                       float* __restrict__ dfinal_b) {
  __shared__ float red[17];
  gan_step_body(fm, mode_g, y_real, y_fake, B, w_gan, dy, up, rs, true, acc, dfinal_b, red);
}

// The loss step and the final conv's backward in ONE launch (three in the D phase, two in the G phase otherwise): every
// block evaluates the loss step on the 2B (or B) logits for itself - a few hundred flops - and keeps the per-sample
// vectors in LDS; block 0 also writes them out (later launches read dy / rs) and adds the scalars.  Then the block's
// element range of the final conv's backward-data pass (final_bwd_data_kernel) and, in the same sweep over the samples,
// of its weight gradient dwf[i] += scale * sum_b dy[b] d4[b][i] (dg_batch_wsum) - d4 is read once for both.
// D mode: ns = 2B samples [real | fake]; r1: chain upstream [1 | dy_fake], bias-gradient weights [dy_real | 1] (the R1
// schedule), else upstream dy, weights 1.  G mode: ns = B samples (the fake batch), upstream dy.
template <typename T>
__global__ __launch_bounds__(512) void final_gan_bwd_kernel(GanForm fm, int mode_g, const float* __restrict__ y_real,
                                                            const float* __restrict__ y_fake, int B, float w_gan, int r1,
                                                            float* __restrict__ dy, float* __restrict__ up,
                                                            float* __restrict__ rs, float* __restrict__ acc,
                                                            float* __restrict__ dfinal_b, const T* __restrict__ d4,
                                                            const float* __restrict__ wf, float scale, long n, int C,
                                                            T* __restrict__ dd4, float* __restrict__ dbias,
                                                            float* __restrict__ dwf, float* __restrict__ dbias_part) {
  constexpr int V = Vec16<T>::V;
  constexpr int NW = 8;                           // waves per workgroup (round 6: four left one workgroup per CU with 16-32 KB in flight)
  __shared__ float part[NW][64 * V];
  __shared__ float s_dy[256], s_u[256], s_r[256], red[17];
  const int ns = mode_g ? B : 2 * B;
  gan_step_body(fm, mode_g, y_real, y_fake, B, w_gan, s_dy, r1 ? s_u : nullptr, r1 ? s_r : nullptr, blockIdx.x == 0, acc,
                dfinal_b, red);
  __syncthreads();
  if (blockIdx.x == 0)
    for (int b = threadIdx.x; b < ns; b += 64 * NW) {
      dy[b] = s_dy[b];
      if (up && r1) up[b] = s_u[b];
      if (rs && r1) rs[b] = s_r[b];
    }
  if (!r1) {
    for (int b = threadIdx.x; b < ns; b += 64 * NW) { s_u[b] = s_dy[b]; s_r[b] = 1.f; }
    __syncthreads();
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long i = ((long)blockIdx.x * 64 + lane) * V;
  float w[V], db[V], dw[V];
#pragma unroll
  for (int k = 0; k < V; ++k) { w[k] = 0.f; db[k] = 0.f; dw[k] = 0.f; }
  if (i < n) {
#pragma unroll
    for (int k4 = 0; k4 < V; k4 += 4) {
      const float4 r = *(const float4*)(wf + i + k4);
      w[k4] = r.x * scale; w[k4 + 1] = r.y * scale; w[k4 + 2] = r.z * scale; w[k4 + 3] = r.w * scale;
    }
    // (round 6) eight samples' loads in flight per lane: with four, one workgroup per CU kept 16 KB in flight and the launch
    // ran at 1.8 TB/s of its 34 MB
    constexpr int NB = 8;
    for (int b0 = wave; b0 < ns; b0 += NW * NB) {
      float a[NB][V];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int b = b0 + NW * j;
        if (b < ns) Vec16<T>::load(d4 + (long)b * n + i, a[j]);
        else {
#pragma unroll
          for (int k = 0; k < V; ++k) a[j][k] = 0.f;
        }
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int b = b0 + NW * j;
        if (b < ns) {
          float g[V];
          const float u = s_u[b], rsb = s_r[b], c = s_dy[b];
#pragma unroll
          for (int k = 0; k < V; ++k) {
            g[k] = u * w[k] * (a[j][k] > 0.f ? SQRT2 : LRELU_SLOPE * SQRT2);
            db[k] += rsb * g[k];
            dw[k] += c * a[j][k];
          }
          Vec16<T>::store(dd4 + (long)b * n + i, g);
        }
      }
    }
  }
  if (dbias) {
#pragma unroll
    for (int k = 0; k < V; ++k) part[wave][lane * V + k] = db[k];
    __syncthreads();
    for (int e = threadIdx.x; e < 64 * V; e += 64 * NW) {
      const long ie = (long)blockIdx.x * 64 * V + e;
      // dbias_part: one partial per element of the map (= per pixel and channel, summed over the samples in a fixed order);
      // the caller sums the n / C pixel rows per channel with dg_wgrad_reduce - no atomics, bit-reproducible
      if (ie < n) {
        float v = part[0][e];
#pragma unroll
        for (int w8 = 1; w8 < NW; ++w8) v += part[w8][e];
        if (dbias_part) dbias_part[ie] = v; else atomicAdd(&dbias[ie % C], v);
      }
    }
  }
  if (dwf) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < V; ++k) part[wave][lane * V + k] = dw[k];
    __syncthreads();
    for (int e = threadIdx.x; e < 64 * V; e += 64 * NW) {
      const long ie = (long)blockIdx.x * 64 * V + e;
      if (ie < n) {
        float v = part[0][e];
#pragma unroll
        for (int w8 = 1; w8 < NW; ++w8) v += part[w8][e];
        dwf[ie] += v * scale;
      }
    }
  }
}

// acc[0] += mean(x[0..n))   (R1 penalty of the micro-batch: mean of the per-sample squared-gradient sums)
__global__ __launch_bounds__(256) void mean_acc_kernel(const float* __restrict__ x, int n, float* __restrict__ acc) {
  __shared__ float red[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += x[i];
  const float t = dg_block_sum(s, red);
  if (threadIdx.x == 0) acc[0] += t / n;
}

// y = a * x
__global__ void scale_kernel(const float* __restrict__ x, float a, long n, float* __restrict__ y) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = a * x[i];
}

__global__ void dg_zero_kernel(float* __restrict__ p, long n) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = 0.f;
}

// several buffers in one launch (a step's accumulator arena and gradient buffers: one graph node instead of three)
struct ZeroItems { float* p[4]; long n[4]; long first[5]; int k; };
__global__ void dg_zero_multi_kernel(ZeroItems z) {
  const long stride = (long)gridDim.x * blockDim.x;
  const long total = z.first[z.k];
  for (long i4 = (long)blockIdx.x * blockDim.x + threadIdx.x; 4 * i4 < total; i4 += stride) {
    const long i = 4 * i4;
    int j = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q)
      if (q < z.k && i >= z.first[q]) j = q;
    *(float4*)(z.p[j] + (i - z.first[j])) = make_float4(0.f, 0.f, 0.f, 0.f);   // (counts are multiples of 4: the launcher pads down)
  }
}

int dg_zero_f32(float* p, long n, hipStream_t s) {
  if (n <= 0) return DG_OK;
  unsigned g = nblk(n);
  if (g > 2048) g = 2048;
  dg_zero_kernel<<<g, 256, 0, s>>>(p, n);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

template <typename DD>
static int head_post_bwd4_launch(DD dd, const float* gout, const float* noise_pixel, const float* noise_image,
                                 const float* mask, int arch, float tau, float drop_const, int B, long HW, float s_depth,
                                 float s_conf, float* draw, float* dbias, void* draw_pm, int cpk, float* bias_ws,
                                 hipStream_t s) {
  const unsigned per = B >= 1024 ? 1u : (unsigned)(1024 / B);
  unsigned hb4 = nblk(HW / 4);
  if (hb4 > per) hb4 = per;
  const dim3 grid4(hb4, B);
#define DG_HPB4(A, C)                                                                                                    \
  head_post_bwd4_kernel<A, C, DD><<<grid4, 256, 0, s>>>(gout, noise_pixel, noise_image, mask, dd, 1.f / tau, drop_const,   \
                                                        B, HW, s_depth, s_conf, draw, dbias, (bf16*)draw_pm, bias_ws)
#define DG_HPB4_A(A) do { if (cpk == 0) DG_HPB4(A, 0); else if (cpk == 2) DG_HPB4(A, 2); else DG_HPB4(A, 4); } while (0)
  if (arch == 0) DG_HPB4_A(0); else if (arch == 1) DG_HPB4_A(1); else DG_HPB4_A(2);
#undef DG_HPB4_A
#undef DG_HPB4
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

extern "C" {

// k <= 4 fp32 buffers (16-byte aligned, counts multiples of 4) zero-filled by one launch
int dg_zero_multi(float* const* ptrs, const long* counts, int k, void* s_) {
  if (!ptrs || !counts || k < 1 || k > 4) return DG_EINVAL;
  ZeroItems z{};
  long tot = 0;
  for (int i = 0; i < k; ++i) {
    if (!ptrs[i] || counts[i] < 0 || counts[i] % 4 != 0 || ((size_t)ptrs[i] & 15) != 0) return DG_EINVAL;
    z.p[i] = ptrs[i]; z.n[i] = counts[i]; z.first[i] = tot;
    tot += counts[i];
  }
  z.first[k] = tot;
  z.k = k;
  if (tot == 0) return DG_OK;
  unsigned g = nblk(tot / 4);
  if (g > 2048) g = 2048;
  dg_zero_multi_kernel<<<g, 256, 0, (hipStream_t)s_>>>(z);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

static int final_fwd_impl(const void* d4, int dtype, const float* wf, const float* bias, float scale, int B, long n, float* y,
                          bool zero, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  if (zero) { const int zrc = dg_zero_f32(y, B, s); if (zrc) return zrc; }
  const DgDet det = dg_det_current();
  const bool vec = vec_ok(d4, n, dtype) && ((size_t)wf & 15) == 0;
  const int V = vec ? (dtype == DG_BF16 ? 8 : 4) : 1;
  unsigned slabs = nblk(n, 256 * 4 * V);
  if (slabs > 32) slabs = 32;
  if (slabs < 1) slabs = 1;
  if (vec) {
    if (dtype == DG_BF16) final_fwd_kernel<bf16><<<dim3(slabs, B), 256, 0, s>>>((const bf16*)d4, wf, bias, scale, n, y, det);
    else final_fwd_kernel<float><<<dim3(slabs, B), 256, 0, s>>>((const float*)d4, wf, bias, scale, n, y, det);
  } else {
    if (dtype == DG_BF16) final_fwd_scalar_kernel<bf16><<<dim3(slabs, B), 256, 0, s>>>((const bf16*)d4, wf, bias, scale, n, y, det);
    else final_fwd_scalar_kernel<float><<<dim3(slabs, B), 256, 0, s>>>((const float*)d4, wf, bias, scale, n, y, det);
  }
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_final_fwd(const void* d4, int dtype, const float* wf, const float* bias, float scale, int B, long n, float* y,
                 void* s_) {
  return final_fwd_impl(d4, dtype, wf, bias, scale, B, n, y, true, s_);
}
// `_acc` forms: the small fp32 accumulator the kernel adds into (y / out / xsum / gsum) was zeroed by the CALLER - a step
// that carves all of them from one buffer zero-fills once instead of once per call (each fill is a ~5 us graph node)
int dg_final_fwd_acc(const void* d4, int dtype, const float* wf, const float* bias, float scale, int B, long n, float* y,
                     void* s_) {
  return final_fwd_impl(d4, dtype, wf, bias, scale, B, n, y, false, s_);
}

int dg_final_bwd_data(const void* d4, int dtype, const float* wf, const float* up, const float* rowscale, float scale,
                      int B, long n, int C, void* dd4, float* dbias, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  const int V = dtype == DG_BF16 ? 8 : 4;
  if (vec_ok(d4, n, dtype) && vec_ok(dd4, n, dtype) && C % V == 0 && B <= 256 && ((size_t)wf & 15) == 0) {
    const unsigned grid = nblk(n / V, 64);
    if (dtype == DG_BF16)
      final_bwd_data_kernel<bf16><<<grid, 256, 0, s>>>((const bf16*)d4, wf, up, rowscale, scale, B, n, C, (bf16*)dd4, dbias);
    else
      final_bwd_data_kernel<float><<<grid, 256, 0, s>>>((const float*)d4, wf, up, rowscale, scale, B, n, C, (float*)dd4, dbias);
  } else if (dtype == DG_BF16) {
    final_bwd_data_scalar_kernel<bf16><<<nblk(n), 256, 0, s>>>((const bf16*)d4, wf, up, rowscale, scale, B, n, C, (bf16*)dd4, dbias);
  } else {
    final_bwd_data_scalar_kernel<float><<<nblk(n), 256, 0, s>>>((const float*)d4, wf, up, rowscale, scale, B, n, C, (float*)dd4, dbias);
  }
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_batch_wsum(const void* src, int dtype, const float* coef, float scale, int B, long n, float* out,
                  void* s_) {
  hipStream_t s = (hipStream_t)s_;
  const int V = dtype == DG_BF16 ? 8 : 4;
  if (vec_ok(src, n, dtype)) {
    const unsigned grid = nblk(n / V, 64);
    if (dtype == DG_BF16) batch_wsum_kernel<bf16><<<grid, 256, 0, s>>>((const bf16*)src, coef, scale, B, n, out);
    else batch_wsum_kernel<float><<<grid, 256, 0, s>>>((const float*)src, coef, scale, B, n, out);
  } else if (dtype == DG_BF16) {
    batch_wsum_scalar_kernel<bf16><<<nblk(n), 256, 0, s>>>((const bf16*)src, coef, scale, B, n, out);
  } else {
    batch_wsum_scalar_kernel<float><<<nblk(n), 256, 0, s>>>((const float*)src, coef, scale, B, n, out);
  }
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

static int head_post_fwd_impl(float* gout, const float* noise_pixel, const float* noise_image, int arch, int training,
                              float tau, float drop_const, int B, long HW, float* mask, float* depth, float* dsum, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  if (arch < 0 || arch > 2) return DG_EINVAL;
  if (dsum && HW % 256 != 0) return DG_EUNSUPPORTED;
  const int chunk = dsum ? sum_chunk(HW) : 256;
  const DgDet det = dg_det_current();
  const unsigned nb = nblk((long)B * HW, chunk);
  if (dsum && chunk % 1024 == 0 && ((size_t)gout & 15) == 0 && ((size_t)depth & 15) == 0 && ((size_t)mask & 15) == 0 &&
      ((size_t)noise_pixel & 15) == 0) {
    if (arch == 0)
      head_post_fwd4_kernel<0><<<nb, 256, 0, s>>>(gout, noise_pixel, noise_image, training, 1.f / tau, drop_const, B, HW, mask, depth, dsum, chunk, det);
    else if (arch == 1)
      head_post_fwd4_kernel<1><<<nb, 256, 0, s>>>(gout, noise_pixel, noise_image, training, 1.f / tau, drop_const, B, HW, mask, depth, dsum, chunk, det);
    else
      head_post_fwd4_kernel<2><<<nb, 256, 0, s>>>(gout, noise_pixel, noise_image, training, 1.f / tau, drop_const, B, HW, mask, depth, dsum, chunk, det);
    HIP_CHECK_RET(hipGetLastError());
    return DG_OK;
  }
  if (arch == 0)
    head_post_fwd_kernel<0><<<nb, 256, 0, s>>>(gout, noise_pixel, noise_image, training, 1.f / tau, drop_const, B, HW, mask, depth, dsum, chunk, det);
  else if (arch == 1)
    head_post_fwd_kernel<1><<<nb, 256, 0, s>>>(gout, noise_pixel, noise_image, training, 1.f / tau, drop_const, B, HW, mask, depth, dsum, chunk, det);
  else
    head_post_fwd_kernel<2><<<nb, 256, 0, s>>>(gout, noise_pixel, noise_image, training, 1.f / tau, drop_const, B, HW, mask, depth, dsum, chunk, det);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}
int dg_head_post_fwd(float* gout, const float* noise_pixel, const float* noise_image, int arch, int training,
                     float tau, float drop_const, int B, long HW, float* mask, float* depth, void* s_) {
  return head_post_fwd_impl(gout, noise_pixel, noise_image, arch, training, tau, drop_const, B, HW, mask, depth, nullptr, s_);
}
// ... + dsum[b] += sum of depth[b] (dsum zeroed by the caller; HW % 256 == 0 or DG_EUNSUPPORTED): the per-sample sums
// that dg_diffaug_fwd_pre takes instead of making its own pass over the image
int dg_head_post_fwd_sum(float* gout, const float* noise_pixel, const float* noise_image, int arch, int training,
                         float tau, float drop_const, int B, long HW, float* mask, float* depth, float* dsum, void* s_) {
  if (!dsum) return DG_EINVAL;
  return head_post_fwd_impl(gout, noise_pixel, noise_image, arch, training, tau, drop_const, B, HW, mask, depth, dsum, s_);
}

int dg_head_post_bwd(const float* gout, const float* noise_pixel, const float* noise_image, const float* mask,
                     const float* ddepth, int arch, float tau, float drop_const, int B, long HW, float s_depth,
                     float s_conf, float* draw, float* dbias, void* draw_pm, int cp, float* bias_ws,
                     void* s_) {
  hipStream_t s = (hipStream_t)s_;
  if (arch < 0 || arch > 2) return DG_EINVAL;
  unsigned hb = nblk(HW);                        // blocks per sample: ~1024 blocks in all, each one atomic per head
  const unsigned per = B >= 1024 ? 1u : (unsigned)(1024 / B);
  if (hb > per) hb = per;
  const dim3 grid(hb, B);
  const int cpk = !draw_pm ? 0 : (cp == 2 ? 2 : (cp == 4 ? 4 : 1));
  if (!draw && !draw_pm) return DG_EINVAL;
  auto al = [](const void* q) { return ((size_t)q & 15) == 0; };
  if (HW % 4 == 0 && cpk != 1 && al(gout) && al(ddepth) && al(draw) && al(draw_pm) && al(noise_pixel) && al(mask))
    return head_post_bwd4_launch(HeadGradPlain{ddepth}, gout, noise_pixel, noise_image, mask, arch, tau, drop_const, B, HW,
                                 s_depth, s_conf, draw, dbias, draw_pm, cpk, bias_ws, s);
  if (!draw) return DG_EUNSUPPORTED;   // (the scalar kernel always writes the planar copy)
#define DG_HPB(A, C)                                                                                                   \
  head_post_bwd_kernel<A, C><<<grid, 256, 0, s>>>(gout, noise_pixel, noise_image, mask, ddepth, 1.f / tau, drop_const, \
                                                  B, HW, s_depth, s_conf, draw, dbias, (bf16*)draw_pm, cp)
#define DG_HPB_A(A)                                                                                  \
  do {                                                                                               \
    if (cpk == 0) DG_HPB(A, 0); else if (cpk == 2) DG_HPB(A, 2); else if (cpk == 4) DG_HPB(A, 4); else DG_HPB(A, 1); \
  } while (0)
  if (arch == 0) DG_HPB_A(0); else if (arch == 1) DG_HPB_A(1); else DG_HPB_A(2);
#undef DG_HPB_A
#undef DG_HPB
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
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
  if (arch < 0 || arch > 2 || !gy || B <= 0 || H <= 0 || W <= 1) return DG_EINVAL;
  if (!draw && !draw_pm) return DG_EINVAL;
  if ((policy & 4) && !gsum) return DG_EINVAL;
  const int cpk = !draw_pm ? 0 : (cp == 2 ? 2 : (cp == 4 ? 4 : 1));
  auto al = [](const void* q) { return ((size_t)q & 15) == 0; };
  if (!(W % 4 == 0 && cpk != 1 && al(gout) && al(draw) && al(draw_pm) && al(noise_pixel) && al(mask))) return DG_EUNSUPPORTED;
  HeadGradAug dd{make_aug(u_b, u_c, t_h, t_w, o_x, o_y, policy, B, H, W), gy, gsum};
  return head_post_bwd4_launch(dd, gout, noise_pixel, noise_image, mask, arch, tau, drop_const, B, (long)H * W, s_depth,
                               s_conf, draw, dbias, draw_pm, cpk, bias_ws, (hipStream_t)s_);
}

int dg_nsgan_d(const float* y_real, const float* y_fake, int B, float w_gan, float* dy_real, float* dy_fake,
               float* scal, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  nsgan_d_kernel<<<1, 256, 0, s>>>(y_real, y_fake, B, w_gan, dy_real, dy_fake, scal);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_nsgan_g(const float* y_fake, int B, float w_gan, float* dy, float* scal, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  nsgan_g_kernel<<<1, 256, 0, s>>>(y_fake, B, w_gan, dy, scal);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_scale(const float* x, float a, long n, float* y, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  scale_kernel<<<nblk(n), 256, 0, s>>>(x, a, n, y);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_nsgan_d_step(const float* y_real, const float* y_fake, int B, float w_gan, float* dy, float* up, float* rs,
                    float* acc, float* dfinal_b, void* s_) {
  if (!y_real || !y_fake || !dy || !acc || B <= 0) return DG_EINVAL;
  nsgan_d_step_kernel<<<1, 256, 0, (hipStream_t)s_>>>(y_real, y_fake, B, w_gan, dy, up, rs, acc, dfinal_b);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_nsgan_g_step(const float* y_fake, int B, float w_gan, float* dy, float* acc, void* s_) {
  if (!y_fake || !dy || !acc || B <= 0) return DG_EINVAL;
  nsgan_g_step_kernel<<<1, 256, 0, (hipStream_t)s_>>>(y_fake, B, w_gan, dy, acc);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_gan_d_step(int metric, float smoothing, const float* y_real, const float* y_fake, int B, float w_gan,
                  float* dy, float* up, float* rs, float* acc, float* dfinal_b, void* s_) {
  if (!y_real || !y_fake || !dy || !acc || B <= 0) return DG_EINVAL;
  GanForm fm;
  const int rc = gan_form(metric, 0, smoothing, &fm);
  if (rc != DG_OK) return rc;
  gan_step_kernel<<<1, 256, 0, (hipStream_t)s_>>>(fm, 0, y_real, y_fake, B, w_gan, dy, up, rs, acc, dfinal_b);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_gan_g_step(int metric, const float* y_real, const float* y_fake, int B, float w_gan, float* dy, float* acc,
                  void* s_) {
  if (!y_fake || !dy || !acc || B <= 0) return DG_EINVAL;
  GanForm fm;
  const int rc = gan_form(metric, 1, 1.f, &fm);
  if (rc != DG_OK) return rc;
  if (fm.kr != PHI_NONE && !y_real) return DG_EINVAL;  // relativistic metrics read D(real) (models/loss.py:76-85)
  gan_step_kernel<<<1, 256, 0, (hipStream_t)s_>>>(fm, 1, y_real, y_fake, B, w_gan, dy, nullptr, nullptr, acc,
                                                  nullptr);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

// dg_gan_d_step / dg_gan_g_step + dg_final_bwd_data (+ dg_batch_wsum with coef = dy when dwf is given) in one launch.
// DG_EUNSUPPORTED (nothing launched) unless the 16-byte forms apply and the samples fit the kernel's per-sample tables:
// the caller then issues the separate calls.
int dg_final_gan_bwd(int metric, int mode_g, float smoothing, const float* y_real, const float* y_fake, int B, float w_gan,
                     int r1, float* dy, float* up, float* rs, float* acc, float* dfinal_b, const void* d4, int dtype,
                     const float* wf, float scale, long n, int C, void* dd4, float* dbias, float* dwf, float* dbias_part,
                     void* s_) {
  if (!y_fake || !dy || !acc || !d4 || !wf || !dd4 || B <= 0 || n <= 0) return DG_EINVAL;
  if (dbias_part && (!dbias || n % C != 0)) return DG_EINVAL;
  if (!mode_g && !y_real) return DG_EINVAL;
  GanForm fm;
  const int rc = gan_form(metric, mode_g ? 1 : 0, mode_g ? 1.f : smoothing, &fm);
  if (rc != DG_OK) return rc;
  if (mode_g && fm.kr != PHI_NONE && !y_real) return DG_EINVAL;
  if (mode_g && r1) return DG_EINVAL;
  const int ns = mode_g ? B : 2 * B;
  const int V = dtype == DG_BF16 ? 8 : 4;
  if (!(vec_ok(d4, n, dtype) && vec_ok(dd4, n, dtype) && C % V == 0 && ns <= 256 && ((size_t)wf & 15) == 0 &&
        (!dwf || ((size_t)dwf & 15) == 0)))
    return DG_EUNSUPPORTED;
  const unsigned grid = nblk(n / V, 64);
  hipStream_t s = (hipStream_t)s_;
  if (dtype == DG_BF16)
    final_gan_bwd_kernel<bf16><<<grid, 512, 0, s>>>(fm, mode_g ? 1 : 0, y_real, y_fake, B, w_gan, r1, dy, up, rs, acc, dfinal_b,
                                                    (const bf16*)d4, wf, scale, n, C, (bf16*)dd4, dbias, dwf, dbias_part);
  else
    final_gan_bwd_kernel<float><<<grid, 512, 0, s>>>(fm, mode_g ? 1 : 0, y_real, y_fake, B, w_gan, r1, dy, up, rs, acc, dfinal_b,
                                                     (const float*)d4, wf, scale, n, C, (float*)dd4, dbias, dwf, dbias_part);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_head_post_bwd2(const float* gout, const float* noise_pixel, const float* noise_image, const float* mask,
                      const float* ddepth, const float* thead, int arch, float tau, float drop_const, int B, long HW,
                      float s_depth, float s_conf, float* draw, float* dbias, void* draw_pm, int cp, void* s_) {
  if (!gout || !ddepth || !thead || !draw || B <= 0 || HW <= 0 || arch < 0 || arch > 2) return DG_EINVAL;
  if (arch >= 1 && (!noise_pixel || !mask)) return DG_EINVAL;
  if (arch == 2 && !noise_image) return DG_EINVAL;
  const long n = (long)B * HW;
  const int hb = (int)min((long)1024, (n + 255) / 256);
  head_post_bwd2_kernel<<<hb, 256, 0, (hipStream_t)s_>>>(gout, noise_pixel, noise_image, mask, ddepth, thead, arch,
                                                         1.f / tau, drop_const, B, HW, s_depth, s_conf, draw, dbias,
                                                         (bf16*)draw_pm, cp);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_pl_penalty(const float* dz, int B, int K, float w, float* pl_ema, float* v, float* acc, void* s_) {
  if (!dz || !pl_ema || !v || !acc || B <= 0 || B > 256 || K <= 0) return DG_EINVAL;
  pl_penalty_kernel<<<1, 256, 0, (hipStream_t)s_>>>(dz, B, K, w, pl_ema, v, acc);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_mean_acc(const float* x, int n, float* acc, void* s_) {
  if (!x || !acc || n <= 0) return DG_EINVAL;
  mean_acc_kernel<<<1, 256, 0, (hipStream_t)s_>>>(x, n, acc);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

}  // extern "C"

// ---- deterministic sums: the accumulator arena and its shadow (common.h dg_acc_add) ----------------------------------------
// One entry per device, on the HOST: every kernel that sums into arena slots takes its device's entry by value as a kernel
// argument (dg_det_current, read by the launcher), so such kernels live in whatever file suits them.  The arena is allocated
// once per device for the life of the process (_lib.AccArena._for_device), so a captured graph that bakes the entry into its
// kernel arguments is as valid as one that bakes in the arena pointers it already holds.
#define DG_DET_MAX_DEVICES 64
static DgDet g_det_table[DG_DET_MAX_DEVICES];   // zero: nothing registered - dg_acc_add falls back to float atomics
DgDet dg_det_current() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= DG_DET_MAX_DEVICES) return DgDet{nullptr, nullptr, 0};
  return g_det_table[dev];
}
extern "C" int dg_det_arena(float* arena, long n, void* shadow) {
  if ((arena == nullptr) != (shadow == nullptr) || n < 0) return DG_EINVAL;
  if (shadow && ((size_t)shadow & 15) != 0) return DG_EINVAL;
  int dev = 0;
  HIP_CHECK_RET(hipGetDevice(&dev));
  if (dev < 0 || dev >= DG_DET_MAX_DEVICES) return DG_EINVAL;
  g_det_table[dev] = DgDet{arena, (unsigned long long*)shadow, arena ? n : 0};
  return DG_OK;
}
