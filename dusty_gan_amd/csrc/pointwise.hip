// HBM-bound kernels of the step's network end: the final (4 x w0) dot, the GAN losses, the path-length penalty, small reductions
// and zero-fills; and the registration of the accumulator arena.  (Head post-processing: head_post.hip; BlurVH, DiffAugment and
// sample_sum: blur_aug.hip; fetch_reals: step_inputs.hip.)  Images are fp32 [B,1,H,W]; feature maps are T.
#include "pointwise.h"

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
// Path-length regularisation (trainers/dcgan_amp.py:268-306), the pieces that are not convolutions (its second-order
// head post-processing: head_post.hip).
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
// The GAN losses' scalar functions.
__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(__expf(x)); }
__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + __expf(-x)); }

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

// One block.  D mode (mode_g = 0): dy = [d/dy_real | d/dy_fake] of w_gan * loss; the two per-sample vectors the R1 schedule
// feeds the backward with (up = [1 .. 1 | dy_fake], rs = [dy_real | 1 .. 1]; either may be null); acc[0..2] += (mean y_real,
// mean y_fake, loss); dfinal_b += sum dy (the final conv's bias gradient; may be null).  G mode: only the fake half carries a gradient (D(real) is data, trainers/dcgan_amp.py:259);
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

int dg_scale(const float* x, float a, long n, float* y, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  scale_kernel<<<nblk(n), 256, 0, s>>>(x, a, n, y);
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
