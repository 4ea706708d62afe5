// Multi-code GAN inversion (mGANprior; reference: demo.py:353-366, 466-488, 523-530), gfx950: N latents per scan run through
// the generator's lower layers, their feature maps at one layer are blended per channel with learnable weights alpha, and the
// blend runs through the rest of the generator as ONE sample.  Feature maps are the engine's pixel-major buffers
// [sample][pixel][channel]; code n of scan s is lower-batch row s N + n.
//   * feat_compose_kernel     : abar[s,p,c] = sum_n alpha[s,n,c] a[s N + n, p, c], fp32 in code order, one rounding on the store
//   * feat_compose_bwd_kernel : dpre[s N + n,p,c] = g[s,p,c] alpha[s,n,c] lrelu'(a[s N + n,p,c])  (the factor of the conv kernels'
//                               EPI_MASK epilogue, dg_epilogue of common.h) and dalpha[s,n,c] = sum_p g[s,p,c] a[s N + n,p,c]
//   * alpha_adam_kernel       : torch.optim.Adam on alpha at the device step index, the step's scalars from a host-made table
// All three stream their operands once: bandwidth-bound, 16-byte (fp32) / 16- or 8-byte (bf16) accesses, no LDS staging.
// dalpha's sum over pixels has a fixed order: a thread walks its pixels in order, the rows of a workgroup are added in row order
// (LDS), the workgroups of one (s, n) in chunk order by the one that draws the last ticket (common.h) - run to run, and a
// replayed graph against the eager loop, the bits are the same.
#include "adam.h"

namespace {

constexpr int FC_THREADS = 256;

template <typename T, int V>
struct alignas(sizeof(T) * V < 16 ? sizeof(T) * V : 16) Vec {
  T v[V];
};

template <typename T, int V>
__device__ __forceinline__ void ld_vec(const T* p, float (&x)[V]) {
  const Vec<T, V> r = *(const Vec<T, V>*)p;
#pragma unroll
  for (int i = 0; i < V; ++i) x[i] = (float)r.v[i];
}
template <typename T, int V>
__device__ __forceinline__ void st_vec(T* p, const float (&x)[V]) {
  Vec<T, V> r;
#pragma unroll
  for (int i = 0; i < V; ++i) r.v[i] = (T)x[i];
  *(Vec<T, V>*)p = r;
}

// grid (chunks of the sample's P C / V vectors, B).  PC = P C: a sample's elements, the same offsets in every lower row and in abar
template <typename T, int V>
__global__ __launch_bounds__(FC_THREADS) void feat_compose_kernel(const T* __restrict__ a, const float* __restrict__ alpha,
                                                                  T* __restrict__ out, int N, long PC, int C) {
  const int s = blockIdx.y;
  const long nvec = PC / V;
  const T* as = a + (long)s * N * PC;
  const float* al = alpha + (long)s * N * C;
  T* o = out + (long)s * PC;
  for (long e = (long)blockIdx.x * FC_THREADS + threadIdx.x; e < nvec; e += (long)gridDim.x * FC_THREADS) {
    const long off = e * V;
    const int c = (int)((unsigned)off % (unsigned)C);   // (P C < 2^31: a 32-bit remainder)
    float acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = 0.f;
    for (int n = 0; n < N; ++n) {
      float x[V], w[V];
      ld_vec<T, V>(as + (long)n * PC + off, x);
      ld_vec<float, V>(al + (long)n * C + c, w);
#pragma unroll
      for (int i = 0; i < V; ++i) acc[i] = __fmaf_rn(w[i], x[i], acc[i]);
    }
    st_vec<T, V>(o + off, acc);
  }
}

// grid (nchunk, N, B); a workgroup = R pixel rows x CT channel vectors (R CT <= FC_THREADS), its pixel chunk walked R rows at
// a time, channel tiles of CT vectors one after the other.  parts [B N][nchunk][C] and tickets [B N]: zero on entry, left zero.
template <typename T, int V>
__global__ __launch_bounds__(FC_THREADS) void feat_compose_bwd_kernel(const T* __restrict__ g, const T* __restrict__ a,
                                                                      const float* __restrict__ alpha, T* __restrict__ dpre,
                                                                      float* __restrict__ dalpha, float* __restrict__ parts,
                                                                      unsigned* __restrict__ tickets, int N, int P, int C) {
  __shared__ float red[FC_THREADS * V];
  const int n = blockIdx.y, s = blockIdx.z, nch = gridDim.x;
  const long row = (long)s * N + n;
  const int CV = C / V;                                  // channel vectors of a pixel
  const int CT = CV < FC_THREADS ? CV : FC_THREADS;      // ... of a channel tile
  const int R = FC_THREADS / CT;
  const int tid = threadIdx.x, r = tid / CT, j = tid - r * CT;
  const bool rows = r < R;                               // (threads beyond R CT idle in the walk)
  const int chunk = (P + nch - 1) / nch;
  const int p0 = blockIdx.x * chunk, p1 = min(P, p0 + chunk);
  const T* gs = g + (long)s * P * C;
  const T* ar = a + row * P * C;
  T* dr = dpre + row * P * C;
  const float* al = alpha + row * C;
  float* part = parts + (row * nch + blockIdx.x) * C;
  for (int c0 = 0; c0 < CV; c0 += CT) {
    const int cv = c0 + j;
    const bool on = rows && cv < CV;
    float acc[V], wp[V], wn[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = 0.f;
    if (on) {
      float w[V];
      ld_vec<float, V>(al + cv * V, w);
#pragma unroll
      for (int i = 0; i < V; ++i) {                      // alpha times the two values of dg_epilogue's EPI_MASK factor
        wp[i] = w[i] * SQRT2;
        wn[i] = w[i] * (LRELU_SLOPE * SQRT2);
      }
      for (int p = p0 + r; p < p1; p += R) {
        const long off = (long)p * C + cv * V;
        float gv[V], av[V], d[V];
        ld_vec<T, V>(gs + off, gv);
        ld_vec<T, V>(ar + off, av);
#pragma unroll
        for (int i = 0; i < V; ++i) {
          d[i] = gv[i] * (av[i] > 0.f ? wp[i] : wn[i]);
          acc[i] = __fmaf_rn(gv[i], av[i], acc[i]);
        }
        st_vec<T, V>(dr + off, d);
      }
    }
    // the workgroup's rows in row order
    __syncthreads();
    if (on) {
#pragma unroll
      for (int i = 0; i < V; ++i) red[(r * CT + j) * V + i] = acc[i];
    }
    __syncthreads();
    if (on && r == 0) {
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float t = acc[i];
        for (int q = 1; q < R; ++q) t += red[(q * CT + j) * V + i];
        if (nch == 1) dalpha[row * C + cv * V + i] = t;
        else atomicExch(&part[cv * V + i], t);           // memory-side, as the last workgroup's reads below
      }
    }
  }
  if (nch == 1) return;
  if (!dg_block_ticket_last(&tickets[row], nch)) return;
  for (int c = tid; c < C; c += FC_THREADS) {
    float t = 0.f;
    for (int q = 0; q < nch; ++q) t += atomicExch(&parts[(row * nch + q) * C + c], 0.f);
    dalpha[row * C + c] = t;
  }
}

// torch.optim.Adam (defaults; single-tensor form) on n elements at step index k = *step: sched [num_step + 1][3] holds per step
// lr(k) / (1 - beta1^(k+1)) and sqrt(1 - beta2^(k+1)) (the third column is the latent optimiser's), row num_step for k beyond it
__global__ __launch_bounds__(FC_THREADS) void alpha_adam_kernel(const float* __restrict__ grad, float* __restrict__ x,
                                                                float* __restrict__ m, float* __restrict__ v,
                                                                const unsigned long long* __restrict__ step,
                                                                const float* __restrict__ sched, int num_step, float beta1,
                                                                float beta2, float eps, long n) {
  const long i = (long)blockIdx.x * FC_THREADS + threadIdx.x;
  if (i >= n) return;
  const int k = (int)*(volatile const unsigned long long*)step;
  const float* sk = sched + 3 * min(k, num_step);
  const float step_size = sk[0], bc2s = sk[1];
  adam_torch_apply(grad[i], m[i], v[i], x[i], step_size, bc2s, 1.f - beta1, beta2, 1.f - beta2, eps);
}

// the widest vector the channel count and the pointers allow: 16 bytes, 8 bytes (bf16), else single elements
template <typename T>
int pick_vec(int C, size_t ptr_bits) {
  if (sizeof(T) == 2 && C % 8 == 0 && (ptr_bits & 15) == 0) return 8;
  if (C % 4 == 0 && (ptr_bits & (4 * sizeof(T) - 1)) == 0) return 4;
  return 1;
}

template <typename T>
int compose_launch(const void* a, const float* alpha, void* out, int B, int N, int P, int C, hipStream_t st) {
  const long PC = (long)P * C;
  const size_t bits = (size_t)a | (size_t)out | (PC * sizeof(T));
  int V = pick_vec<T>(C, bits);
  if (((size_t)alpha & 15) != 0) V = 1;
  const long nvec = PC / V;
  long gx = (nvec + FC_THREADS - 1) / FC_THREADS;
  // enough workgroups for 8 per compute unit over the whole launch, a few vectors per thread otherwise
  const long want = (2048 + B - 1) / B;
  if (gx > want) gx = want;
  const dim3 grid((unsigned)gx, (unsigned)B);
  const T* ap = (const T*)a;
  T* op = (T*)out;
  if (V == 8) {
    if constexpr (sizeof(T) == 2) feat_compose_kernel<T, 8><<<grid, FC_THREADS, 0, st>>>(ap, alpha, op, N, PC, C);
  } else if (V == 4) feat_compose_kernel<T, 4><<<grid, FC_THREADS, 0, st>>>(ap, alpha, op, N, PC, C);
  else feat_compose_kernel<T, 1><<<grid, FC_THREADS, 0, st>>>(ap, alpha, op, N, PC, C);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

template <typename T>
int compose_bwd_launch(const void* g, const void* a, const float* alpha, void* dpre, float* dalpha, float* parts,
                       unsigned* tickets, int B, int N, int P, int C, int nchunk, hipStream_t st) {
  const long PC = (long)P * C;
  const size_t bits = (size_t)g | (size_t)a | (size_t)dpre | (PC * sizeof(T));
  int V = pick_vec<T>(C, bits);
  if (((size_t)alpha & 15) != 0) V = 1;
  const dim3 grid((unsigned)nchunk, (unsigned)N, (unsigned)B);
  const T *gp = (const T*)g, *ap = (const T*)a;
  T* dp = (T*)dpre;
  if (V == 8) {
    if constexpr (sizeof(T) == 2)
      feat_compose_bwd_kernel<T, 8><<<grid, FC_THREADS, 0, st>>>(gp, ap, alpha, dp, dalpha, parts, tickets, N, P, C);
  } else if (V == 4)
    feat_compose_bwd_kernel<T, 4><<<grid, FC_THREADS, 0, st>>>(gp, ap, alpha, dp, dalpha, parts, tickets, N, P, C);
  else
    feat_compose_bwd_kernel<T, 1><<<grid, FC_THREADS, 0, st>>>(gp, ap, alpha, dp, dalpha, parts, tickets, N, P, C);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

bool compose_shape_ok(int B, int N, int P, int C) { return B > 0 && N > 0 && P > 0 && C > 0; }

}  // namespace

extern "C" {

int dg_feat_compose(const void* a, const float* alpha, void* out, int dtype, int B, int N, int P, int C, void* s_) {
  if (!a || !alpha || !out || !compose_shape_ok(B, N, P, C)) return DG_EINVAL;
  if (dtype != DG_F32 && dtype != DG_BF16) return DG_EINVAL;
  if (B > 65535 || N > 65535 || (long)P * C > 0x7fffffffL) return DG_EUNSUPPORTED;
  return dtype == DG_BF16 ? compose_launch<bf16>(a, alpha, out, B, N, P, C, (hipStream_t)s_)
                          : compose_launch<float>(a, alpha, out, B, N, P, C, (hipStream_t)s_);
}

int dg_feat_compose_bwd(const void* g, const void* a, const float* alpha, void* dpre, float* dalpha, float* parts,
                        unsigned* tickets, int nchunk, int dtype, int B, int N, int P, int C, void* s_) {
  if (!g || !a || !alpha || !dpre || !dalpha || !compose_shape_ok(B, N, P, C)) return DG_EINVAL;
  if (dtype != DG_F32 && dtype != DG_BF16) return DG_EINVAL;
  if (nchunk < 1 || nchunk > P || nchunk > 65535) return DG_EINVAL;
  if (nchunk > 1 && (!parts || !tickets)) return DG_EINVAL;
  if (B > 65535 || N > 65535 || (long)P * C > 0x7fffffffL) return DG_EUNSUPPORTED;
  return dtype == DG_BF16
             ? compose_bwd_launch<bf16>(g, a, alpha, dpre, dalpha, parts, tickets, B, N, P, C, nchunk, (hipStream_t)s_)
             : compose_bwd_launch<float>(g, a, alpha, dpre, dalpha, parts, tickets, B, N, P, C, nchunk, (hipStream_t)s_);
}

int dg_alpha_adam(const float* grad, float* alpha, float* m, float* v, const unsigned long long* step_dev, const float* sched,
                  int num_step, float beta1, float beta2, float eps, long n, void* s_) {
  if (!grad || !alpha || !m || !v || !step_dev || !sched || num_step <= 0 || n <= 0) return DG_EINVAL;
  alpha_adam_kernel<<<(unsigned)((n + FC_THREADS - 1) / FC_THREADS), FC_THREADS, 0, (hipStream_t)s_>>>(
      grad, alpha, m, v, step_dev, sched, num_step, beta1, beta2, eps, n);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

}  // extern "C"
