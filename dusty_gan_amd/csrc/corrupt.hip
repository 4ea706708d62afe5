// The target corruptions of the reference's restoration experiment (demo.py:71-137), as kernels (gfx950).  The demo degrades
// the scan it inverts against - additive noise, 1/8 of the rows, 90 % dropout, or a morphological closing - and compares
// the inversion with the full scan.  All images are fp32 [B,1,H,W], contiguous.
//   * corrupt_mask_kernel   : mask * row_keep[h] * col_keep[w] * (u < rate): dropout_noise, sparse_hlines / sparse_vlines,
//     random_lines, corrupt_half, corrupt_quarter (demo.py:71-108) are one body; the host builds the keep vectors.
//   * additive_noise_kernel : depth + noise * strength (demo.py:111-113), two fp32 roundings.
//   * median3x3_kernel      : kornia.filters.median_blur(x, (3, 3)) as closing calls it (demo.py:117): nine taps, zeros
//     outside the image, the 5th smallest - a 19-exchange selection network.
//   * hole_fill_kernel      : the `while` loop of closing (demo.py:118-123) with a guaranteed end, one workgroup per sample.
// Every result is a selection, a maximum, a product with 0 / 1 or two correctly rounded operations: bit-exact against torch.
#include "common.h"

namespace {

inline int nblk(long n) { return (int)((n + 255) / 256); }

__global__ __launch_bounds__(256) void corrupt_mask_kernel(const float* mask, const float* __restrict__ row_keep,
                                                           const float* __restrict__ col_keep, const float* __restrict__ u,
                                                           float rate, long n, int H, int W, float* out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float m = mask[i];
  if (row_keep) m *= row_keep[(i / W) % H];
  if (col_keep) m *= col_keep[i % W];
  if (u) m *= u[i] < rate ? 1.f : 0.f;   // (noise < rate).float()
  out[i] = m;
}

__global__ __launch_bounds__(256) void additive_noise_kernel(const float* x, const float* __restrict__ noise, float strength,
                                                             long n, float* out) {
#pragma clang fp contract(off)   // randn * strength is rounded to fp32 before the add (demo.py:112-113): never one FMA.  Plain
                                 // operators: hipcc fuses HIP's __fadd_rn(x, __fmul_rn(..)) wrappers into v_fmac_f32 (seen in the ISA)
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float scaled = noise[i] * strength;
  out[i] = x[i] + scaled;
}

__device__ __forceinline__ void cswap(float& a, float& b) {
  const float lo = fminf(a, b), hi = fmaxf(a, b);
  a = lo;
  b = hi;
}

// median of nine: the 19-exchange network (Paeth, Graphics Gems I), p[4] ends as the 5th smallest
__device__ __forceinline__ float median9(float* p) {
  cswap(p[1], p[2]); cswap(p[4], p[5]); cswap(p[7], p[8]);
  cswap(p[0], p[1]); cswap(p[3], p[4]); cswap(p[6], p[7]);
  cswap(p[1], p[2]); cswap(p[4], p[5]); cswap(p[7], p[8]);
  cswap(p[0], p[3]); cswap(p[5], p[8]); cswap(p[4], p[7]);
  cswap(p[3], p[6]); cswap(p[1], p[4]); cswap(p[2], p[5]);
  cswap(p[4], p[7]); cswap(p[4], p[2]); cswap(p[6], p[4]);
  cswap(p[4], p[2]);
  return p[4];
}

__global__ __launch_bounds__(256) void median3x3_kernel(const float* __restrict__ x, long n, int H, int W,
                                                        float* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int w = (int)(i % W), h = (int)((i / W) % H);
  float p[9];
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int hh = h + dy, ww = w + dx;
      const bool in = hh >= 0 && hh < H && ww >= 0 && ww < W;
      p[(dy + 1) * 3 + dx + 1] = in ? x[i + (long)dy * W + dx] : 0.f;   // zero padding (F.pad's default mode in kornia)
    }
  out[i] = median9(p);
}

// One workgroup per sample; the image ping-pongs between x and tmp in global memory (256 KB at 64x1024: L2-resident), one
// Jacobi sweep per barrier: every pixel of sweep k reads the buffer sweep k - 1 wrote.  A sweep that fills nothing is
// discarded (its source is the result), so an all-hole sample comes back as it went in.  The sample stops when no hole
// is left, when a sweep fills nothing, or after `cap` sweeps - all three decided from LDS counters every thread reads alike.
__global__ __launch_bounds__(1024) void hole_fill_kernel(float* x, float* tmp, int H, int W, float thresh, int cap,
                                                         int* __restrict__ sweeps, int* __restrict__ left) {
  __shared__ int s_holes[3], s_filled[3];   // slot k % 3 counts sweep k; slot (k + 1) % 3 is zeroed meanwhile (last read two barriers ago)
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int HW = H * W;
  float* src = x + (long)b * HW;
  float* dst = tmp + (long)b * HW;
  if (tid < 3) s_holes[tid] = s_filled[tid] = 0;
  __syncthreads();
  int nsweep = 0, nleft = 0;
  for (int k = 0; k < cap; ++k) {
    const int slot = k % 3;
    int holes = 0, filled = 0;
    for (int p = tid; p < HW; p += nt) {
      float v = src[p];
      if (v <= thresh) {
        const int h = p / W, w = p - h * W;
        const int h0 = h > 0 ? h - 1 : 0, h1 = h < H - 1 ? h + 1 : H - 1;
        const int w0 = w > 0 ? w - 1 : 0, w1 = w < W - 1 ? w + 1 : W - 1;
        float m = v;   // the window includes the centre; taps outside the image are ignored (max_pool2d pads with -inf)
        for (int hh = h0; hh <= h1; ++hh)
          for (int ww = w0; ww <= w1; ++ww) {
            const float t = src[hh * W + ww];
            m = t > m ? t : m;
          }
        ++holes;
        filled += m > thresh ? 1 : 0;
        v = m;
      }
      dst[p] = v;
    }
    if (holes) atomicAdd(&s_holes[slot], holes);
    if (filled) atomicAdd(&s_filled[slot], filled);
    if (tid == 0) s_holes[(k + 1) % 3] = s_filled[(k + 1) % 3] = 0;
    __syncthreads();   // dst complete and visible to the workgroup; the counters final
    const int nh = s_holes[slot], nf = s_filled[slot];
    nleft = nh;
    if (nf == 0) break;   // nothing filled: no hole, or no pixel above thresh to fill from (the reference loops for ever)
    ++nsweep;
    nleft = nh - nf;
    float* t = src;
    src = dst;
    dst = t;
    if (nleft == 0) break;
  }
  if (src != x + (long)b * HW)   // an odd number of kept sweeps: the result is in tmp
    for (int p = tid; p < HW; p += nt) dst[p] = src[p];
  if (tid == 0) {
    sweeps[b] = nsweep;
    left[b] = nleft;
  }
}

}  // namespace

extern "C" {

int dg_corrupt_mask(const float* mask, const float* row_keep, const float* col_keep, const float* u, float rate, int B, int H,
                    int W, float* out, void* s_) {
  if (!mask || !out || B <= 0 || H <= 0 || W <= 0) return DG_EINVAL;
  const long n = (long)B * H * W;
  corrupt_mask_kernel<<<nblk(n), 256, 0, (hipStream_t)s_>>>(mask, row_keep, col_keep, u, rate, n, H, W, out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_additive_noise(const float* x, const float* noise, float strength, long n, float* out, void* s_) {
  if (!x || !noise || !out || n <= 0) return DG_EINVAL;
  additive_noise_kernel<<<nblk(n), 256, 0, (hipStream_t)s_>>>(x, noise, strength, n, out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_median3x3(const float* x, int B, int H, int W, float* out, void* s_) {
  if (!x || !out || x == out || B <= 0 || H <= 0 || W <= 0) return DG_EINVAL;
  const long n = (long)B * H * W;
  median3x3_kernel<<<nblk(n), 256, 0, (hipStream_t)s_>>>(x, n, H, W, out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_hole_fill(float* x, float* tmp, int B, int H, int W, float thresh, int* sweeps, int* left, void* s_) {
  if (!x || !tmp || x == tmp || !sweeps || !left || B <= 0 || H <= 0 || W <= 0) return DG_EINVAL;
  if ((long)H * W > (1L << 18)) return DG_EUNSUPPORTED;
  const int HW = H * W;
  const int threads = HW >= 1024 ? 1024 : (HW + 63) / 64 * 64;
  // a valid pixel reaches every other within max(H, W) - 1 sweeps (Chebyshev distance); at least one, which counts the holes
  const int cap = (H > W ? H : W) - 1 > 1 ? (H > W ? H : W) - 1 : 1;
  hole_fill_kernel<<<B, threads, 0, (hipStream_t)s_>>>(x, tmp, H, W, thresh, cap, sweeps, left);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

}  // extern "C"
