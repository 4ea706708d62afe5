// The synthesis command's two kernels (gfx950; dusty_gan_amd/synthesis.py):
//   * latent_walk_kernel   : n latents on the line (lerp) or the great-circle-like arc (slerp) between two endpoints,
//     utils/interp.py:4-16 at the weights of torch.linspace(0, 1, n) (demo.py:278-293).  One workgroup: the two norms and
//     the dot product are reduced once, then the rows are written.
//   * export_count_kernel / export_points_kernel : generated inverse depth -> one KITTI record (x, y, z, 0) in metres per
//     VALID pixel, packed in row-major pixel order per scan: an ordered stream compaction fused behind the pixel body of
//     inv_to_xyz (inv_point.h).  Two launches and no waiting between workgroups (the compaction itself: compact.h): the
//     first counts the valid pixels of every chunk of DG_EXPORT_CHUNK consecutive pixels; the second recomputes validity,
//     sums the counts of the chunks before its own, ranks its pixels with a wave ballot and a scan of the wave totals in
//     LDS, and stores each record with one 16-byte store at its final place.  No atomics: the bytes do not depend on the
//     order workgroups run in.
//     HBM traffic: 4 B of depth per pixel in each launch (the second read is L2-warm at the sizes of a batch), 8 B of
//     angles per VALID pixel (at most per pixel), 16 B written per kept point.
#include "common.h"
#include "compact.h"
#include "inv_point.h"

namespace {

// the sum of v over the workgroup's 256 threads, in a fixed order (every thread gets it)
__device__ __forceinline__ double block_sum256(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();  // the previous call's readers are done with `red`
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// torch.linspace(0, 1, n)[i] in float32 (RangeFactories: step = 1 / (n - 1) in float32; the first half counts up from 0,
// the second down from 1 with ONE rounding, 1 - step k as a fused multiply-add); n = 1 gives 0
__device__ __forceinline__ float linspace01(int i, int n) {
  if (n == 1) return 0.f;
  const float step = 1.f / (float)(n - 1);
  return i < n / 2 ? step * (float)i : __fmaf_rn(-step, (float)(n - 1 - i), 1.f);
}

// Arithmetic in float64 on the float32 inputs and weights, rounded once per output: lerp's end rows are then z0 and z1
// exactly.  slerp's cosine is rounded to float32 before acos, as the reference holds it: endpoints on one line give
// |cos| = 1 exactly, where sin(omega) is taken as 0 and every row comes out non-finite (the reference's 0 / 0).
__global__ __launch_bounds__(256) void latent_walk_kernel(const float* __restrict__ z0, const float* __restrict__ z1, int n,
                                                          int nz, int mode, float* __restrict__ out) {
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double omega = 0.0, so = 1.0;
  if (mode == 1) {
    double s0 = 0.0, s1 = 0.0;
    for (int j = tid; j < nz; j += 256) {
      const double a = z0[j], b = z1[j];
      s0 += a * a;
      s1 += b * b;
    }
    const double n0 = sqrt(block_sum256(s0, red)), n1 = sqrt(block_sum256(s1, red));
    double d = 0.0;
    for (int j = tid; j < nz; j += 256) d += ((double)z0[j] / n0) * ((double)z1[j] / n1);   // the NORMALISED endpoints
    const float c = (float)block_sum256(d, red);
    omega = acos((double)c);
    so = fabsf(c) < 1.f ? sin(omega) : 0.0;   // (NaN compares false: 0 as well)
  }
  for (int i = wave; i < n; i += 4) {
    const double w = (double)linspace01(i, n);
    double ca = 0.0, cb = 0.0;
    if (mode == 1) {
      ca = sin((1.0 - w) * omega) / so;
      cb = sin(w * omega) / so;
    }
    float* row = out + (long)i * nz;
    for (int j = lane; j < nz; j += 64) {
      const double a = z0[j], b = z1[j];   // the UN-normalised endpoints are the ones blended
      row[j] = (float)(mode == 1 ? ca * a + cb * b : a + (b - a) * w);
    }
  }
}

// launch 1: chunk_counts[b][c] = the valid pixels among pixels [c CHUNK, min((c + 1) CHUNK, hw)) of scan b
__global__ __launch_bounds__(CP_THREADS) void export_count_kernel(const float* __restrict__ in, long hw, long nchunk,
                                                                  int from_tanh, float drop_const, float tol,
                                                                  int* __restrict__ chunk_counts) {
  const long b = (long)blockIdx.x / nchunk, c = (long)blockIdx.x % nchunk;
  const float* src = in + b * hw;
  cp_count_chunk(c, [&](int, long px) { return px < hw && dg_inv_valid(dg_inv01(src[px < hw ? px : 0], from_tanh), drop_const, tol); },
                 chunk_counts + blockIdx.x);
}

// launch 2: the records of chunk c of scan b, placed behind those of the chunks before it
__global__ __launch_bounds__(CP_THREADS) void export_points_kernel(const float* __restrict__ in,
                                                                   const float* __restrict__ angle, long hw, long nchunk,
                                                                   int from_tanh, float min_d, float max_d, float drop_const,
                                                                   float tol, const int* __restrict__ chunk_counts,
                                                                   float4* __restrict__ out, int* __restrict__ counts) {
  const long b = (long)blockIdx.x / nchunk, c = (long)blockIdx.x % nchunk;
  const float* src = in + b * hw;
  float4* dst = out + b * hw;
  float4 rec[CP_ITERS];
  cp_place_chunk(
      chunk_counts + b * nchunk, c,
      [&](int k, long px) {
        float inv = 0.f;
        bool valid = false;
        if (px < hw) {
          inv = dg_inv01(src[px], from_tanh);
          valid = dg_inv_valid(inv, drop_const, tol);
        }
        rec[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (valid) {
          float x, y, z;
          dg_inv_point(inv, true, min_d, max_d, angle[px], angle[hw + px], x, y, z);
          rec[k] = make_float4(x * max_d, y * max_d, z * max_d, 0.f);   // metres; reflectance 0
        }
        return valid;
      },
      [&](int k, int pos) { dst[pos] = rec[k]; },   // pos < the scan's count <= hw
      c == nchunk - 1 ? counts + b : nullptr);
}

}  // namespace

extern "C" {

int dg_latent_walk(const float* z0, const float* z1, int n, int nz, int mode, float* out, void* s_) {
  if (!z0 || !z1 || !out || n < 1 || nz < 1 || mode < 0 || mode > 1) return DG_EINVAL;
  latent_walk_kernel<<<1, 256, 0, (hipStream_t)s_>>>(z0, z1, n, nz, mode, out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_export_points(const float* inv, const float* angle, int B, int H, int W, int from_tanh, float min_depth,
                     float max_depth, float drop_const, float tol, int* chunk_counts, float* out, int* counts, void* s_) {
  if (!inv || !angle || !chunk_counts || !out || !counts || B <= 0 || H <= 0 || W <= 0) return DG_EINVAL;
  if (((uintptr_t)out & 15) != 0) return DG_EINVAL;   // one 16-byte store per record
  const long hw = (long)H * W, nchunk = (hw + DG_EXPORT_CHUNK - 1) / DG_EXPORT_CHUNK;
  if (hw > 0x7fffffffL || (long)B * nchunk > 0x7fffffffL) return DG_EINVAL;   // int32 counts; one workgroup per chunk
  const int grid = (int)((long)B * nchunk);
  export_count_kernel<<<grid, CP_THREADS, 0, (hipStream_t)s_>>>(inv, hw, nchunk, from_tanh, drop_const, tol, chunk_counts);
  HIP_CHECK_RET(hipGetLastError());
  export_points_kernel<<<grid, CP_THREADS, 0, (hipStream_t)s_>>>(inv, angle, hw, nchunk, from_tanh, min_depth, max_depth,
                                                                 drop_const, tol, chunk_counts,
                                                                 reinterpret_cast<float4*>(out), counts);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

}  // extern "C"
