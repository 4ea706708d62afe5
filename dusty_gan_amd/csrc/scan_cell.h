// The cell side of the two cloud projections, written once: scan_project.hip (rows from KITTI's file order) and
// beam_project.hip (rows from a beam table) must agree on a point's column, on the z-buffer key and on what an empty cell
// holds, bit for bit.  Reference: process_point_clouds, process_kitti.py:60-73, :85-86, :109-111.
#pragma once

#define KEY_EMPTY 0xFFFFFFFFFFFFFFFFull

static inline int sc_nblk(long n) { return (int)((n + 255) / 256); }

// column coordinate floor(((-atan2(y, x) / pi + 1) / 2 mod 1) * W), every step in float32 (:109-111).  The caller keeps the
// point only for 0 <= result < W: a non-finite coordinate has no column
__device__ __forceinline__ float sc_column(float x, float y, int W) {
#pragma clang fp contract(off)  // plain IEEE operators (as scan_to_polar_kernel): numpy's float32 arithmetic, step for step
  const float yaw = -atan2f(y, x);
  float g = (yaw / 3.14159274101257324f + 1.f) / 2.f;   // np.pi as float32
  g = fmodf(g, 1.f);                                    // np.remainder(g, 1): g >= 0, so the C remainder is numpy's
  if (g < 0.f) g += 1.f;
  return floorf(g * (float)W);
}

// the z-buffer word: non-negative floats order like their bits, so a 64-bit atomicMin keeps the NEAREST point and, of two
// points with the same float32 depth, the LOWER index
__device__ __forceinline__ unsigned long long sc_key(float depth, unsigned index) {
  return ((unsigned long long)__float_as_uint(depth) << 32) | index;
}

// status (nullable): S words cleared beside the keys
static __global__ __launch_bounds__(256) void key_fill_kernel(unsigned long long* __restrict__ keys, long n,
                                                              int* __restrict__ status, int S) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) keys[i] = KEY_EMPTY;
  if (status && i < S) status[i] = 0;
}

// every cell <- its winner's record, bit for bit; zeros for a cell without one (and, with status, for a refused scan)
static __global__ __launch_bounds__(256) void scan_gather_kernel(const float* __restrict__ points,
                                                                 const long* __restrict__ offsets,
                                                                 const unsigned long long* __restrict__ keys,
                                                                 const int* __restrict__ status, long cells_per_scan, long n,
                                                                 float* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = (int)(i / cells_per_scan);
  const unsigned long long k = keys[i];
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (k != KEY_EMPTY && (!status || status[s] == 0)) {
    const long o0 = offsets[s], idx = (long)(unsigned)(k & 0xFFFFFFFFull);
    if (idx < offsets[s + 1] - o0) v = reinterpret_cast<const float4*>(points)[o0 + idx];
  }
  reinterpret_cast<float4*>(out)[i] = v;
}
