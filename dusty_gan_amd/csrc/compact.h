// Ordered stream compaction over the pixels of a row (a scan, or one realisation of one), written once: the flagged pixels'
// items packed in row-major pixel order, in two launches and without atomics or waiting between workgroups, so that the bytes
// do not depend on the order workgroups run in.  A workgroup of CP_THREADS threads owns one chunk of DG_EXPORT_CHUNK consecutive
// pixels; launch 1 counts the flagged pixels of every chunk, launch 2 flags again, sums the counts of the chunks before its
// own, ranks its pixels with a wave ballot and a scan of the wave totals in LDS, and puts each item at its final place.
// Used by dg_export_points (synthesis.hip) and dg_raydrop_gather (raydrop.hip).
#pragma once
#include "common.h"

constexpr int CP_THREADS = 256;
constexpr int CP_ITERS = DG_EXPORT_CHUNK / CP_THREADS;   // a thread's pixels of a chunk, CP_THREADS apart
constexpr int CP_SEGS = DG_EXPORT_CHUNK / 64;            // the chunk's runs of 64 consecutive pixels (one wave ballot each)
static_assert(DG_EXPORT_CHUNK % CP_THREADS == 0 && CP_THREADS % 64 == 0, "a chunk is whole waves of consecutive pixels");

// the thread's k-th pixel of chunk c (may lie beyond the row's end: the caller's flag is false there)
__device__ __forceinline__ long cp_pixel(long c, int k) { return c * DG_EXPORT_CHUNK + k * CP_THREADS + threadIdx.x; }

// launch 1 (every thread of the workgroup calls it): *count = the pixels of chunk c with flag(k, pixel)
template <class Flag>
__device__ __forceinline__ void cp_count_chunk(long c, Flag flag, int* __restrict__ count) {
  __shared__ int wsum[CP_THREADS / 64];
  const int tid = threadIdx.x;
  int cnt = 0;   // wave-uniform
#pragma unroll
  for (int k = 0; k < CP_ITERS; ++k) cnt += __popcll(__ballot(flag(k, cp_pixel(c, k))));
  if ((tid & 63) == 0) wsum[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < CP_THREADS / 64; ++w) s += wsum[w];
    *count = s;
  }
}

// launch 2 (every thread calls it): row_counts[0..c) = launch 1's counts of the row's earlier chunks (read-only data of the
// finished first launch: nothing to wait for).  flag(k, pixel) as in launch 1 - it may keep what it computed for put -;
// put(k, pos) stores the thread's k-th item at place pos of the row (pos < the row's count).  total != nullptr (the row's last
// chunk): *total = the row's count.
template <class Flag, class Put>
__device__ __forceinline__ void cp_place_chunk(const int* __restrict__ row_counts, long c, Flag flag, Put put,
                                               int* __restrict__ total) {
  __shared__ int wpre[CP_THREADS / 64];
  __shared__ int seg[CP_SEGS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int before = 0;
  for (long c2 = tid; c2 < c; c2 += CP_THREADS) before += row_counts[c2];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o);
  if (lane == 0) wpre[wave] = before;
  bool on[CP_ITERS];
  int rank[CP_ITERS];   // the flagged pixels before this one in its run of 64
#pragma unroll
  for (int k = 0; k < CP_ITERS; ++k) {
    on[k] = flag(k, cp_pixel(c, k));
    const unsigned long long m = __ballot(on[k]);
    rank[k] = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) seg[k * (CP_THREADS / 64) + wave] = __popcll(m);   // run k * 4 + wave starts at pixel k * 256 + wave * 64
  }
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int w = 0; w < CP_THREADS / 64; ++w) base += wpre[w];
#pragma unroll
  for (int k = 0; k < CP_ITERS; ++k) {
    const int s = k * (CP_THREADS / 64) + wave;
    int pre = base;
    for (int t = 0; t < s; ++t) pre += seg[t];
    if (on[k]) put(k, pre + rank[k]);
  }
  if (total && tid == 0) {
    int sum = base;
#pragma unroll
    for (int t = 0; t < CP_SEGS; ++t) sum += seg[t];
    *total = sum;
  }
}
