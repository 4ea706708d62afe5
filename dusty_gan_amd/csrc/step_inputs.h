// What the kernels that feed a training step share ACROSS translation units (the library is built without relocatable device
// code, so a body two files run lives in a header):
//   * the counter adds: step_inputs.hip's dg_counter_add* launches and the tail block of optim.hip's shadow refresh;
//   * fetch_reals' pixel, source addressing and validation: step_inputs.hip's stand-alone kernel and the fetch blocks of its
//     step prologue.
#pragma once
#include "common.h"

// ---- k <= 8 DISTINCT device-resident counters advanced by one block (a step's Philox offsets and Adam step counts, queued by
//      the caller behind their consumers); optionally src[0..snap_n) filed in slot (OLD value of c[snap_idx]) % snap_ring
struct CounterAdds {
  unsigned long long* c[8]; unsigned long long d[8]; int k;
  int snap_idx, snap_n, snap_ring; const float* snap_src; float* snap_dst;   // snap_idx < 0: no snapshot
};
__device__ __forceinline__ void counter_adds_body(const CounterAdds& a) {   // (one block's threads 0 .. k-1)
  if ((int)threadIdx.x >= a.k) return;
  const unsigned long long v = *a.c[threadIdx.x];
  *a.c[threadIdx.x] = v + a.d[threadIdx.x];
  if ((int)threadIdx.x == a.snap_idx) {          // the thread that advances the counter also files the snapshot under its old value
    float* dst = a.snap_dst + (long)(v % (unsigned long long)a.snap_ring) * a.snap_n;
    for (int i = 0; i < a.snap_n; ++i) dst[i] = a.snap_src[i];
    __threadfence_system();                      // (dst may be mapped host memory)
  }
}
static int fill_counter_adds(CounterAdds& a, unsigned long long* const* counters, const unsigned long long* deltas, int k,
                             int snap_idx, const float* src, int n, float* dst_ring, int ring) {
  if (k < 1 || k > 8 || !counters || !deltas) return DG_EINVAL;
  if (snap_idx >= 0 && (snap_idx >= k || !src || !dst_ring || n < 1 || n > 64 || ring < 1)) return DG_EINVAL;
  a = CounterAdds{};
  a.snap_idx = snap_idx; a.snap_n = n; a.snap_ring = ring; a.snap_src = src; a.snap_dst = dst_ring;
  for (int i = 0; i < k; ++i) {
    if (!counters[i]) return DG_EINVAL;
    for (int j = 0; j < i; ++j)
      if (counters[j] == counters[i]) return DG_EINVAL;
    a.c[i] = counters[i]; a.d[i] = deltas[i];
  }
  a.k = k;
  return DG_OK;
}

// ---- GumbelSigmoid.logistic_noise (models/dusty.py:30-36) straight from the generator: element o of U1 is word o & 3 of Philox
//      counter offset + o / 4, U2 the same (n + 3) / 4 counters further - exactly what two uniform fills of n elements followed
//      by dg_logistic_noise produce, in one launch and without the two 4 n-byte round trips.  philox_logistic4: the four
//      elements of group i in registers (step_inputs.hip's draws store them; raydrop.hip's keep kernel consumes them in place).
__device__ __forceinline__ void philox_logistic4(uint64_t seed, uint64_t stream, uint64_t offset, float eps, long n, long i,
                                                 float (&v)[4]) {
  const uint64_t n4 = (uint64_t)((n + 3) / 4);
  uint32_t r1[4], r2[4];
  philox4x32_10(seed, offset + (uint64_t)i, stream, r1);
  philox4x32_10(seed, offset + n4 + (uint64_t)i, stream, r2);
  const float s24 = 1.f / 16777216.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float u1 = (float)(r1[j] >> 8) * s24, u2 = (float)(r2[j] >> 8) * s24;
    v[j] = -logf(logf(u1 + eps) / logf(u2 + eps) + eps);
  }
}
__device__ __forceinline__ void philox_logistic_body(uint64_t seed, uint64_t stream, uint64_t offset, float eps, long n,
                                                     float* __restrict__ out, long i) {
  if (4 * i >= n) return;
  float v[4];
  philox_logistic4(seed, stream, offset, eps, n, i, v);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long o = 4 * i + j;
    if (o >= n) break;
    out[o] = v[j];
  }
}

// ---- fetch_reals (trainers/dcgan_amp.py:154-160; utils/lidar.py:31-36; utils/__init__.py:70-73)
__device__ __forceinline__ float fetch_real_px(float pol, float m, float min_d, float max_d, float drop_const) {
  const float depth = pol * (max_d - min_d) + min_d;
  const float disp = 1.f / depth;
  float inv = (disp - 1.f / max_d) / (1.f / min_d - 1.f / max_d);
  inv = inv * 2.f - 1.f;
  return m * inv + (1.f - m) * drop_const;
}
// Where pixel px of sample b of the batch a DgFetch names lies (include/dusty_gan_hip.h states the three forms):
//   plain     pol / mask ARE the batch;
//   pool      pool_ctr != nullptr: batch *pool_ctr % npool of `npool` batches (a device-resident loader position: a captured
//             training step replays on the next pooled batch without a copy);
//   resident  kResident (the caller's choice where nslab > 0): slab *pool_ctr % nslab of a scan store, the sample's variant
//             from the flip table of the epoch's parity; mask == nullptr - the validity is pol > 0 (a resident store keeps
//             no mask: datasets/resident.py states why that is the stored mask bit for bit).
struct FetchSrc { const float* pol; const float* mask; };
template <bool kResident>
__device__ __forceinline__ FetchSrc fetch_src(const DgFetch& f, long b, long px) {
  if constexpr (kResident) {
    const unsigned long long ctr = *f.pool_ctr, ns = (unsigned long long)f.nslab;
    const long row = (long)(ctr % ns) * f.B + b;
    const long var = f.flip_tab ? (long)f.flip_tab[(long)((ctr / ns) & 1ull) * f.nslab * f.B + row] : 0;
    return {f.pol + (var * f.nslab * f.B + row) * f.HW + px, nullptr};
  }
  long off = b * f.HW + px;
  if (f.pool_ctr) off += (long)(*f.pool_ctr % (unsigned long long)f.npool) * ((long)f.B * f.HW);
  return {f.pol + off, f.mask + off};
}
// (the destination of the sums - DgFetch.parts or an accumulator - is the caller's to check)
static int fetch_check(const DgFetch& f) {
  if (!f.pol || !f.out || f.B <= 0 || f.HW <= 0 || f.nslab < 0) return DG_EINVAL;
  if (f.nslab > 0 ? !f.pool_ctr : (!f.mask || (f.pool_ctr && f.npool <= 0))) return DG_EINVAL;
  return DG_OK;
}
