// What the pointwise translation units (pointwise.hip, head_post.hip, blur_aug.hip, step_inputs.hip) share: 16-byte accesses of feature-map
// elements and the launchers' block arithmetic.
#pragma once
#include "common.h"

// 16-byte loads / stores of feature-map elements as floats: V = 8 bf16 or 4 fp32 per access
template <typename T> struct Vec16;
template <> struct Vec16<bf16> {
  static constexpr int V = 8;
  static __device__ __forceinline__ void load(const bf16* p, float (&v)[8]) {
    const uint4 r = *(const uint4*)p;
    const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[2 * k] = __builtin_bit_cast(float, w[k] << 16);
      v[2 * k + 1] = __builtin_bit_cast(float, w[k] & 0xffff0000u);
    }
  }
  static __device__ __forceinline__ void store(bf16* p, const float (&v)[8]) {
    unsigned w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      w[k] = (unsigned)__builtin_bit_cast(unsigned short, (bf16)v[2 * k]) |
             ((unsigned)__builtin_bit_cast(unsigned short, (bf16)v[2 * k + 1]) << 16);
    *(uint4*)p = make_uint4(w[0], w[1], w[2], w[3]);
  }
};
template <> struct Vec16<float> {
  static constexpr int V = 4;
  static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
    const float4 r = *(const float4*)p;
    v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
  }
  static __device__ __forceinline__ void store(float* p, const float (&v)[4]) { *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); }
};

static inline unsigned nblk(long n, int bs = 256) { return (unsigned)((n + bs - 1) / bs); }
// pixels per block of the kernels that also sum their output per sample: the largest power-of-two multiple of 256 that
// divides HW, at most 4096 (one atomic per block: 16 per 64x1024 sample)
static int sum_chunk(long HW) {
  int c = 256;
  while (c < 4096 && HW % (2 * c) == 0) c *= 2;
  return c;
}

// 16-byte accesses of n elements of `dtype` at p
static inline bool vec_ok(const void* p, long n, int dtype) {
  const int V = dtype == DG_BF16 ? 8 : 4;
  return n % V == 0 && ((size_t)p & 15) == 0;
}
