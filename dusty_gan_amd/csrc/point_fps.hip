// Furthest point sampling (the reference's native CUDA extension), gfx950:
//   * fps_kernel     : iterative furthest point sampling, one workgroup per cloud, the running minima in global memory.
//                      Reference: utils/sampling/fps/furthest_point_sampling.cu:97-207 (+ gather :38-60).
//   * fps_map_kernel : the same selection on a planar point map [B,3,HW] with the running minima in registers and LDS
//                      (dg_fps_map).
// Both share the visit (fps_visit) and the workgroup's pick (fps_pick), so they select the same samples.
#include "common.h"

namespace {

// FPS.  Selection rule of the reference, including its tie-breaking: every thread t scans k = t, t + T, ... keeping the
// FIRST strictly-greater candidate (T = opt_n_threads(n), a power of two <= 512); the tree reduction then folds slot
// t + w into slot t for w = T/2 .. 1 keeping the lower SLOT on ties, so two threads meet at the lowest bit in which
// their ids differ and the one with that bit clear wins.  Among equal maxima the winner therefore minimises
// (bit-reversed (k mod T), k); `tie_mod` carries T.
// Points with |p|^2 <= 1e-3 (dropped returns at the origin) never become candidates (:132-134).  The reference compares
// the float `mag` with the DOUBLE literal 1e-3; float(1e-3) = 0.0010000000475 lies above it and its lower neighbour
// below, so in float terms the skip is `mag < 1e-3f`: a point of squared norm exactly 1e-3f IS a candidate
// (tests/golden/fps_emd.npz thresh_*, recorded from the reference's kernel).
struct Cand {
  float v;
  int k;
};
__device__ __forceinline__ bool cand_better(const Cand& a, const Cand& b, int tie_mod) {
  if (a.v != b.v) return a.v > b.v;
  const unsigned ra = __brev((unsigned)(a.k & (tie_mod - 1))), rb = __brev((unsigned)(b.k & (tie_mod - 1)));
  return ra != rb ? ra < rb : a.k < b.k;
}

// One point's visit, shared by both kernels: fold the distance to the last sample into the point's running minimum `t`
// and offer the result to the thread's best.  Returns the new minimum.
__device__ __forceinline__ float fps_visit(float x2, float y2, float z2, float x1, float y1, float z1, float t, int k,
                                           int tie_mod, Cand& best) {
#pragma clang fp contract(off)
  const float d = (x2 - x1) * (x2 - x1) + (y2 - y1) * (y2 - y1) + (z2 - z1) * (z2 - z1);
  const float d2 = fminf(d, t);
  const Cand c = {d2, k};
  if (cand_better(c, best, tie_mod)) best = c;
  return d2;
}
__device__ __forceinline__ bool fps_skipped(float x, float y, float z) {
#pragma clang fp contract(off)
  const float mag = (x * x) + (y * y) + (z * z);
  return mag < 1e-3f;  // == the reference's `mag <= 1e-3` (double literal): see above
}
// The workgroup's pick from its threads' bests: wave reduction, then across waves; two barriers.  Returns the index
// every thread continues from (all-skipped: the reference's besti stays 0) and records it as sample j.
__device__ __forceinline__ int fps_pick(Cand best, int tie_mod, Cand* red, int* s_old, int* idx, int j) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  for (int o = 32; o > 0; o >>= 1) {
    Cand other = {__shfl_xor(best.v, o, 64), __shfl_xor(best.k, o, 64)};
    if (cand_better(other, best, tie_mod)) best = other;
  }
  if (lane == 0) red[wave] = best;
  __syncthreads();
  if (tid == 0) {
    Cand b = red[0];
    for (int w = 1; w < nw; ++w)
      if (cand_better(red[w], b, tie_mod)) b = red[w];
    *s_old = b.v < 0.f ? 0 : b.k;
    idx[j] = *s_old;
  }
  __syncthreads();
  return *s_old;
}

// Minima in global memory (`temp`).  PACKED: [B,n,3] clouds, strides known at compile time (dg_fps); otherwise coordinate
// c of point p is at p * sp + c * sc (dg_fps_map's general path).
template <bool PACKED>
__global__ __launch_bounds__(1024) void fps_kernel(const float* __restrict__ xyz, long sb, long sp_, long sc_, int n, int m,
                                                   int tie_mod, float* __restrict__ temp, int* __restrict__ idx,
                                                   float* __restrict__ out) {
  __shared__ Cand red[16];
  __shared__ int s_old;
  const int tid = threadIdx.x;
  const long sp = PACKED ? 3 : sp_, sc = PACKED ? 1 : sc_;
  xyz += (long)blockIdx.x * (PACKED ? (long)n * 3 : sb);
  temp += (long)blockIdx.x * n;
  idx += (long)blockIdx.x * m;
  if (out) out += (long)blockIdx.x * m * 3;
  for (int k = tid; k < n; k += blockDim.x) temp[k] = 1e10f;  // furthest_point_sampling.cpp: torch::full(1e10)
  int old = 0;
  if (tid == 0) idx[0] = 0;
  if (out && tid < 3) out[tid] = xyz[tid * sc];
  __syncthreads();
  for (int j = 1; j < m; ++j) {
    const float x1 = xyz[old * sp], y1 = xyz[old * sp + sc], z1 = xyz[old * sp + 2 * sc];
    Cand best = {-1.f, 0};
    for (int k = tid; k < n; k += blockDim.x) {
      const float x2 = xyz[k * sp], y2 = xyz[k * sp + sc], z2 = xyz[k * sp + 2 * sc];
      if (fps_skipped(x2, y2, z2)) continue;
      temp[k] = fps_visit(x2, y2, z2, x1, y1, z1, temp[k], k, tie_mod, best);
    }
    old = fps_pick(best, tie_mod, red, &s_old, idx, j);
    if (out && tid < 3) out[j * 3 + tid] = xyz[old * sp + tid * sc];
  }
}

// Minima on chip, for planar point maps (point stride 1) of n <= (RS + LS) * 1024 points: thread t owns the points
// k = t + i * 1024 and keeps the minima of its first RS slots in registers (t[] is indexed statically: the slot loop is
// fully unrolled) and of the next LS slots in LDS (t_lds[i][tid]: conflict-free, never shared between threads).
// A point the reference skips, and a slot past n, holds the minimum -1: fps_visit then offers {-1, k}, which loses to
// every real candidate (d >= 0) and which fps_pick maps to index 0 - exactly what `continue` gives in fps_kernel.  So no
// per-slot mask lives across the sample loop: reads are clamped to n - 1 and whole groups of slots past n are stepped
// over on a scalar test.
// `p`, `t0` and `nn` pass through an empty asm once per sample so that neither the loop-invariant point loads nor the
// per-slot offsets and end-of-walk tests are hoisted out of the sample loop (hoisted, they spill).
constexpr int FM_T = 1024;
constexpr int FM_G = 8;       // slots whose 3 * FM_G loads are in flight together; the walk ends at a group boundary
constexpr int FM_RS64 = 48;   // register slots of the 64-slot instantiation; the other 16 are 64 KB of LDS
template <int RS, int LS>
__global__ __launch_bounds__(FM_T) void fps_map_kernel(const float* __restrict__ X, long sb, long sc, int n, int m,
                                                       int tie_mod, int* __restrict__ idx, float* __restrict__ out) {
  __shared__ float t_lds[LS > 0 ? LS * FM_T : 1];
  __shared__ Cand red[16];
  __shared__ int s_old;
  const int tid = threadIdx.x;
  X += (long)blockIdx.x * sb;
  idx += (long)blockIdx.x * m;
  if (out) out += (long)blockIdx.x * m * 3;
  float t[RS];
#pragma unroll
  for (int i = 0; i < RS + LS; ++i) {
    const int k = tid + i * FM_T, kk = min(k, n - 1);
    const float v = (k < n && !fps_skipped(X[kk], X[kk + sc], X[kk + 2 * sc])) ? 1e10f : -1.f;
    if (i < RS) t[i] = v;
    else t_lds[(i - RS) * FM_T + tid] = v;
    __builtin_amdgcn_sched_barrier(0);  // one slot at a time: 64 slots' loads and masks in flight at once spill SGPRs
  }
  int old = 0;
  if (tid == 0) idx[0] = 0;
  if (out && tid < 3) out[tid] = X[tid * sc];
  __syncthreads();
  for (int j = 1; j < m; ++j) {
    const float* p = X;
    int t0 = tid, nn = n;
    asm volatile("" : "+s"(p), "+v"(t0), "+s"(nn));
    const float x1 = p[old], y1 = p[old + sc], z1 = p[old + 2 * sc];
    const int ns = __builtin_amdgcn_readfirstlane((nn + FM_T - 1) / FM_T);  // slots that hold a point: a scalar
    Cand best = {-1.f, 0};
#pragma unroll
    for (int g = 0; g < RS + LS; g += FM_G) {
      if (g >= ns) continue;
      float x2[FM_G], y2[FM_G], z2[FM_G];
#pragma unroll
      for (int e = 0; e < FM_G; ++e) {
        const int kk = min(t0 + (g + e) * FM_T, nn - 1);
        x2[e] = p[kk], y2[e] = p[kk + sc], z2[e] = p[kk + 2 * sc];
      }
#pragma unroll
      for (int e = 0; e < FM_G; ++e) {
        const int i = g + e, k = t0 + i * FM_T;
        if (i < RS) t[i] = fps_visit(x2[e], y2[e], z2[e], x1, y1, z1, t[i], k, tie_mod, best);
        else {
          float* q = &t_lds[(i - RS) * FM_T + t0];
          *q = fps_visit(x2[e], y2[e], z2[e], x1, y1, z1, *q, k, tie_mod, best);
        }
      }
    }
    old = fps_pick(best, tie_mod, red, &s_old, idx, j);
    if (out && tid < 3) out[j * 3 + tid] = X[old + tid * sc];
  }
}

}  // namespace

extern "C" {

// opt_n_threads(n) of the reference launcher: the largest power of two <= min(n, 512) -- only its tie rule is kept
static int fps_tie_mod(int n) {
  int tie = 1;
  while (tie * 2 <= n && tie * 2 <= 512) tie *= 2;
  return tie;
}
static int fps_threads(int n) { return n >= 1024 ? 1024 : (n >= 256 ? 256 : 64); }

int dg_fps(const float* xyz, int B, int n, int m, float* temp, int* idx, float* out, void* s_) {
  if (!xyz || !temp || !idx || B <= 0 || n <= 0 || m <= 0 || m > n) return DG_EINVAL;
  fps_kernel<true><<<B, fps_threads(n), 0, (hipStream_t)s_>>>(xyz, 0, 3, 1, n, m, fps_tie_mod(n), temp, idx, out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_fps_map(const float* X, long x_sb, long x_sp, long x_sc, int B, int n, int m, float* temp, int* idx, float* out,
               void* s_) {
  if (!X || !idx || B <= 0 || n <= 0 || m <= 0 || m > n) return DG_EINVAL;
  if (x_sp <= 0 || x_sc <= 0 || x_sb < 0) return DG_EINVAL;
  // point offsets are formed in 64 bits; the bound keeps p * x_sp + 2 * x_sc inside them for every n
  if (x_sp > 0x7fffffffL || x_sc > 0x3fffffffL) return DG_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)s_;
  const int tie = fps_tie_mod(n);
  if (x_sp == 1 && n <= 16 * FM_T)
    fps_map_kernel<16, 0><<<B, FM_T, 0, s>>>(X, x_sb, x_sc, n, m, tie, idx, out);
  else if (x_sp == 1 && n <= 64 * FM_T)
    fps_map_kernel<FM_RS64, 64 - FM_RS64><<<B, FM_T, 0, s>>>(X, x_sb, x_sc, n, m, tie, idx, out);
  else {
    if (!temp) return DG_EINVAL;
    fps_kernel<false><<<B, fps_threads(n), 0, s>>>(X, x_sb, x_sp, x_sc, n, m, tie, temp, idx, out);
  }
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

}  // extern "C"
