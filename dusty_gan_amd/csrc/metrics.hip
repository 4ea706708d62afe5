// Point-cloud kernels of the validation metrics (the reference's native CUDA extensions), gfx950:
//   * fps_kernel            : iterative furthest point sampling, one workgroup per cloud.
//                             Reference: utils/sampling/fps/furthest_point_sampling.cu:97-207 (+ gather :38-60).
//   * fps_map_kernel        : the same selection on a planar point map [B,3,HW] with the running minima in registers
//                             and LDS instead of global memory (dg_fps_map).
//   * chamfer_dir_kernel    : ALL-PAIRS directed Chamfer means  L[i][j] = mean_{p in A_i} min_{q in B_j} |p - q|^2.
//                             Reference: utils/metrics/distance/cd/chamfer_distance.{cu,cpp} (nnsearch :41-66) as driven by
//                             utils/metrics/cov_mmd_1nna.py:20-52, which loops i in Python and calls the extension on
//                             (cloud i expanded) x (512 clouds) -- N^2 / 512 launches.  Here one launch fills a whole
//                             [Na,Nb] matrix; CD(i,j) = L_AB[i][j] + L_BA[j][i].
// Both are VALU-bound fp32 work (K = 3: no matrix-core shape): the Chamfer kernel keeps PT points of cloud A per lane in
// registers, streams cloud B through LDS with broadcast 16-byte reads and evaluates two points per packed instruction.
#include "common.h"

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

// --------------------------------------------------------------------------------------------------------------
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

// --------------------------------------------------------------------------------------------------------------
// Directed Chamfer means, all pairs.
// Work split: a WAVE owns 512 consecutive points of one cloud A_i (8 per lane, as 4 packed pairs, in registers for the
// whole kernel) and their running minima; a workgroup is 4 waves = 4 clouds (n <= 512), 2 clouds (n <= 1024) or a
// 2048-point slice of one cloud (larger n: blockIdx.z walks the slices and the partial means are added atomically).
// The workgroup streams TB clouds B_j through LDS in chunks of MC points (x, y, z as 16 bytes, double-buffered; the
// next chunk's global loads are issued before the math and stored to LDS after it); every lane reads the SAME LDS
// address (broadcast).  Per point pair: 6 packed fp32 instructions per two pairs + one v_min each = 4 lane-ops.
constexpr int CH_THREADS = 256;
constexpr int CH_PT = 8;                 // points of A per lane
constexpr int CH_WPTS = 64 * CH_PT;      // points of A per wave
constexpr int CH_MC = 512;               // points of B per LDS chunk (8 KB), two buffers
constexpr int CH_LD = CH_MC / CH_THREADS;  // chunk points loaded per thread

// PAIRED: cloud A_i against B_i only (L[i]); the workgroup then owns one cloud (wpc >= 4) and streams just B_i - the same
// per-wave arithmetic and sums as the diagonal of the all-pairs launch.
template <bool PAIRED>
__global__ __launch_bounds__(CH_THREADS) void chamfer_dir_kernel(const float* __restrict__ A, int Na, int n, int wpc,
                                                                 const float* __restrict__ Bc, int Nb, int m, int TB,
                                                                 float* __restrict__ L) {
  __shared__ float4 qbuf[2][CH_MC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // wpc = waves per cloud (1, 2 or a multiple of 4).  Which cloud / slice does this wave own?
  int i, slice;
  if (wpc >= 4) { i = blockIdx.y; slice = blockIdx.z * 4 + wave; }
  else { i = blockIdx.y * (4 / wpc) + wave / wpc; slice = wave % wpc; }
  const bool live = i < Na;
  const int p0 = slice * CH_WPTS + lane * CH_PT;
  f2 px[CH_PT / 2], py[CH_PT / 2], pz[CH_PT / 2];
  const float* a = A + (long)(live ? i : 0) * n * 3;
#pragma unroll
  for (int h = 0; h < CH_PT / 2; ++h) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int p = p0 + 2 * h + e;
      const int pp = p < n ? p : 0;  // out-of-range slots replicate point 0; their minima are dropped from the sum
      px[h][e] = a[pp * 3 + 0];
      py[h][e] = a[pp * 3 + 1];
      pz[h][e] = a[pp * 3 + 2];
    }
  }
  const int j0 = PAIRED ? i : blockIdx.x * TB, j1 = PAIRED ? i + 1 : min(Nb, j0 + TB);
  const int nchunk = (m + CH_MC - 1) / CH_MC;
  const int total = (j1 - j0) * nchunk;  // (cloud, chunk) steps of this workgroup
  float r[CH_LD][3];
  auto fetch = [&](int step) {
    const int j = j0 + step / nchunk, c = step % nchunk;
    const float* q = Bc + (long)j * m * 3;
#pragma unroll
    for (int u = 0; u < CH_LD; ++u) {
      const int k = c * CH_MC + u * CH_THREADS + tid;
      const int kk = k < m ? k : 0;  // the tail of the last chunk repeats the cloud's first point: no effect on a minimum
      r[u][0] = q[kk * 3 + 0]; r[u][1] = q[kk * 3 + 1]; r[u][2] = q[kk * 3 + 2];
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int u = 0; u < CH_LD; ++u) qbuf[buf][u * CH_THREADS + tid] = make_float4(r[u][0], r[u][1], r[u][2], 0.f);
  };
  f2 rmin[CH_PT / 2];
  if (total > 0) { fetch(0); commit(0); }
  __syncthreads();
  for (int step = 0; step < total; ++step) {
    const int buf = step & 1, c = step % nchunk;
    if (c == 0) {
#pragma unroll
      for (int h = 0; h < CH_PT / 2; ++h) rmin[h] = (f2){3.0e38f, 3.0e38f};
    }
    if (step + 1 < total) fetch(step + 1);
#pragma unroll 2
    for (int t = 0; t < CH_MC; ++t) {
      const float4 q = qbuf[buf][t];
      const f2 qx = (f2){q.x, q.x}, qy = (f2){q.y, q.y}, qz = (f2){q.z, q.z};
#pragma unroll
      for (int h = 0; h < CH_PT / 2; ++h) {
        const f2 dx = qx - px[h], dy = qy - py[h], dz = qz - pz[h];
        f2 d = dx * dx;
        d = __builtin_elementwise_fma(dy, dy, d);
        d = __builtin_elementwise_fma(dz, dz, d);
        rmin[h][0] = __builtin_fminf(rmin[h][0], d[0]);
        rmin[h][1] = __builtin_fminf(rmin[h][1], d[1]);
      }
    }
    if (c == nchunk - 1) {  // cloud B_j finished: this wave's share of mean_p min_q
      float s = 0.f;
#pragma unroll
      for (int h = 0; h < CH_PT / 2; ++h) {
        if (p0 + 2 * h < n) s += rmin[h][0];
        if (p0 + 2 * h + 1 < n) s += rmin[h][1];
      }
      s = dg_wave_sum(s);
      if (lane == 0 && live && slice * CH_WPTS < n) {
        float* dst = PAIRED ? &L[i] : &L[(long)i * Nb + j0 + step / nchunk];
        if (wpc == 1) *dst = s / (float)n;
        else atomicAdd(dst, s / (float)n);
      }
    }
    if (step + 1 < total) commit(buf ^ 1);
    __syncthreads();
  }
}

// --------------------------------------------------------------------------------------------------------------
// Paired nearest-neighbour search WITH indices (chamfer_distance.cu:9-127 / nnsearch chamfer_distance.cpp:39-62):
// dist[i][p] = min_q |A_i[p] - B_i[q]|^2, idx[i][p] = the LOWEST q attaining it.  The work split and the inner loop are
// chamfer_dir_kernel<true>'s (a wave owns 512 points of A in registers, B_i streamed through the double-buffered LDS chunks,
// the same three packed operations per distance: a distance here is the one dg_chamfer_paired sums, bit for bit).  The loop
// tracks the minimum only; per point and chunk ONE strict compare notes the chunk in which the running minimum last fell,
// i.e. the first chunk that attains the final minimum.  After the stream every lane rescans the winning chunk of each of its
// points (from global memory: the chunks differ lane to lane) for the first minimum, strict `<` - the reference's rule.
// Clouds come with a point stride and a channel stride (planar [B,3,HW] point maps and [B,n,3] clouds alike).  Every dist /
// idx element has one writer; no atomics.
__global__ __launch_bounds__(CH_THREADS) void chamfer_nn_kernel(const float* __restrict__ A, long a_sb, int a_sp, int a_sc,
                                                                int n, const float* __restrict__ Bc, long b_sb, int b_sp,
                                                                int b_sc, int m, float* __restrict__ dist,
                                                                int* __restrict__ idx) {
  __shared__ float4 qbuf[2][CH_MC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.y, slice = blockIdx.z * 4 + wave;
  const int p0 = slice * CH_WPTS + lane * CH_PT;
  f2 px[CH_PT / 2], py[CH_PT / 2], pz[CH_PT / 2];
  const float* a = A + (long)i * a_sb;
  const float* q = Bc + (long)i * b_sb;
#pragma unroll
  for (int h = 0; h < CH_PT / 2; ++h) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int p = p0 + 2 * h + e;
      const long pp = (long)(p < n ? p : 0) * a_sp;  // out-of-range slots replicate point 0 and store nothing
      px[h][e] = a[pp];
      py[h][e] = a[pp + a_sc];
      pz[h][e] = a[pp + 2l * a_sc];
    }
  }
  const int nchunk = (m + CH_MC - 1) / CH_MC;
  float r[CH_LD][3];
  auto fetch = [&](int c) {
#pragma unroll
    for (int u = 0; u < CH_LD; ++u) {
      const int k = c * CH_MC + u * CH_THREADS + tid;
      const long kk = (long)(k < m ? k : 0) * b_sp;  // the last chunk's tail repeats point 0: chunk 0 holds it first
      r[u][0] = q[kk]; r[u][1] = q[kk + b_sc]; r[u][2] = q[kk + 2l * b_sc];
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int u = 0; u < CH_LD; ++u) qbuf[buf][u * CH_THREADS + tid] = make_float4(r[u][0], r[u][1], r[u][2], 0.f);
  };
  f2 rmin[CH_PT / 2];
  int wch[CH_PT];
#pragma unroll
  for (int h = 0; h < CH_PT / 2; ++h) {
    rmin[h] = (f2){3.0e38f, 3.0e38f};
    wch[2 * h] = 0; wch[2 * h + 1] = 0;
  }
  fetch(0);
  commit(0);
  __syncthreads();
  for (int c = 0; c < nchunk; ++c) {
    const int buf = c & 1;
    if (c + 1 < nchunk) fetch(c + 1);
    f2 was[CH_PT / 2];
#pragma unroll
    for (int h = 0; h < CH_PT / 2; ++h) was[h] = rmin[h];
#pragma unroll 2
    for (int t = 0; t < CH_MC; ++t) {
      const float4 v = qbuf[buf][t];
      const f2 qx = (f2){v.x, v.x}, qy = (f2){v.y, v.y}, qz = (f2){v.z, v.z};
#pragma unroll
      for (int h = 0; h < CH_PT / 2; ++h) {
        const f2 dx = qx - px[h], dy = qy - py[h], dz = qz - pz[h];
        f2 d = dx * dx;
        d = __builtin_elementwise_fma(dy, dy, d);
        d = __builtin_elementwise_fma(dz, dz, d);
        rmin[h][0] = __builtin_fminf(rmin[h][0], d[0]);
        rmin[h][1] = __builtin_fminf(rmin[h][1], d[1]);
      }
    }
#pragma unroll
    for (int h = 0; h < CH_PT / 2; ++h) {
      if (rmin[h][0] < was[h][0]) wch[2 * h] = c;
      if (rmin[h][1] < was[h][1]) wch[2 * h + 1] = c;
    }
    if (c + 1 < nchunk) commit(buf ^ 1);
    __syncthreads();
  }
  // the first minimum inside the winning chunk; the distance stored is the streamed one
#pragma unroll
  for (int h = 0; h < CH_PT / 2; ++h) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int p = p0 + 2 * h + e;
      if (p >= n) continue;
      const int k0 = wch[2 * h + e] * CH_MC, k1 = min(m, k0 + CH_MC);
      const float x = px[h][e], y = py[h][e], z = pz[h][e];
      float best = 3.0e38f;
      int bi = k0;
      for (int k = k0; k < k1; ++k) {
        const long kk = (long)k * b_sp;
        const float dx = q[kk] - x, dy = q[kk + b_sc] - y, dz = q[kk + 2l * b_sc] - z;
        float d = dx * dx;
        d = __builtin_fmaf(dy, dy, d);
        d = __builtin_fmaf(dz, dz, d);
        if (d < best) { best = d; bi = k; }
      }
      dist[(long)i * n + p] = rmin[h][e];
      idx[(long)i * n + p] = bi;
    }
  }
}

// --------------------------------------------------------------------------------------------------------------
// JSD occupancy histogram (utils/metrics/jsd.py:24-79): every point votes for its nearest node of the in-sphere unit
// grid -- brute force like the reference (argmin over all nodes, first index on ties), nodes streamed through LDS.
constexpr int GV_CHUNK = 2048;

__global__ __launch_bounds__(256) void grid_vote_kernel(const float* __restrict__ pts, long P,
                                                        const float* __restrict__ grid, int Ng,
                                                        float* __restrict__ counters) {
#pragma clang fp contract(off)
  __shared__ float4 g[GV_CHUNK];
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool ok = p < P;
  const float x = ok ? pts[p * 3 + 0] : 0.f, y = ok ? pts[p * 3 + 1] : 0.f, z = ok ? pts[p * 3 + 2] : 0.f;
  float best = 3.0e38f;
  int bi = 0;
  for (int c0 = 0; c0 < Ng; c0 += GV_CHUNK) {
    const int cn = min(GV_CHUNK, Ng - c0);
    __syncthreads();
    for (int t = threadIdx.x; t < cn; t += blockDim.x)
      g[t] = make_float4(grid[(c0 + t) * 3 + 0], grid[(c0 + t) * 3 + 1], grid[(c0 + t) * 3 + 2], 0.f);
    __syncthreads();
    for (int t = 0; t < cn; ++t) {
      const float4 q = g[t];
      const float dx = x - q.x, dy = y - q.y, dz = z - q.z;
      const float d = (dx * dx + dy * dy) + dz * dz;
      if (d < best) { best = d; bi = c0 + t; }  // strict: the first minimum wins, as torch.argmin
    }
  }
  if (ok) atomicAdd(&counters[bi], 1.f);
}

// _jensen_shannon_divergence (jsd.py:96-107), base-2 entropies with the reference's eps handling: `_entropy` adds 1e-8
// IN PLACE, so the normalised P and Q carry it into the mixture term, which then gets its own 1e-8.
__global__ __launch_bounds__(1024) void jsd_kernel(const float* __restrict__ P, const float* __restrict__ Q, int n,
                                                   float* __restrict__ out) {
  __shared__ float red[16];
  __shared__ float bc[2];
  float sp = 0.f, sq = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) { sp += P[i]; sq += Q[i]; }
  const float tp = dg_block_sum(sp, red);
  const float tq = dg_block_sum(sq, red);
  if (threadIdx.x == 0) { bc[0] = tp; bc[1] = tq; }
  __syncthreads();
  const float SP = bc[0], SQ = bc[1];
  float e1 = 0.f, e2 = 0.f, es = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float p = P[i] / SP + 1e-8f, q = Q[i] / SQ + 1e-8f;
    const float mix = (p + q) / 2.f + 1e-8f;
    e1 -= p * log2f(p); e2 -= q * log2f(q); es -= mix * log2f(mix);
  }
  const float a = dg_block_sum(e1, red), b = dg_block_sum(e2, red), c = dg_block_sum(es, red);
  if (threadIdx.x == 0) out[0] = c - (a + b) / 2.f;
}

// --------------------------------------------------------------------------------------------------------------
// SWD descriptors (utils/metrics/swd.py:23-68): Laplacian pyramid levels and patch gathering.
// Gaussian taps [1,4,6,4,1] (x) [1,4,6,4,1] / 256 with reflect padding 2 (get_kernel :16-21, pyramid_down :24-30).
__device__ __forceinline__ int reflect_idx(int i, int n) {
  i = i < 0 ? -i : i;
  return i >= n ? 2 * n - 2 - i : i;
}
__device__ __constant__ float GAUSS5[5] = {1.f / 16.f, 4.f / 16.f, 6.f / 16.f, 4.f / 16.f, 1.f / 16.f};

// out [P,H/2,W/2] = gaussian 5x5, stride 2, of reflect-padded in [P,H,W]   (P = B*C planes)
__global__ __launch_bounds__(256) void pyr_down_kernel(const float* __restrict__ in, long planes, int H, int W,
                                                       float* __restrict__ out) {
  const int Ho = H / 2, Wo = W / 2;
  const long n = planes * Ho * Wo;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int x = (int)(i % Wo), y = (int)((i / Wo) % Ho);
  const float* src = in + (i / ((long)Wo * Ho)) * H * W;
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    const int yy = reflect_idx(2 * y + a - 2, H);
    float row = 0.f;
#pragma unroll
    for (int b = 0; b < 5; ++b) row += GAUSS5[b] * src[(long)yy * W + reflect_idx(2 * x + b - 2, W)];
    acc += GAUSS5[a] * row;
  }
  out[i] = acc;
}

// fine [P,H,W] -= pyramid_up(coarse [P,H/2,W/2])   (pyramid_up :33-42, laplacian_pyramid :45-50): zero-insertion
// puts coarse(i,j) at the ODD position (2i+1, 2j+1) of an H x W plane (the transposed conv's centre tap, last row /
// column cropped), then reflect pad 2 and the 5x5 gaussian times 4.
__global__ __launch_bounds__(256) void pyr_up_sub_kernel(float* __restrict__ fine, const float* __restrict__ coarse,
                                                         long planes, int H, int W) {
  const long n = planes * H * W;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int x = (int)(i % W), y = (int)((i / W) % H);
  const int Hc = H / 2, Wc = W / 2;
  const float* src = coarse + (i / ((long)W * H)) * Hc * Wc;
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    const int yy = reflect_idx(y + a - 2, H);
    if (!(yy & 1)) continue;
    float row = 0.f;
#pragma unroll
    for (int b = 0; b < 5; ++b) {
      const int xx = reflect_idx(x + b - 2, W);
      if (xx & 1) row += GAUSS5[b] * src[(long)(yy >> 1) * Wc + (xx >> 1)];
    }
    acc += GAUSS5[a] * row;
  }
  fine[i] -= 4.f * acc;
}

// out [B,NP,C,ph,pw] = the patches of img [B,C,H,W] whose top-left corners are inds[k] = y * (W - pw + 1) + x
// (extract_patches :53-62: unfold + index_select; the same positions for every image of the minibatch)
__global__ __launch_bounds__(256) void patches_kernel(const float* __restrict__ img, int B, int C, int H, int W, int ph,
                                                      int pw, const long* __restrict__ inds, int NP,
                                                      float* __restrict__ out) {
  const long n = (long)B * NP * C * ph * pw;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int dx = (int)(i % pw), dy = (int)((i / pw) % ph);
  const int c = (int)((i / ((long)pw * ph)) % C);
  const int k = (int)((i / ((long)pw * ph * C)) % NP);
  const int b = (int)(i / ((long)pw * ph * C * NP));
  const long pos = inds[k];
  const int nW = W - pw + 1;
  const int y = (int)(pos / nW) + dy, x = (int)(pos % nW) + dx;
  out[i] = img[(((long)b * C + c) * H + y) * W + x];
}

// --------------------------------------------------------------------------------------------------------------
// Earth mover's distance, approximate matching (utils/metrics/distance/emd/earth_mover_distance.cu:28-190 approxmatch,
// :218-262 matchcost): ten annealing levels exp(-4^j d^2), j = 7 .. -1, then 0; per level the three sweeps of the
// reference (left ratios, right consumption, matched mass).  The match matrix is never stored: matchcost is linear in
// it, so the cost sum_{k,l} match[l][k] d^2(k,l) is accumulated while the mass is produced.  One workgroup per cloud
// pair, both clouds and the four mass vectors in LDS.  (i, j) = (blockIdx.y, blockIdx.x), or the diagonal pairing
// (i = j) when `paired`.
// The sweeps are one device body for dg_emd and dg_emd_grad.  GRAD adds the gradient of matchcost with `match` held constant
// (matchcostgrad1 / matchcostgrad2, :305-388): match = sum over the levels of w, and both gradients are linear in it, so they
// are accumulated while the mass is produced, like the cost:
//   ga[k] = gscale * sum_levels sum_l w (A_k - B_l)      in the third sweep, by the thread that owns k;
//   gb[l] = gscale * sum_levels sum_k w (B_l - A_k)      in a FOURTH sweep per level, where a thread owns l and forms w again
//                                                        with the third sweep's product order (the same match bits).
// The accumulators are the output rows themselves: one thread owns row k (row l) in every level, adds the level's share to it
// and scales it after the last, so there are no atomics, no [m,n] buffer and no LDS beyond dg_emd's.  A level's share is
// summed in registers from zero and added to the row once: the steep levels leave large entries, and the later levels' small
// terms added to them one at a time would each be rounded at the row's magnitude (on 520 x 1030 points one running sum over
// all levels lay 5e-6 from the float64 gradient, the per-level sums 6e-7, which is the error of `match` itself).  The fourth sweep
// reads what the third leaves alone (the points, ratioL, ratioR), so it follows it without a barrier.
// Returns the thread's share of the cost; GRAD = false is dg_emd's arithmetic, statement for statement.
template <bool GRAD>
__device__ __forceinline__ float emd_sweeps(const float* __restrict__ a, int n, const float* __restrict__ b, int m,
                                            unsigned char* lds, float* __restrict__ ga, float* __restrict__ gb,
                                            float gscale) {
  float4* p1 = (float4*)lds;                // [n]
  float4* p2 = p1 + n;                      // [m]
  float* remainL = (float*)(p2 + m);        // [n]
  float* remainR = remainL + n;             // [m]
  float* ratioL = remainR + m;              // [n]
  float* ratioR = ratioL + n;               // [m]
  const int tid = threadIdx.x, nt = blockDim.x;
  const float multiL = n >= m ? 1.f : (float)(m / n), multiR = n >= m ? (float)(n / m) : 1.f;
  for (int k = tid; k < n; k += nt) { p1[k] = make_float4(a[k * 3], a[k * 3 + 1], a[k * 3 + 2], 0.f); remainL[k] = multiL; }
  for (int l = tid; l < m; l += nt) { p2[l] = make_float4(b[l * 3], b[l * 3 + 1], b[l * 3 + 2], 0.f); remainR[l] = multiR; }
  __syncthreads();
  float cost = 0.f;
  for (int lev = 7; lev >= -2; --lev) {
    const float level = lev == -2 ? 0.f : -powf(4.0f, (float)lev);
    for (int k = tid; k < n; k += nt) {
      const float4 x = p1[k];
      float suml = 1e-9f;
      for (int l = 0; l < m; ++l) {
        const float4 q = p2[l];
        const float d = (q.x - x.x) * (q.x - x.x) + (q.y - x.y) * (q.y - x.y) + (q.z - x.z) * (q.z - x.z);
        suml += __expf(level * d) * remainR[l];
      }
      ratioL[k] = remainL[k] / suml;
    }
    __syncthreads();
    for (int l = tid; l < m; l += nt) {
      const float4 q = p2[l];
      float sumr = 0.f;
      for (int k = 0; k < n; ++k) {
        const float4 x = p1[k];
        const float d = (q.x - x.x) * (q.x - x.x) + (q.y - x.y) * (q.y - x.y) + (q.z - x.z) * (q.z - x.z);
        sumr += __expf(level * d) * ratioL[k];
      }
      const float r = remainR[l];
      sumr *= r;
      const float consumption = fminf(r / (sumr + 1e-9f), 1.0f);
      ratioR[l] = consumption * r;
      remainR[l] = fmaxf(0.0f, r - sumr);
    }
    __syncthreads();
    for (int k = tid; k < n; k += nt) {
      const float4 x = p1[k];
      const float rl = ratioL[k];
      float suml = 0.f;
      float gx = 0.f, gy = 0.f, gz = 0.f;   // this level's share, summed on its own (see above)
      for (int l = 0; l < m; ++l) {
        const float4 q = p2[l];
        const float d = (q.x - x.x) * (q.x - x.x) + (q.y - x.y) * (q.y - x.y) + (q.z - x.z) * (q.z - x.z);
        const float w = __expf(level * d) * rl * ratioR[l];
        cost += w * d;       // matchcost (:218-262): match[l][k] * d, summed over levels
        suml += w;
        if (GRAD) { gx += w * (x.x - q.x); gy += w * (x.y - q.y); gz += w * (x.z - q.z); }
      }
      remainL[k] = fmaxf(0.0f, remainL[k] - suml);
      if (GRAD) {
        if (lev != 7) { gx += ga[k * 3]; gy += ga[k * 3 + 1]; gz += ga[k * 3 + 2]; }
        const float sc = lev == -2 ? gscale : 1.f;   // the reference scales after the sum
        ga[k * 3] = gx * sc; ga[k * 3 + 1] = gy * sc; ga[k * 3 + 2] = gz * sc;
      }
    }
    if (GRAD) {
      for (int l = tid; l < m; l += nt) {
        const float4 q = p2[l];
        const float rr = ratioR[l];
        float gx = 0.f, gy = 0.f, gz = 0.f;
        for (int k = 0; k < n; ++k) {
          const float4 x = p1[k];
          const float d = (q.x - x.x) * (q.x - x.x) + (q.y - x.y) * (q.y - x.y) + (q.z - x.z) * (q.z - x.z);
          const float w = __expf(level * d) * ratioL[k] * rr;
          gx += w * (q.x - x.x); gy += w * (q.y - x.y); gz += w * (q.z - x.z);
        }
        if (lev != 7) { gx += gb[l * 3]; gy += gb[l * 3 + 1]; gz += gb[l * 3 + 2]; }
        const float sc = lev == -2 ? gscale : 1.f;
        gb[l * 3] = gx * sc; gb[l * 3 + 1] = gy * sc; gb[l * 3 + 2] = gz * sc;
      }
    }
    __syncthreads();
  }
  return cost;
}

__global__ __launch_bounds__(512) void emd_kernel(const float* __restrict__ A, int n, const float* __restrict__ Bc,
                                                  int m, int Nb, int paired, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char emd_lds[];
  __shared__ float red[16];
  const int j = blockIdx.x, i = paired ? blockIdx.x : blockIdx.y;
  const float cost = emd_sweeps<false>(A + (long)i * n * 3, n, Bc + (long)j * m * 3, m, emd_lds, nullptr, nullptr, 0.f);
  const float tot = dg_block_sum(cost, red);
  if (threadIdx.x == 0) out[paired ? (long)i : (long)i * Nb + j] = tot;
}

// dg_emd_grad: pair i = blockIdx.x.  gscale = 2 grad_cost[i] (the 2 of d|p - q|^2, exact).
__global__ __launch_bounds__(512) void emd_grad_kernel(const float* __restrict__ A, int n, const float* __restrict__ Bc, int m,
                                                       const float* __restrict__ grad_cost, float* __restrict__ cost_out,
                                                       float* __restrict__ gradA, float* __restrict__ gradB) {
  extern __shared__ __attribute__((aligned(16))) unsigned char emd_lds[];
  __shared__ float red[16];
  const long i = blockIdx.x;
  const float gscale = 2.f * (grad_cost ? grad_cost[i] : 1.f);
  const float cost = emd_sweeps<true>(A + i * n * 3, n, Bc + i * m * 3, m, emd_lds, gradA + i * n * 3, gradB + i * m * 3, gscale);
  const float tot = dg_block_sum(cost, red);
  if (threadIdx.x == 0 && cost_out) cost_out[i] = tot;
}

// --------------------------------------------------------------------------------------------------------------
// The Chamfer extension's backward for packed clouds (chamfer_distance.cpp:82-140 / the .cu backward): point p of cloud 1 with
// neighbour k = idx1[p] in cloud 2 contributes t = 2 g1[p] (A_p - B_k) to gradA[p] - the DIRECT term, one writer per element -
// and -t to gradB[k] - the SCATTERED term, any number of writers; mirrored with g2 / idx2.  The scattered terms are summed in
// 24.40 fixed point (dg_fix40) with integer atomics, so the total does not depend on the arrival order.
// Range: unit-space points give |A_p - B_k| <= 2 per coordinate; g is the gradient of a reduction over the distances, 1 / n
// under a mean and 1 under a sum, so |t| <= 4 with room to spare in the codec's per-term window of 2^22; a point is the
// neighbour of at most 2^18 others (the entry refuses larger clouds), so |total| <= 2^20 and the word holds 2^22.
// acc: 4 u64 words per point, cloud 1's [B,n] first, then cloud 2's [B,m]: x, y, z and a flag that a term did not fit the
// window (or was not finite) - the finish then stores NaN instead of a sum with a term missing.  ZERO AT REST: the finish
// zeroes what it reads.  An index outside its cloud contributes nothing, on either side.
__global__ __launch_bounds__(256) void chamfer_bwd_scatter_kernel(const float* __restrict__ A, int n, const float* __restrict__ Bc,
                                                                  int m, int B, const float* __restrict__ g1,
                                                                  const float* __restrict__ g2, const int* __restrict__ idx1,
                                                                  const int* __restrict__ idx2, float* __restrict__ gradA,
                                                                  float* __restrict__ gradB,
                                                                  unsigned long long* __restrict__ acc) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per = (long)n + m;
  if (t >= B * per) return;
  const long b = t / per;
  const int r = (int)(t - b * per);
  const bool first = r < n;                                   // a point of cloud 1 (else of cloud 2)
  const int p = first ? r : r - n, np = first ? n : m, nq = first ? m : n;
  const long bp = b * np + p;
  const float* P = (first ? A : Bc) + bp * 3;
  float* gd = (first ? gradA : gradB) + bp * 3;
  const int k = (first ? idx1 : idx2)[bp];
  if (k < 0 || k >= nq) { gd[0] = 0.f; gd[1] = 0.f; gd[2] = 0.f; return; }
  const float* Q = (first ? Bc : A) + (b * nq + k) * 3;
  const float g = 2.f * (first ? g1 : g2)[bp];
  unsigned long long* cell = acc + ((first ? (long)B * n : 0l) + b * nq + k) * 4;   // the neighbour's words
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = g * (P[c] - Q[c]);
    gd[c] = v;
    long long q;
    if (!dg_fix40(-(double)v, q)) atomicOr(cell + 3, 1ull);
    else if (q != 0) atomicAdd(cell + c, (unsigned long long)q);
  }
}

// grad = direct + scattered, rounded to float once; the words go back to zero
__global__ __launch_bounds__(256) void chamfer_bwd_finish_kernel(long points_a, long points, float* __restrict__ gradA,
                                                                 float* __restrict__ gradB,
                                                                 unsigned long long* __restrict__ acc) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= points) return;
  float* gd = t < points_a ? gradA + t * 3 : gradB + (t - points_a) * 3;
  unsigned long long* cell = acc + t * 4;
  const unsigned long long w0 = cell[0], w1 = cell[1], w2 = cell[2], bad = cell[3];
  if (w0 | w1 | w2 | bad) { cell[0] = 0ull; cell[1] = 0ull; cell[2] = 0ull; cell[3] = 0ull; }
  const float nan = __builtin_nanf("");
  gd[0] = bad ? nan : (float)((double)gd[0] + dg_fix40_value((long long)w0));
  gd[1] = bad ? nan : (float)((double)gd[1] + dg_fix40_value((long long)w1));
  gd[2] = bad ? nan : (float)((double)gd[2] + dg_fix40_value((long long)w2));
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

int dg_chamfer_dir(const float* A, int Na, int n, const float* Bc, int Nb, int m, float* L, void* s_) {
  if (!A || !Bc || !L || Na <= 0 || Nb <= 0 || n <= 0 || m <= 0) return DG_EINVAL;
  hipStream_t s = (hipStream_t)s_;
  int wpc = (n + CH_WPTS - 1) / CH_WPTS;        // waves per cloud
  if (wpc > 2) wpc = (wpc + 3) / 4 * 4;         // 1, 2 or whole workgroups
  const int gy = wpc >= 4 ? Na : (Na + 4 / wpc - 1) / (4 / wpc);
  const int gz = wpc >= 4 ? wpc / 4 : 1;
  if (wpc > 1) { const int zrc = dg_zero_f32(L, (long)Na * Nb, s); if (zrc) return zrc; }
  // TB clouds of B per workgroup: long enough to amortise the A registers, short enough for >= ~8 workgroups per CU
  int TB = 32;
  while (TB > 1 && (long)((Nb + TB - 1) / TB) * gy * gz < 2048) TB >>= 1;
  const dim3 grid((Nb + TB - 1) / TB, gy, gz);
  if (grid.y > 65535 || grid.z > 65535) return DG_EUNSUPPORTED;
  chamfer_dir_kernel<false><<<grid, CH_THREADS, 0, s>>>(A, Na, n, wpc, Bc, Nb, m, TB, L);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_chamfer_paired(const float* A, int n, const float* Bc, int m, int B, float* L, void* s_) {
  if (!A || !Bc || !L || B <= 0 || n <= 0 || m <= 0) return DG_EINVAL;
  hipStream_t s = (hipStream_t)s_;
  // whole workgroups per cloud (a workgroup streams ONE cloud B_i); slices past n hold no points and store nothing
  const int wpc = (n + 4 * CH_WPTS - 1) / (4 * CH_WPTS) * 4;
  if (B > 65535 || wpc / 4 > 65535) return DG_EUNSUPPORTED;
  const int zrc = dg_zero_f32(L, B, s);
  if (zrc) return zrc;
  chamfer_dir_kernel<true><<<dim3(1, B, wpc / 4), CH_THREADS, 0, s>>>(A, B, n, wpc, Bc, B, m, 1, L);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_chamfer_nn(const float* A, long a_sb, long a_sp, long a_sc, int n, const float* Bc, long b_sb, long b_sp, long b_sc,
                  int m, int B, float* dist, int* idx, void* s_) {
  if (!A || !Bc || !dist || !idx || B <= 0 || n <= 0 || m <= 0) return DG_EINVAL;
  if (a_sp <= 0 || a_sc <= 0 || b_sp <= 0 || b_sc <= 0 || a_sb < 0 || b_sb < 0) return DG_EINVAL;
  // 2^18 points per cloud: what the fixed-point sums behind the search (dg_inv_chamfer_grad) are sized for
  if (n > (1 << 18) || m > (1 << 18)) return DG_EUNSUPPORTED;
  if (a_sp > 0x7fffffffL || a_sc > 0x3fffffffL || b_sp > 0x7fffffffL || b_sc > 0x3fffffffL) return DG_EUNSUPPORTED;
  const int wgs = (n + 4 * CH_WPTS - 1) / (4 * CH_WPTS);   // whole workgroups per cloud, as dg_chamfer_paired
  if (B > 65535 || wgs > 65535) return DG_EUNSUPPORTED;
  chamfer_nn_kernel<<<dim3(1, B, wgs), CH_THREADS, 0, (hipStream_t)s_>>>(A, a_sb, (int)a_sp, (int)a_sc, n, Bc, b_sb,
                                                                        (int)b_sp, (int)b_sc, m, dist, idx);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_grid_vote(const float* pts, long P, const float* grid, int Ng, float* counters, void* s_) {
  if (!pts || !grid || !counters || P <= 0 || Ng <= 0) return DG_EINVAL;
  grid_vote_kernel<<<(unsigned)((P + 255) / 256), 256, 0, (hipStream_t)s_>>>(pts, P, grid, Ng, counters);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_jsd(const float* P, const float* Q, int n, float* out, void* s_) {
  if (!P || !Q || !out || n <= 0) return DG_EINVAL;
  jsd_kernel<<<1, 1024, 0, (hipStream_t)s_>>>(P, Q, n, out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_pyr_down(const float* in, long planes, int H, int W, float* out, void* s_) {
  if (!in || !out || planes <= 0 || H < 4 || W < 4 || (H & 1) || (W & 1)) return DG_EINVAL;
  const long n = planes * (H / 2) * (W / 2);
  pyr_down_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)s_>>>(in, planes, H, W, out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_pyr_up_sub(float* fine, const float* coarse, long planes, int H, int W, void* s_) {
  if (!fine || !coarse || planes <= 0 || H < 4 || W < 4 || (H & 1) || (W & 1)) return DG_EINVAL;
  const long n = planes * H * W;
  pyr_up_sub_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)s_>>>(fine, coarse, planes, H, W);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_extract_patches(const float* img, int B, int C, int H, int W, int ph, int pw, const long* inds, int NP,
                       float* out, void* s_) {
  if (!img || !inds || !out || B <= 0 || C <= 0 || ph <= 0 || pw <= 0 || ph > H || pw > W || NP <= 0) return DG_EINVAL;
  const long n = (long)B * NP * C * ph * pw;
  patches_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)s_>>>(img, B, C, H, W, ph, pw, inds, NP, out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_emd(const float* A, int Na, int n, const float* Bc, int Nb, int m, int paired, float* out, void* s_) {
  if (!A || !Bc || !out || Na <= 0 || Nb <= 0 || n <= 0 || m <= 0) return DG_EINVAL;
  if (paired && Na != Nb) return DG_EINVAL;
  const size_t lds = (size_t)(n + m) * (16 + 8);
  if (lds > 150 * 1024) return DG_EUNSUPPORTED;
  static bool opted = false;
  if (!opted) {
    HIP_CHECK_RET(hipFuncSetAttribute((const void*)emd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
    opted = true;
  }
  const dim3 grid(Nb, paired ? 1 : Na);
  if (grid.y > 65535) return DG_EUNSUPPORTED;
  emd_kernel<<<grid, 512, lds, (hipStream_t)s_>>>(A, n, Bc, m, Nb, paired, out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_emd_grad(const float* A, int n, const float* Bc, int m, int B, const float* grad_cost, float* cost, float* gradA,
                float* gradB, void* s_) {
  if (!A || !Bc || !gradA || !gradB || B <= 0 || n <= 0 || m <= 0) return DG_EINVAL;
  const size_t lds = (size_t)(n + m) * (16 + 8);   // dg_emd's: the gradient rows are the accumulators
  if (lds > 150 * 1024) return DG_EUNSUPPORTED;
  static bool opted = false;
  if (!opted) {
    HIP_CHECK_RET(hipFuncSetAttribute((const void*)emd_grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
    opted = true;
  }
  emd_grad_kernel<<<B, 512, lds, (hipStream_t)s_>>>(A, n, Bc, m, grad_cost, cost, gradA, gradB);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_chamfer_backward(const float* A, int n, const float* Bc, int m, int B, const float* g1, const float* g2, const int* idx1,
                        const int* idx2, float* gradA, float* gradB, unsigned long long* acc, void* s_) {
  if (!A || !Bc || !g1 || !g2 || !idx1 || !idx2 || !gradA || !gradB || !acc || B <= 0 || n <= 0 || m <= 0) return DG_EINVAL;
  if (n > (1 << 18) || m > (1 << 18)) return DG_EUNSUPPORTED;   // the codec's range, as dg_chamfer_nn
  const long points = (long)B * ((long)n + m);
  const long blocks = (points + 255) / 256;
  if (blocks > 0x7fffffffL) return DG_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)s_;
  chamfer_bwd_scatter_kernel<<<(unsigned)blocks, 256, 0, s>>>(A, n, Bc, m, B, g1, g2, idx1, idx2, gradA, gradB, acc);
  HIP_CHECK_RET(hipGetLastError());
  chamfer_bwd_finish_kernel<<<(unsigned)blocks, 256, 0, s>>>((long)B * n, points, gradA, gradB, acc);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

}  // extern "C"
