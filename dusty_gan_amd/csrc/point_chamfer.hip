// Chamfer distance between point clouds (the reference's native CUDA extension
// utils/metrics/distance/cd/chamfer_distance.{cu,cpp}), gfx950:
//   * chamfer_dir_kernel : ALL-PAIRS directed Chamfer means  L[i][j] = mean_{p in A_i} min_{q in B_j} |p - q|^2, or the paired
//                          means L[i] (dg_chamfer_dir, dg_chamfer_paired).  The reference (nnsearch :41-66) as driven by
//                          utils/metrics/cov_mmd_1nna.py:20-52 loops i in Python and calls the extension on (cloud i expanded) x
//                          (512 clouds) -- N^2 / 512 launches.  Here one launch fills a whole [Na,Nb] matrix;
//                          CD(i,j) = L_AB[i][j] + L_BA[j][i].
//   * chamfer_nn_kernel  : the paired nearest-neighbour search with indices (dg_chamfer_nn).
//   * chamfer_bwd_scatter_kernel, chamfer_bwd_finish_kernel : the extension's backward (dg_chamfer_backward).
// The searches are VALU-bound fp32 work (K = 3: no matrix-core shape) on the streamed search of nn_stream.h: PT points of cloud A
// per lane in registers, cloud B through LDS with broadcast 16-byte reads, two points per packed instruction.
#include "common.h"
#include "nn_stream.h"

namespace {

// Directed Chamfer means, all pairs.
// Work split: a WAVE owns 512 consecutive points of one cloud A_i (8 per lane, as 4 packed pairs, in registers for the
// whole kernel) and their running minima; a workgroup is 4 waves = 4 clouds (n <= 512), 2 clouds (n <= 1024) or a
// 2048-point slice of one cloud (larger n: blockIdx.z walks the slices and the partial means are added atomically).
// The workgroup streams TB clouds B_j through LDS in chunks of MC points (nn_stream.h: x, y, z as 16 bytes, double-buffered,
// broadcast reads).  Per point pair: 6 packed fp32 instructions per two pairs + one v_min each = 4 lane-ops.
constexpr int CH_THREADS = 256;
constexpr int CH_PT = 8;                 // points of A per lane
constexpr int CH_WPTS = 64 * CH_PT;      // points of A per wave
constexpr int CH_MC = 512;               // points of B per LDS chunk (8 KB), two buffers

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
  f2 pa[3][CH_PT / 2];
  const float* a = A + (long)(live ? i : 0) * n * 3;
#pragma unroll
  for (int h = 0; h < CH_PT / 2; ++h) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int p = p0 + 2 * h + e;
      const int pp = p < n ? p : 0;  // out-of-range slots replicate point 0; their minima are dropped from the sum
      pa[0][h][e] = a[pp * 3 + 0];
      pa[1][h][e] = a[pp * 3 + 1];
      pa[2][h][e] = a[pp * 3 + 2];
    }
  }
  const int j0 = PAIRED ? i : blockIdx.x * TB, j1 = PAIRED ? i + 1 : min(Nb, j0 + TB);
  const int nchunk = (m + CH_MC - 1) / CH_MC;
  const int total = (j1 - j0) * nchunk;  // (cloud, chunk) steps of this workgroup
  // The walk is over (cloud, chunk) steps - a reset at a cloud's chunk 0, a wave sum at its last chunk - so it is not
  // nn_stream_first's; the chunk filler and the inner loop are the shared ones.
  float r[CH_MC / CH_THREADS][3];
  auto fetch = [&](int step) {
    const float* q = Bc + (long)(j0 + step / nchunk) * m * 3;
    nn_fetch<3, CH_MC, CH_THREADS>(
        [&](int k, float (&v)[3]) { v[0] = q[k * 3 + 0]; v[1] = q[k * 3 + 1]; v[2] = q[k * 3 + 2]; }, step % nchunk, m, r);
  };
  f2 rmin[CH_PT / 2];
  if (total > 0) { fetch(0); nn_commit<3, CH_MC, CH_THREADS>(r, qbuf[0]); }
  __syncthreads();
  for (int step = 0; step < total; ++step) {
    const int buf = step & 1, c = step % nchunk;
    if (c == 0) {
#pragma unroll
      for (int h = 0; h < CH_PT / 2; ++h) rmin[h] = (f2){3.0e38f, 3.0e38f};
    }
    if (step + 1 < total) fetch(step + 1);
    nn_chunk_min<3, CH_PT, CH_MC, 2>(qbuf[buf], pa, rmin);
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
    if (step + 1 < total) nn_commit<3, CH_MC, CH_THREADS>(r, qbuf[buf ^ 1]);
    __syncthreads();
  }
}

// --------------------------------------------------------------------------------------------------------------
// Paired nearest-neighbour search WITH indices (chamfer_distance.cu:9-127 / nnsearch chamfer_distance.cpp:39-62):
// dist[i][p] = min_q |A_i[p] - B_i[q]|^2, idx[i][p] = the LOWEST q attaining it.  The work split and the inner loop are
// chamfer_dir_kernel<true>'s (a wave owns 512 points of A in registers, B_i streamed through the double-buffered LDS chunks,
// nn_chunk_min per chunk: a distance here is the one dg_chamfer_paired sums, bit for bit).  The stream and the rescan of the
// winning chunk (from global memory: the chunks differ lane to lane) are nn_stream.h's, tie rule included - the reference's.
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
  f2 pa[3][CH_PT / 2];
  const float* a = A + (long)i * a_sb;
  const float* q = Bc + (long)i * b_sb;
#pragma unroll
  for (int h = 0; h < CH_PT / 2; ++h) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int p = p0 + 2 * h + e;
      const long pp = (long)(p < n ? p : 0) * a_sp;  // out-of-range slots replicate point 0 and store nothing
      pa[0][h][e] = a[pp];
      pa[1][h][e] = a[pp + a_sc];
      pa[2][h][e] = a[pp + 2l * a_sc];
    }
  }
  auto load = [&](int k, float (&v)[3]) {
    const long kk = (long)k * b_sp;
    v[0] = q[kk]; v[1] = q[kk + b_sc]; v[2] = q[kk + 2l * b_sc];
  };
  f2 rmin[CH_PT / 2];
  int wch[CH_PT];
  nn_stream_first<3, CH_PT, CH_MC, CH_THREADS, 2>(load, m, qbuf, pa, rmin, wch);
  // the first minimum inside the winning chunk; the distance stored is the streamed one
#pragma unroll
  for (int h = 0; h < CH_PT / 2; ++h) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int p = p0 + 2 * h + e;
      if (p >= n) continue;
      const float x[3] = {pa[0][h][e], pa[1][h][e], pa[2][h][e]};
      const int bi = nn_first_in_chunk<3, CH_MC>(load, m, wch[2 * h + e], x);
      dist[(long)i * n + p] = rmin[h][e];
      idx[(long)i * n + p] = bi;
    }
  }
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
    if (!dg_fix40_add(cell + c, -(double)v)) atomicOr(cell + 3, 1ull);
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
  // what the fixed-point sums behind the search (dg_inv_chamfer_grad) are sized for
  if (n > DG_FIX40_MAX_TERMS || m > DG_FIX40_MAX_TERMS) return DG_EUNSUPPORTED;
  if (a_sp > 0x7fffffffL || a_sc > 0x3fffffffL || b_sp > 0x7fffffffL || b_sc > 0x3fffffffL) return DG_EUNSUPPORTED;
  const int wgs = (n + 4 * CH_WPTS - 1) / (4 * CH_WPTS);   // whole workgroups per cloud, as dg_chamfer_paired
  if (B > 65535 || wgs > 65535) return DG_EUNSUPPORTED;
  chamfer_nn_kernel<<<dim3(1, B, wgs), CH_THREADS, 0, (hipStream_t)s_>>>(A, a_sb, (int)a_sp, (int)a_sc, n, Bc, b_sb,
                                                                        (int)b_sp, (int)b_sc, m, dist, idx);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_chamfer_backward(const float* A, int n, const float* Bc, int m, int B, const float* g1, const float* g2, const int* idx1,
                        const int* idx2, float* gradA, float* gradB, unsigned long long* acc, void* s_) {
  if (!A || !Bc || !g1 || !g2 || !idx1 || !idx2 || !gradA || !gradB || !acc || B <= 0 || n <= 0 || m <= 0) return DG_EINVAL;
  if (n > DG_FIX40_MAX_TERMS || m > DG_FIX40_MAX_TERMS) return DG_EUNSUPPORTED;
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
