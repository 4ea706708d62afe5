// An arbitrary point cloud onto the model's range image (gfx950).  Reference: Coordinate.points_to_depth, utils/lidar.py:70-107,
// over render.bilinear_rasterizer (utils/render.py:67-127): there a [B,N,HW,2] difference tensor, its norm, a min, an embedding and
// two float scatter_add_ images.  For a point p of a cloud in unit space (metres / max_depth):
//     d_u = |p|, d_m = d_u max_depth, w = exp(-tau d_u) [min_depth < d_m < max_depth]               (both strict)      :78-81
//     u = atan2(z, hypot(x, y)), v = atan2(y, x)                                                                     :83-84
//     id = argmin over the H W pixels of (u - U_p)^2 + (v - V_p)^2, the LOWEST index on a tie                        :89
//     depth_2d[id] = sum w d_m / (sum w + 1e-8); valid = depth_2d != 0                                               :101-103
//     out = (depth_2d - min_depth) / (max_depth - min_depth) where valid, drop_value elsewhere                       :104-105
// The reference hands INTEGER pixel coordinates to its rasterizer: the bottom / right corner weights are exactly zero and the
// splat is a plain scatter-add of weight 1 onto pixel id.  Line 104 calls `self.minmax_norm`, which does not exist (the function
// raises as shipped); `normalize_minmax` is the call that was meant and what is built here.
// NO AZIMUTH WRAP-AROUND: the distance is the plain difference of angles, as in the reference.  A pixel row ends half a pixel
// from +-pi, so a point just across the seam is still nearest to the row's end pixel on its own side: nothing is lost.
// DEVIATION: a point with a non-finite coordinate takes no part (weight 0; the reference's NaN would poison its pixel), nor does
// the origin (d_m = 0 fails the range test whenever min_depth >= 0, which the entry point requires).
//   * search : a wave owns 256 consecutive points of one cloud, 4 per lane as 2 packed pairs of (u, v) in registers; a workgroup
//     (4 waves, 1024 points) streams the grid's (U, V) pairs through double-buffered LDS chunks of PD_MC pixels, every lane reading
//     the SAME address (broadcast).  The distance is formed from DIFFERENCES - 2 packed subtractions, a packed multiply, a packed
//     fma, 2 minima per two pairs - never from the expanded |a|^2 + |b|^2 - 2ab, whose fp32 error with angles up to pi (~1e-6) is
//     not small against a squared pixel pitch (9e-6 at W = 2048).  The loop tracks the minimum only; per point and chunk one strict
//     compare notes the FIRST chunk that attains the final minimum, and the lane rescans that chunk (from global memory) for the
//     first minimum, strict `<` over ascending indices: the project's tie rule (chamfer_nn_kernel, metrics.hip).  The same lane then
//     adds (w d_u, w) to the two u64 words of pixel id in 24.40 fixed point (dg_fix40) with integer atomics.  d_u, not d_m: a term
//     stays <= 1, inside dg_fix40's range analysis (<= 2^18 points per cloud: a total <= 2^58); the finish multiplies by
//     max_depth.  Integer adds are associative, so the image is bit-identical for any permutation of the points and a graph
//     replay equals an eager launch.  Resolution: tau <= 16 keeps w >= e^-16 = 1.1e-7 = 2^-23.1, 17 bits above the 2^-40 quantum
//     (a relative 4e-6 per term at that extreme; at the reference's tau = 2, w >= 0.135 and a term keeps 37 bits).
//     Per-point arithmetic (norm, range test, atan2, exp) is DOUBLE on the float32 coordinates: the range test is a
//     discontinuity, and per point it is a few hundred flops against 5 H W in the search.
//   * finish : ratio, valid, normalised depth, drop_value fill; zeroes the words (ZERO AT REST, as dg_splat_accum's).
#include "common.h"
#include "points_body.h"

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int PD_THREADS = 256;
constexpr int PD_PT = 4;                      // points per lane
constexpr int PD_WPTS = 64 * PD_PT;           // points per wave
constexpr int PD_BPTS = 4 * PD_WPTS;          // points per workgroup
constexpr int PD_MC = 512;                    // pixels per LDS chunk (4 KB), two buffers
constexpr int PD_LD = PD_MC / PD_THREADS;     // chunk pixels loaded per thread
#define PD_MAX (1l << 18)                     // points per cloud (dg_fix40's range analysis) and pixels per image

// (pd_point, the per-point body, lives in points_body.h: raydrop.hip's pixel winner shares it)

__global__ __launch_bounds__(PD_THREADS) void points_search_kernel(const float* __restrict__ rec, long rec_sb, int stride,
                                                                   const int* __restrict__ counts, int N,
                                                                   const float* __restrict__ angle, int HW, double min_depth,
                                                                   double max_depth, double tau,
                                                                   unsigned long long* __restrict__ acc, int* __restrict__ idx) {
  __shared__ float2 qbuf[2][PD_MC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y;
  const int nb = counts ? min(max(counts[b], 0), N) : N;
  const int p0 = blockIdx.x * PD_BPTS + wave * PD_WPTS + lane * PD_PT;
  const float* cloud = rec + (long)b * rec_sb;
  if (blockIdx.x * PD_BPTS >= nb) {   // (block-uniform) nothing of this cloud here: records at and beyond counts[b] are not read
    if (idx)
      for (int e = 0; e < PD_PT; ++e)
        if (p0 + e < N) idx[(long)b * N + p0 + e] = -1;
    return;
  }
  f2 pu[PD_PT / 2], pv[PD_PT / 2];
  unsigned part = 0;   // bit e: point p0 + e takes part
#pragma unroll
  for (int e = 0; e < PD_PT; ++e) {
    float u = 0.f, v = 0.f;
    double wd, w;
    if (p0 + e < nb && pd_point(cloud + (long)(p0 + e) * stride, min_depth, max_depth, tau, u, v, wd, w)) part |= 1u << e;
    else u = v = 0.f;   // an idle slot searches for (0, 0) and stores nothing
    pu[e >> 1][e & 1] = u;
    pv[e >> 1][e & 1] = v;
  }
  const float* U = angle;
  const float* V = angle + HW;
  const int nchunk = (HW + PD_MC - 1) / PD_MC;
  float r[PD_LD][2];
  auto fetch = [&](int c) {
#pragma unroll
    for (int k = 0; k < PD_LD; ++k) {
      const int p = c * PD_MC + k * PD_THREADS + tid;
      const int pp = p < HW ? p : 0;   // the last chunk's tail repeats pixel 0: chunk 0 holds it first
      r[k][0] = U[pp]; r[k][1] = V[pp];
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int k = 0; k < PD_LD; ++k) qbuf[buf][k * PD_THREADS + tid] = make_float2(r[k][0], r[k][1]);
  };
  f2 rmin[PD_PT / 2];
  int wch[PD_PT];
#pragma unroll
  for (int h = 0; h < PD_PT / 2; ++h) {
    rmin[h] = (f2){3.0e38f, 3.0e38f};
    wch[2 * h] = 0; wch[2 * h + 1] = 0;
  }
  fetch(0);
  commit(0);
  __syncthreads();
  for (int c = 0; c < nchunk; ++c) {
    const int buf = c & 1;
    if (c + 1 < nchunk) fetch(c + 1);
    f2 was[PD_PT / 2];
#pragma unroll
    for (int h = 0; h < PD_PT / 2; ++h) was[h] = rmin[h];
#pragma unroll 4
    for (int t = 0; t < PD_MC; ++t) {
      const float2 q = qbuf[buf][t];
      const f2 qu = (f2){q.x, q.x}, qv = (f2){q.y, q.y};
#pragma unroll
      for (int h = 0; h < PD_PT / 2; ++h) {
        const f2 du = qu - pu[h], dv = qv - pv[h];
        f2 d = du * du;
        d = __builtin_elementwise_fma(dv, dv, d);
        rmin[h][0] = __builtin_fminf(rmin[h][0], d[0]);
        rmin[h][1] = __builtin_fminf(rmin[h][1], d[1]);
      }
    }
#pragma unroll
    for (int h = 0; h < PD_PT / 2; ++h) {
      if (rmin[h][0] < was[h][0]) wch[2 * h] = c;
      if (rmin[h][1] < was[h][1]) wch[2 * h + 1] = c;
    }
    if (c + 1 < nchunk) commit(buf ^ 1);
    __syncthreads();
  }
  // the first minimum inside the winning chunk (the same operations as the stream: the same distances, bit for bit), then the sums
  unsigned long long* img = acc + (long)b * HW * 2;
#pragma unroll
  for (int e = 0; e < PD_PT; ++e) {
    const int p = p0 + e;
    if (p >= N) continue;
    int id = -1;
    if (part >> e & 1) {
      const int k0 = wch[e] * PD_MC, k1 = min(HW, k0 + PD_MC);
      const float u = pu[e >> 1][e & 1], v = pv[e >> 1][e & 1];
      float best = 3.0e38f;
      id = k0;
      for (int k = k0; k < k1; ++k) {
        const float du = U[k] - u, dv = V[k] - v;
        float d = du * du;
        d = __builtin_fmaf(dv, dv, d);
        if (d < best) { best = d; id = k; }
      }
      float uu, vv;
      double wd, w;
      pd_point(cloud + (long)p * stride, min_depth, max_depth, tau, uu, vv, wd, w);
      long long q1, q0;
      if (dg_fix40(wd, q1) && dg_fix40(w, q0)) {
        atomicAdd(img + 2l * id, (unsigned long long)q1);
        atomicAdd(img + 2l * id + 1, (unsigned long long)q0);
      }
    }
    if (idx) idx[(long)b * N + p] = id;
  }
}

__global__ __launch_bounds__(256) void points_finish_kernel(unsigned long long* __restrict__ acc, long total, double min_depth,
                                                            double max_depth, float drop_value, float* __restrict__ depth,
                                                            unsigned char* __restrict__ valid) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const double swd = dg_fix40_value((long long)acc[2 * i]), sw = dg_fix40_value((long long)acc[2 * i + 1]);
  acc[2 * i] = 0ull;
  acc[2 * i + 1] = 0ull;
  const double depth_2d = swd * max_depth / (sw + 1e-8);
  const bool ok = depth_2d != 0.0;
  depth[i] = ok ? (float)((depth_2d - min_depth) / (max_depth - min_depth)) : drop_value;
  valid[i] = ok ? 1 : 0;
}

}  // namespace

extern "C" int dg_points_to_depth(const float* rec, long rec_sb, int stride, const int* counts, int B, int N, const float* angle,
                                  int H, int W, double min_depth, double max_depth, double tau, float drop_value,
                                  unsigned long long* acc, float* depth, unsigned char* valid, int* idx, void* s_) {
  if (!rec || !angle || !acc || !depth || !valid || B <= 0 || B > 65535 || N <= 0 || H <= 0 || W <= 0) return DG_EINVAL;
  if ((stride != 3 && stride != 4) || rec_sb < (long)N * stride) return DG_EINVAL;
  if (!(min_depth >= 0.0 && max_depth > min_depth && max_depth < INFINITY) || !(tau >= 0.0 && tau <= 16.0)) return DG_EINVAL;
  const long hw = (long)H * W;
  if (hw > PD_MAX || N > PD_MAX) return DG_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)s_;
  points_search_kernel<<<dim3((N + PD_BPTS - 1) / PD_BPTS, B), PD_THREADS, 0, s>>>(rec, rec_sb, stride, counts, N, angle, (int)hw,
                                                                                 min_depth, max_depth, tau, acc, idx);
  HIP_CHECK_RET(hipGetLastError());
  const long total = (long)B * hw;
  points_finish_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(acc, total, min_depth, max_depth, drop_value, depth, valid);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}
