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
//     not small against a squared pixel pitch (9e-6 at W = 2048).  The stream and the rescan of the first chunk that attains the
//     minimum are nn_stream.h's, shared with chamfer_nn_kernel (point_chamfer.hip): the project's tie rule.  The same lane then
//     adds (w d_u, w) to the two u64 words of pixel id in 24.40 fixed point (dg_fix40) with integer atomics.  d_u, not d_m: a term
//     stays <= 1, inside dg_fix40's range analysis (<= 2^18 points per cloud: a total <= 2^58); the finish multiplies by
//     max_depth.  Integer adds are associative, so the image is bit-identical for any permutation of the points and a graph
//     replay equals an eager launch.  Resolution: tau <= 16 keeps w >= e^-16 = 1.1e-7 = 2^-23.1, 17 bits above the 2^-40 quantum
//     (a relative 4e-6 per term at that extreme; at the reference's tau = 2, w >= 0.135 and a term keeps 37 bits).
//     Per-point arithmetic (norm, range test, atan2, exp) is DOUBLE on the float32 coordinates: the range test is a
//     discontinuity, and per point it is a few hundred flops against 5 H W in the search.
//   * finish : ratio, valid, normalised depth, drop_value fill; zeroes the words (ZERO AT REST, as dg_splat_accum's).
#include "common.h"
#include "nn_stream.h"
#include "points_body.h"

namespace {

constexpr int PD_THREADS = 256;
constexpr int PD_PT = 4;                      // points per lane
constexpr int PD_WPTS = 64 * PD_PT;           // points per wave
constexpr int PD_BPTS = 4 * PD_WPTS;          // points per workgroup
constexpr int PD_MC = 512;                    // pixels per LDS chunk (4 KB), two buffers

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
  f2 pa[2][PD_PT / 2];   // (u, v)
  unsigned part = 0;   // bit e: point p0 + e takes part
#pragma unroll
  for (int e = 0; e < PD_PT; ++e) {
    float u = 0.f, v = 0.f;
    double wd, w;
    if (p0 + e < nb && pd_point(cloud + (long)(p0 + e) * stride, min_depth, max_depth, tau, u, v, wd, w)) part |= 1u << e;
    else u = v = 0.f;   // an idle slot searches for (0, 0) and stores nothing
    pa[0][e >> 1][e & 1] = u;
    pa[1][e >> 1][e & 1] = v;
  }
  const float* U = angle;
  const float* V = angle + HW;
  auto load = [&](int k, float (&q)[2]) { q[0] = U[k]; q[1] = V[k]; };
  f2 rmin[PD_PT / 2];
  int wch[PD_PT];
  nn_stream_first<2, PD_PT, PD_MC, PD_THREADS, 4>(load, HW, qbuf, pa, rmin, wch);
  // the first minimum inside the winning chunk, then the sums
  unsigned long long* img = acc + (long)b * HW * 2;
#pragma unroll
  for (int e = 0; e < PD_PT; ++e) {
    const int p = p0 + e;
    if (p >= N) continue;
    int id = -1;
    if (part >> e & 1) {
      const float x[2] = {pa[0][e >> 1][e & 1], pa[1][e >> 1][e & 1]};
      id = nn_first_in_chunk<2, PD_MC>(load, HW, wch[e], x);
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
  if (hw > DG_FIX40_MAX_TERMS || N > DG_FIX40_MAX_TERMS) return DG_EUNSUPPORTED;   // points per cloud and pixels per image
  hipStream_t s = (hipStream_t)s_;
  points_search_kernel<<<dim3((N + PD_BPTS - 1) / PD_BPTS, B), PD_THREADS, 0, s>>>(rec, rec_sb, stride, counts, N, angle, (int)hw,
                                                                                 min_depth, max_depth, tau, acc, idx);
  HIP_CHECK_RET(hipGetLastError());
  const long total = (long)B * hw;
  points_finish_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(acc, total, min_depth, max_depth, drop_value, depth, valid);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}
