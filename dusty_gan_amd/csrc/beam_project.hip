// Unordered clouds of ANY spinning LiDAR -> the dataset's files (gfx950): what scan_project.hip does for HDL-64E scans in
// KITTI's file order, without the file order.  The reference holds no code for it: its rows come from the azimuth wrap of
// consecutive records (process_kitti.py:90-106), which only that one recording format has.  DESIGN.md 7m.
//   * elev_hist    : the histogram of the points' elevations u = atan2(z, |xy|) over [lo, hi) in NB bins, for the points with
//     min_depth < |xyz| < max_depth.  The host clusters it into the sensor's beam table (datasets/beams.py).  A workgroup
//     counts into its own NB u32 words of LDS, then adds its non-zero bins to the caller's u64 words: one global integer
//     atomic per non-zero bin per workgroup.  Integer counts: the result depends neither on the chunking nor on scheduling.
//   * beam_project : S clouds (concatenated [N,4] points + [S+1] offsets) -> [S,H,W,4] projections.  Three launches, as
//     scan_project: key fill, scatter, gather (the first and the last ARE scan_project's, scan_cell.h).
//       row    the beam nearest to u, in double; on an exact tie the LOWER row.  Binary search over the table in LDS.
//       column scan_project's float32 expression (sc_column)
//       cell   keeps its NEAREST point: 64-bit atomicMin of (float32 range bits << 32 | point index within the scan) - on a
//              range tie the LOWER index (sc_key)
// Per-point quantities as points_body.h forms them: double arithmetic on the float32 coordinates, the range rounded once to
// float32 where it becomes a key.  A point with a non-finite coordinate, or at the origin, takes no part anywhere.
// HBM-bound by bytes (16 per point in; 8 of key + 16 out per cell), with a double-precision atan2 per point on top.
#include "common.h"
#include "points_body.h"
#include "scan_cell.h"

namespace {

#define HIST_THREADS 1024
#define HIST_GRID 256        // one workgroup per CU: the fewer workgroups, the fewer global atomics per non-zero bin
#define BEAM_THREADS 256
#define BEAM_SPLIT 64        // workgroups per cloud (one with no tile of its own leaves at once)
#define BEAM_MAX_H 256

struct BeamTable {
  double b[BEAM_MAX_H];      // by value in the kernel's arguments: validated on the host, no copy to wait for
};

// one record -> does the point take part?  u = its elevation, d = its range (metres), both in double
__device__ __forceinline__ bool beam_point(const float4 v, double& u, double& d) {
  const float rec[3] = {v.x, v.y, v.z};
  double x, y, z, r2;
  d = pd_range(rec, x, y, z, r2);
  if (!(d > 0.0 && d < __builtin_inf())) return false;   // the origin; an infinite or NaN coordinate
  u = atan2(z, sqrt(r2));
  return true;
}

__global__ __launch_bounds__(HIST_THREADS) void elev_hist_kernel(const float* __restrict__ points,
                                                                 const long* __restrict__ offsets, int S, double min_depth,
                                                                 double max_depth, double lo, double hi, double scale, int NB,
                                                                 unsigned long long* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) unsigned lh[];   // [NB]
  const long first = offsets[0], n = offsets[S] - first;          // the clouds lie back to back
  const long start = (long)blockIdx.x * HIST_THREADS;
  if (start >= n) return;                                         // (the whole workgroup: nothing to count, nothing to add)
  for (int b = threadIdx.x; b < NB; b += HIST_THREADS) lh[b] = 0u;
  __syncthreads();
  const float4* p = reinterpret_cast<const float4*>(points) + first;
  for (long i = start + threadIdx.x; i < n; i += (long)HIST_GRID * HIST_THREADS) {
    double u, d;
    if (!beam_point(p[i], u, d)) continue;
    if (!(d > min_depth && d < max_depth && u >= lo && u < hi)) continue;
    const int bin = min((int)floor((u - lo) * scale), NB - 1);    // (u just below hi may round up to NB)
    atomicAdd(&lh[bin], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < NB; b += HIST_THREADS) {
    const unsigned c = lh[b];
    if (c) atomicAdd(&hist[b], (unsigned long long)c);
  }
}

__global__ __launch_bounds__(BEAM_THREADS) void beam_scatter_kernel(const float* __restrict__ points,
                                                                    const long* __restrict__ offsets, const BeamTable table,
                                                                    int H, int W, unsigned long long* __restrict__ keys,
                                                                    int* __restrict__ cell_out) {
  __shared__ double beams[BEAM_MAX_H];
  const int s = blockIdx.x, tid = threadIdx.x;
  const long o0 = offsets[s];
  const long n = offsets[s + 1] - o0;
  if ((long)blockIdx.y * BEAM_THREADS >= n) return;
  if (tid < H) beams[tid] = table.b[tid];
  __syncthreads();
  const float4* p = reinterpret_cast<const float4*>(points) + o0;
  unsigned long long* kimg = keys + (long)s * H * W;
  for (long i = (long)blockIdx.y * BEAM_THREADS + tid; i < n; i += (long)BEAM_SPLIT * BEAM_THREADS) {
    const float4 v = p[i];
    int cell = -1;
    double u, d;
    if (beam_point(v, u, d)) {
      // j = the first row whose beam is not above u (the table descends); the nearest beam is row j - 1 or row j
      int a = 0, b = H;
      while (a < b) {
        const int mid = (a + b) >> 1;
        if (beams[mid] > u) a = mid + 1; else b = mid;
      }
      int row = a;
      if (a == H) row = H - 1;
      else if (a > 0 && beams[a - 1] - u <= u - beams[a]) row = a - 1;   // a tie goes to the lower row
      const float colf = sc_column(v.x, v.y, W);
      if (colf >= 0.f && colf < (float)W) {
        cell = row * W + (int)colf;
        atomicMin(&kimg[cell], sc_key((float)d, (unsigned)i));
      }
    }
    if (cell_out) cell_out[o0 + i] = cell;
  }
}

}  // namespace

extern "C" {

int dg_elev_hist(const float* points, const long* offsets, int S, double min_depth, double max_depth, double lo, double hi,
                 int NB, unsigned long long* hist, void* s_) {
  if (!points || !offsets || !hist || S <= 0 || !(lo < hi) || !(hi - lo < __builtin_inf())) return DG_EINVAL;
  if (NB < 64 || NB > 16384) return DG_EINVAL;
  elev_hist_kernel<<<HIST_GRID, HIST_THREADS, (size_t)NB * sizeof(unsigned), (hipStream_t)s_>>>(
      points, offsets, S, min_depth, max_depth, lo, hi, (double)NB / (hi - lo), NB, hist);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_beam_project(const float* points, const long* offsets, int S, const double* beams, int H, int W,
                    unsigned long long* keys, int* cell, float* out, void* s_) {
  if (!points || !offsets || !beams || !keys || !out || S <= 0) return DG_EINVAL;
  if (H < 1 || H > BEAM_MAX_H || W < 1 || W > 8192) return DG_EINVAL;
  BeamTable table;
  for (int h = 0; h < BEAM_MAX_H; ++h) table.b[h] = h < H ? beams[h] : 0.0;
  for (int h = 0; h < H; ++h) {
    if (!(table.b[h] >= -4.0 && table.b[h] <= 4.0)) return DG_EINVAL;        // radians (and not NaN)
    if (h > 0 && !(table.b[h] < table.b[h - 1])) return DG_EINVAL;           // strictly descending
  }
  hipStream_t st = (hipStream_t)s_;
  const long cells = (long)H * W, n = (long)S * cells;
  key_fill_kernel<<<sc_nblk(n), 256, 0, st>>>(keys, n, nullptr, 0);
  beam_scatter_kernel<<<dim3(S, BEAM_SPLIT), BEAM_THREADS, 0, st>>>(points, offsets, table, H, W, keys, cell);
  scan_gather_kernel<<<sc_nblk(n), 256, 0, st>>>(points, offsets, keys, nullptr, cells, n, out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

}  // extern "C"
