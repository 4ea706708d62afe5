// Raw Velodyne scans -> the dataset's files (gfx950): what the reference's process_kitti.py does on CPU workers, as streaming
// kernels.
//   * scan_project : S raw scans (concatenated [N,4] points + [S+1] offsets) -> [S,64,W,4] spherical projections
//     (process_point_clouds, process_kitti.py:76-118).  Three launches: key fill, rows + z-buffer, gather.
//       row    a point starts a ring when its cyclic predecessor lies in quadrant 3 and the point itself in quadrant 0 (:90-98);
//              with L starts and c(i) = the inclusive count of starts up to i, row = 0 if c = 0 else 64 - L + c - 1 (:101-106).
//              c is a segmented prefix count of 1-bit flags: wave ballot + popcount, the waves' totals through LDS, a running
//              carry per workgroup.  SCAN_SPLIT workgroups share a scan; each counts the whole scan's flags itself (8 bytes
//              of every point, out of L2 after the first reader), so no workgroup waits for another.
//       L > 64 rows in [-64,-1] wrap to row + 64 (numpy's negative index in `scatter`, :62-63); a row below -64 makes numpy
//              raise: status[s] = 1 and the scan's points are not scattered (its output is all zeros).
//       column floor(((-atan2(y, x) / pi + 1) / 2 mod 1) * W), every step in float32 (:109-111)
//       cell   the reference sorts far-to-near and lets later writes win (:85-86, :60-73): each cell keeps its NEAREST point.
//              Here: a 64-bit atomicMin of (depth bits << 32 | point index) - non-negative floats order like their bits.  No
//              sort, nothing depends on scheduling.  TIE RULE: of two points of one cell with the same float32 depth the LOWER
//              point index wins (the reference's argsort leaves ties undefined).
//   * angle_accum / angle_finish : the per-pixel mean elevation / azimuth of a dataset (compute_avg_angles, :143-183) over
//     projected scans at their own size.  One thread per pixel walks the scans of a chunk in order and adds pitch, yaw (32.32
//     fixed point, common.h) and the valid count: integer sums, so the grid depends neither on the chunk size nor on scheduling.
// All HBM-bound: 16 bytes per point in, 8 bytes of key + 16 bytes out per cell.
#include "common.h"
#include "scan_cell.h"   // the column, the z-buffer key, key fill and gather: shared with beam_project.hip

namespace {

#define SCAN_THREADS 1024
#define SCAN_SPLIT 8      // workgroups per scan
#define PROJ_H 64         // the reference hard-codes line_idx = 63

// quadrant as process_kitti.py:90-94 (a NaN coordinate matches no line there: 0)
__device__ __forceinline__ int quadrant(float x, float y) {
  if (x < 0.f && y >= 0.f) return 1;
  if (x < 0.f && y < 0.f) return 2;
  if (x >= 0.f && y < 0.f) return 3;
  return 0;
}

// does point i of the scan [p, p + n) start a ring?
__device__ __forceinline__ int ring_start(const float4* __restrict__ p, int n, int i) {
  const float2 a = *reinterpret_cast<const float2*>(p + i);
  const float2 b = *reinterpret_cast<const float2*>(p + (i == 0 ? n - 1 : i - 1));
  return quadrant(b.x, b.y) == 3 && quadrant(a.x, a.y) == 0;
}

// block-wide sum of one int per thread (SCAN_THREADS threads); every thread gets the total.  red: 16 ints of LDS
__device__ __forceinline__ int block_count(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < SCAN_THREADS / 64; ++w) t += red[w];
  return t;
}

__global__ __launch_bounds__(SCAN_THREADS) void scan_scatter_kernel(const float* __restrict__ points,
                                                                    const long* __restrict__ offsets, int W,
                                                                    unsigned long long* __restrict__ keys,
                                                                    int* __restrict__ status, int* __restrict__ cell_out) {
#pragma clang fp contract(off)  // plain IEEE operators (as scan_to_polar_kernel): numpy's float32 arithmetic, step for step
  __shared__ int red[SCAN_THREADS / 64];
  const int s = blockIdx.x, part = blockIdx.y, tid = threadIdx.x;
  const long o0 = offsets[s];
  const int n = (int)(offsets[s + 1] - o0);
  if (n <= 0) return;
  const float4* p = reinterpret_cast<const float4*>(points) + o0;
  // this workgroup's slice [lo, hi) of the scan, in whole tiles of SCAN_THREADS points
  const int tiles = (n + SCAN_THREADS - 1) / SCAN_THREADS, per = (tiles + SCAN_SPLIT - 1) / SCAN_SPLIT;
  const int lo = min(n, part * per * SCAN_THREADS), hi = min(n, (part + 1) * per * SCAN_THREADS);
  if (lo >= hi) return;
  // L = the scan's ring starts; carry = those before the slice
  int before = 0, all = 0;
  for (int i = tid; i < n; i += SCAN_THREADS) {
    const int f = ring_start(p, n, i);
    all += f;
    before += i < lo ? f : 0;
  }
  const int L = block_count(all, red);
  int carry = block_count(before, red);
  unsigned long long* kimg = keys + (long)s * PROJ_H * W;
  const int lane = tid & 63, wave = tid >> 6;
  for (int base = lo; base < hi; base += SCAN_THREADS) {
    const int i = base + tid;
    const bool live = i < hi;
    const int f = live ? ring_start(p, n, i) : 0;
    const unsigned long long bal = __ballot(f);
    const int incl = __popcll(bal & (~0ull >> (63 - lane)));   // starts of this wave up to and including this lane
    __syncthreads();                                           // (red is free: the previous tile's readers are done)
    if (lane == 0) red[wave] = __popcll(bal);
    __syncthreads();
    int woff = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SCAN_THREADS / 64; ++w) {
      const int c = red[w];
      woff += w < wave ? c : 0;
      total += c;
    }
    const int c = carry + woff + incl;
    carry += total;
    if (!live) continue;
    int row = c == 0 ? 0 : PROJ_H - L + c - 1;
    int cell = -1;
    if (row < -PROJ_H) {
      status[s] = 1;              // every writer stores the same word
    } else {
      if (row < 0) row += PROJ_H;
      const float4 v = p[i];
      const float colf = sc_column(v.x, v.y, W);
      const float depth = sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);   // np.linalg.norm(xyz, ord=2, axis=1) in float32
      // (a non-finite coordinate has no column, and the reference's scatter would index out of range: the point is dropped)
      if (colf >= 0.f && colf < (float)W && depth >= 0.f) {
        cell = row * W + (int)colf;
        atomicMin(&kimg[cell], sc_key(depth, (unsigned)i));
      }
    }
    if (cell_out) cell_out[o0 + i] = cell;
  }
}

// compute_avg_angles' loop body (process_kitti.py:150-166) on KITTIOdometry.preprocess's unit-space xyz (datasets/kitti.py:54-67,
// the arithmetic of scan_to_polar_kernel), one thread per pixel, the scans of the chunk in order
__global__ __launch_bounds__(256) void angle_accum_kernel(const float* __restrict__ scans, int S, long HW, int C, float min_d,
                                                          float max_d, long long* __restrict__ sums, int* __restrict__ count) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= HW) return;
  long long sp = sums[i], sy = sums[HW + i];
  int cnt = count[i];
  for (int s = 0; s < S; ++s) {
    const float* cell = scans + ((long)s * HW + i) * C;
    float x, y, z;
    if (C == 4) {
      const float4 v = *reinterpret_cast<const float4*>(cell);
      x = v.x; y = v.y; z = v.z;
    } else {
      x = cell[0]; y = cell[1]; z = cell[2];
    }
    const float d = sqrtf((x * x + y * y) + z * z);
    const bool in_range = d > 0.f && d > min_d && d < max_d;
    x = in_range ? x / max_d : 0.f;
    y = in_range ? y / max_d : 0.f;
    z = in_range ? z / max_d : 0.f;
    const float depth = sqrtf((x * x + y * y) + z * z) * max_d;
    if (!(depth > 1e-8f)) continue;      // valid = 0: the pixel adds nothing
    const float r = sqrtf(x * x + y * y);
    const float pitch = atan2f(z, r), yaw = atan2f(y, x);
    long long qp = 0, qy = 0;
    dg_fix1(pitch, qp);                  // |angle| <= pi: always inside the codec's window
    dg_fix1(yaw, qy);
    sp += qp;
    sy += qy;
    cnt += 1;
  }
  sums[i] = sp;
  sums[HW + i] = sy;
  count[i] = cnt;
}

// sums / counts, then the never-valid pixels: pitch <- the mean of its ROW's valid pixels, yaw <- the mean of its COLUMN's
// (mean() over the non-NaN entries, process_kitti.py:134-140, :172-179).  Blocks [0, H): one row each; the rest: 256 columns each.
// A row / column without any valid pixel leaves NaN, where the reference's assert fires (:181).
__global__ __launch_bounds__(256) void angle_finish_kernel(const long long* __restrict__ sums, const int* __restrict__ count,
                                                           int H, int W, float* __restrict__ angles) {
  __shared__ double s_sum[256];
  __shared__ int s_cnt[256];
  const long HW = (long)H * W;
  const double unit = 1.0 / 4294967296.0;
  if ((int)blockIdx.x < H) {
    const int h = blockIdx.x;
    double acc = 0.0;
    int nv = 0;
    for (int w = threadIdx.x; w < W; w += 256) {
      const long px = (long)h * W + w;
      const int c = count[px];
      if (c > 0) {
        const float a = (float)((double)sums[px] * unit / (double)c);
        angles[px] = a;
        acc += (double)a;
        nv += 1;
      }
    }
    s_sum[threadIdx.x] = acc;
    s_cnt[threadIdx.x] = nv;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {   // fixed tree: the same bits every run
      if ((int)threadIdx.x < o) {
        s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
        s_cnt[threadIdx.x] += s_cnt[threadIdx.x + o];
      }
      __syncthreads();
    }
    const float fill = s_cnt[0] > 0 ? (float)(s_sum[0] / (double)s_cnt[0]) : __builtin_nanf("");
    for (int w = threadIdx.x; w < W; w += 256) {
      const long px = (long)h * W + w;
      if (count[px] <= 0) angles[px] = fill;
    }
    return;
  }
  const int w = ((int)blockIdx.x - H) * 256 + threadIdx.x;
  if (w >= W) return;
  double acc = 0.0;
  int nv = 0;
  for (int h = 0; h < H; ++h) {
    const long px = (long)h * W + w;
    const int c = count[px];
    if (c > 0) {
      const float a = (float)((double)sums[HW + px] * unit / (double)c);
      angles[HW + px] = a;
      acc += (double)a;
      nv += 1;
    }
  }
  const float fill = nv > 0 ? (float)(acc / (double)nv) : __builtin_nanf("");
  for (int h = 0; h < H; ++h) {
    const long px = (long)h * W + w;
    if (count[px] <= 0) angles[HW + px] = fill;
  }
}

}  // namespace

extern "C" {

int dg_scan_project(const float* points, const long* offsets, int S, int H, int W, unsigned long long* keys, int* status,
                    int* cell, float* out, void* s_) {
  if (!points || !offsets || !keys || !status || !out || S <= 0 || H <= 0 || W <= 0) return DG_EINVAL;
  if (H != PROJ_H) return DG_EUNSUPPORTED;
  if ((long)H * W > 0x7FFFFFFFl) return DG_EINVAL;
  hipStream_t st = (hipStream_t)s_;
  const long cells = (long)H * W, n = (long)S * cells;
  key_fill_kernel<<<sc_nblk(n), 256, 0, st>>>(keys, n, status, S);
  scan_scatter_kernel<<<dim3(S, SCAN_SPLIT), SCAN_THREADS, 0, st>>>(points, offsets, W, keys, status, cell);
  scan_gather_kernel<<<sc_nblk(n), 256, 0, st>>>(points, offsets, keys, status, cells, n, out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_angle_accum(const float* scans, int S, int H, int W, int C, double min_depth, double max_depth, long long* sums,
                   int* count, void* s_) {
  if (!scans || !sums || !count || S <= 0 || H <= 0 || W <= 0 || C < 3 || !(max_depth > min_depth)) return DG_EINVAL;
  const long hw = (long)H * W;
  angle_accum_kernel<<<sc_nblk(hw), 256, 0, (hipStream_t)s_>>>(scans, S, hw, C, (float)min_depth, (float)max_depth, sums, count);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_angle_finish(const long long* sums, const int* count, int H, int W, float* angles, void* s_) {
  if (!sums || !count || !angles || H <= 0 || W <= 0) return DG_EINVAL;
  angle_finish_kernel<<<H + (W + 255) / 256, 256, 0, (hipStream_t)s_>>>(sums, count, H, W, angles);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

}  // extern "C"
