// Ray-drop transfer (gfx950; dusty_gan_amd/raydrop.py): the drops G infers for a scan, applied to the points of
// the scan that was inverted - a simulator's complete cloud keeps its own geometry and annotations and loses the returns a
// real sensor would not have measured.  Three small streaming / atomic kernels, nothing of the reference to follow (the paper
// describes the experiment, its repository holds no code for it):
//   * winner : which input point a pixel stands for.  points_to_depth binned every point into a pixel (its `idx`); of the points
//     of one pixel the NEAREST stands for it - a sensor returns the first hit, and a label cannot be averaged - the LOWEST
//     point index on equal ranges (the project's tie rule).  The range is points_body.h's d_u (double arithmetic on the float32
//     coordinates, what the projection's range test saw), rounded once to float32.  One 64-bit atomic per point: the key
//     (range bits << 32 | index) orders like (range, index) - a positive float's bits order like its value - and its COMPLEMENT
//     goes in with an atomic max, so that an all-zero word means "no point" (ZERO AT REST, utils.render._workspace; the
//     complement of a real key is never 0: that would take a NaN range).  A maximum does not depend on the order of its
//     operands: the result is the same for any launch order and under graph replay.  The finish pass unpacks the index (-1
//     for an empty pixel) and zeroes the word.
//   * keep   : keep[b,k,p] = win[b,p] >= 0 && mp && mi, the masks head_px_fwd (head_post.h) forms in eval mode from the raw
//     confidence logits: mp from h1 + noise, mi (dusty2) from the sign of h2.  The noise of realisation k is injected
//     [B,K,HW], or drawn here: philox_logistic4 (step_inputs.h) on counter offset (first_index + b) 2 ceil(HW / 4), stream
//     word (stream id | k << 32) - scan and realisation each own a counter range no batch composition or K moves.
//   * gather : for every (b, k) the records of the kept pixels' winners, bit for bit, in row-major pixel order, with their
//     labels and point indices: dg_export_points' ordered compaction (compact.h: count the chunks, then rank by ballot and
//     place) - two launches, no atomics, the same bytes on every call.
#include "common.h"
#include "compact.h"
#include "head_post.h"
#include "points_body.h"
#include "step_inputs.h"

namespace {

constexpr int RD_THREADS = 256;

// ---- winner -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RD_THREADS) void winner_key_kernel(const float* __restrict__ rec, long rec_sb, int stride,
                                                                const int* __restrict__ counts, const int* __restrict__ idx,
                                                                int N, int HW, unsigned long long* __restrict__ ws) {
  const int b = blockIdx.y;
  const int n = blockIdx.x * RD_THREADS + threadIdx.x;
  const int nb = counts ? min(max(counts[b], 0), N) : N;
  if (n >= nb) return;   // records at and beyond counts[b] are not read
  const int id = idx[(long)b * N + n];
  if (id < 0 || id >= HW) return;   // took no part (anything else out of range is ignored, never an address)
  double x, y, z, r2;
  const float d = (float)pd_range(rec + (long)b * rec_sb + (long)n * stride, x, y, z, r2);
  const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)n;
  atomicMax(ws + (long)b * HW + id, ~key);
}

__global__ __launch_bounds__(RD_THREADS) void winner_finish_kernel(unsigned long long* __restrict__ ws, long total,
                                                                   int* __restrict__ win) {
  const long i = (long)blockIdx.x * RD_THREADS + threadIdx.x;
  if (i >= total) return;
  const unsigned long long w = ws[i];
  ws[i] = 0ull;
  win[i] = w ? (int)(unsigned)(~w & 0xffffffffull) : -1;
}

// ---- keep -------------------------------------------------------------------------------------------------------------------------
// a thread: 4 consecutive pixels (one Philox group) of realisation blockIdx.y of scan blockIdx.z
template <int arch>
__global__ __launch_bounds__(RD_THREADS) void keep_kernel(const float* __restrict__ conf, const int* __restrict__ win,
                                                          const float* __restrict__ noise_in, uint64_t seed, uint64_t stream,
                                                          uint64_t first_index, float eps, float inv_tau, int K, long HW,
                                                          unsigned char* __restrict__ keep, float* __restrict__ noise_out) {
  const long i = (long)blockIdx.x * RD_THREADS + threadIdx.x;
  const long p0 = 4 * i;
  if (p0 >= HW) return;
  const long b = blockIdx.z, k = blockIdx.y;
  const long row = (b * K + k) * HW;
  float nz[4];
  if (noise_in) {
#pragma unroll
    for (int j = 0; j < 4; ++j) nz[j] = p0 + j < HW ? noise_in[row + p0 + j] : 0.f;
  } else {
    const uint64_t n4 = (uint64_t)((HW + 3) / 4);
    philox_logistic4(seed, stream | ((uint64_t)k << 32), (first_index + (uint64_t)b) * 2ull * n4, eps, HW, i, nz);
  }
  const float* h1 = conf + b * arch * HW;
  unsigned char kp[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long p = p0 + j;
    kp[j] = 0;
    if (p >= HW) continue;
    const HeadPx o = head_px_fwd<arch>(0.f, h1[p] + nz[j], arch == 2 ? h1[HW + p] : 0.f, 0.f, 0, inv_tau, 0.f);
    kp[j] = (win[b * HW + p] >= 0 && o.mp > 0.f && o.mi > 0.f) ? 1 : 0;
  }
  if ((HW & 3) == 0) {   // every row starts on a 4-pixel boundary: one store per output
    *(uchar4*)(keep + row + p0) = make_uchar4(kp[0], kp[1], kp[2], kp[3]);
    if (noise_out) *(float4*)(noise_out + row + p0) = make_float4(nz[0], nz[1], nz[2], nz[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (p0 + j < HW) {
        keep[row + p0 + j] = kp[j];
        if (noise_out) noise_out[row + p0 + j] = nz[j];
      }
  }
}

// ---- gather -----------------------------------------------------------------------------------------------------------------------
// the winner of pixel px of scan b if realisation row `kp` keeps it, else -1 (a winner outside [0, N) is never an address)
__device__ __forceinline__ int kept_winner(const unsigned char* __restrict__ kp, const int* __restrict__ wb, long px, long hw, int N) {
  if (px >= hw || !kp[px]) return -1;
  const int w = wb[px];
  return w < N ? w : -1;
}

// launch 1: chunk_counts[(b K + k)][c] = the kept pixels among pixels [c CHUNK, min((c + 1) CHUNK, hw))
__global__ __launch_bounds__(CP_THREADS) void gather_count_kernel(const int* __restrict__ win, const unsigned char* __restrict__ keep,
                                                                  int K, int N, long hw, long nchunk,
                                                                  int* __restrict__ chunk_counts) {
  const long bk = (long)blockIdx.x / nchunk, c = (long)blockIdx.x % nchunk;
  const unsigned char* kp = keep + bk * hw;
  const int* wb = win + (bk / K) * hw;
  cp_count_chunk(c, [&](int, long px) { return kept_winner(kp, wb, px, hw, N) >= 0; }, chunk_counts + blockIdx.x);
}

// launch 2: the records of chunk c of (b, k), placed behind those of the chunks before it
__global__ __launch_bounds__(CP_THREADS) void gather_place_kernel(const unsigned* __restrict__ rec, long rec_sb, int stride, int N,
                                                                  const int* __restrict__ win,
                                                                  const unsigned char* __restrict__ keep,
                                                                  const unsigned* __restrict__ labels, int K, long hw, long nchunk,
                                                                  const int* __restrict__ chunk_counts, uint4* __restrict__ out_rec,
                                                                  unsigned* __restrict__ out_lab, int* __restrict__ out_idx,
                                                                  int* __restrict__ out_counts) {
  const long bk = (long)blockIdx.x / nchunk, c = (long)blockIdx.x % nchunk, b = bk / K;
  const unsigned char* kp = keep + bk * hw;
  const int* wb = win + b * hw;
  int w[CP_ITERS];   // the winner of the thread's k-th pixel (-1: not kept)
  cp_place_chunk(
      chunk_counts + bk * nchunk, c, [&](int k, long px) { return (w[k] = kept_winner(kp, wb, px, hw, N)) >= 0; },
      [&](int k, int pos) {
        const long j = bk * hw + pos;   // pos < the row's count <= hw
        const unsigned* r = rec + b * rec_sb + (long)w[k] * stride;
        out_rec[j] = make_uint4(r[0], r[1], r[2], stride == 4 ? r[3] : 0u);   // the bits as they lie; column 3 = +0.0f for stride 3
        if (out_lab) out_lab[j] = labels[b * N + w[k]];
        out_idx[j] = w[k];
      },
      c == nchunk - 1 ? out_counts + bk : nullptr);
}

}  // namespace

extern "C" {

int dg_pixel_winner(const float* rec, long rec_sb, int stride, const int* counts, const int* idx, int B, int N, int H, int W,
                    unsigned long long* ws, int* win, void* s_) {
  if (!rec || !idx || !ws || !win || B <= 0 || B > 65535 || N <= 0 || H <= 0 || W <= 0) return DG_EINVAL;
  if ((stride != 3 && stride != 4) || rec_sb < (long)N * stride) return DG_EINVAL;
  const long hw = (long)H * W;
  if (hw > 0x7fffffffL) return DG_EINVAL;
  hipStream_t s = (hipStream_t)s_;
  winner_key_kernel<<<dim3((N + RD_THREADS - 1) / RD_THREADS, B), RD_THREADS, 0, s>>>(rec, rec_sb, stride, counts, idx, N, (int)hw,
                                                                                    ws);
  HIP_CHECK_RET(hipGetLastError());
  const long total = (long)B * hw;
  winner_finish_kernel<<<(unsigned)((total + RD_THREADS - 1) / RD_THREADS), RD_THREADS, 0, s>>>(ws, total, win);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_raydrop_keep(const float* conf, int arch, const int* win, const float* noise_in, uint64_t seed, uint64_t stream_id,
                    uint64_t first_index, float eps, float tau, int B, int K, int H, int W, unsigned char* keep, float* noise_out,
                    void* s_) {
  if (!conf || !win || !keep || (arch != 1 && arch != 2) || B <= 0 || B > 65535 || K <= 0 || K > 65535 || H <= 0 || W <= 0)
    return DG_EINVAL;
  if (!(tau > 0.f) || (stream_id >> 32) != 0) return DG_EINVAL;   // (the stream word's high half carries the realisation)
  const long hw = (long)H * W;
  if (hw > 0x7fffffffL) return DG_EINVAL;
  if ((hw & 3) == 0 && ((((uintptr_t)keep) & 3) != 0 || (((uintptr_t)noise_out) & 15) != 0)) return DG_EINVAL;
  const dim3 grid((unsigned)(((hw + 3) / 4 + RD_THREADS - 1) / RD_THREADS), K, B);
  hipStream_t s = (hipStream_t)s_;
  if (arch == 1)
    keep_kernel<1><<<grid, RD_THREADS, 0, s>>>(conf, win, noise_in, seed, stream_id, first_index, eps, 1.f / tau, K, hw, keep,
                                               noise_out);
  else
    keep_kernel<2><<<grid, RD_THREADS, 0, s>>>(conf, win, noise_in, seed, stream_id, first_index, eps, 1.f / tau, K, hw, keep,
                                               noise_out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_raydrop_gather(const float* rec, long rec_sb, int stride, int N, const int* win, const unsigned char* keep,
                      const unsigned* labels, int B, int K, int H, int W, int* chunk_counts, float* out_records,
                      unsigned* out_labels, int* out_index, int* out_counts, void* s_) {
  if (!rec || !win || !keep || !chunk_counts || !out_records || !out_index || !out_counts || B <= 0 || K <= 0 || N <= 0 ||
      H <= 0 || W <= 0)
    return DG_EINVAL;
  if ((stride != 3 && stride != 4) || rec_sb < (long)N * stride || (labels != nullptr) != (out_labels != nullptr)) return DG_EINVAL;
  if (((uintptr_t)out_records & 15) != 0) return DG_EINVAL;   // one 16-byte store per record
  const long hw = (long)H * W, nchunk = (hw + DG_EXPORT_CHUNK - 1) / DG_EXPORT_CHUNK;
  if (hw > 0x7fffffffL || (long)B * K * nchunk > 0x7fffffffL) return DG_EINVAL;   // int32 counts; one workgroup per chunk
  const int grid = (int)((long)B * K * nchunk);
  hipStream_t s = (hipStream_t)s_;
  gather_count_kernel<<<grid, CP_THREADS, 0, s>>>(win, keep, K, N, hw, nchunk, chunk_counts);
  HIP_CHECK_RET(hipGetLastError());
  gather_place_kernel<<<grid, CP_THREADS, 0, s>>>(reinterpret_cast<const unsigned*>(rec), rec_sb, stride, N, win, keep, labels, K,
                                                  hw, nchunk, chunk_counts, reinterpret_cast<uint4*>(out_records), out_labels,
                                                  out_index, out_counts);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

}  // extern "C"
