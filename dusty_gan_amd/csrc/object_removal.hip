// Label-driven object removal (gfx950; dusty_gan_amd/removal.py): the restoration experiment with a mask that
// comes from the scene's semantic labels instead of a random draw.  Nothing of the reference to follow (it holds no such
// command).  Everything here is integer work or bit-for-bit copies:
//   * label_resize  : a label image [B,Hs,Ws] -> [B,H,W] with nearest_src (nearest.h), the rule dg_scan_to_polar resamples the
//     scan itself with: a pixel and its label come from the same cell.  No flip.
//   * remove_mask   : remove[p] = 1 where any pixel q with |dh| <= r, |dw| <= r has valid[q] && table[sem[q]] - a square
//     dilation of the flagged pixels.  Columns wrap (the azimuth is a ring); rows outside the image take no part.  A workgroup
//     owns RM_THREADS consecutive columns of one row: it ORs the flags of rows h - r .. h + r per column into LDS (its columns
//     and r more on either side), then every thread ORs 2 r + 1 LDS bytes.  class_pixels [B,256] counts the VALID pixels of
//     every class before dilation: into 256 u32 words of LDS, then one global integer atomic per non-zero bin (dg_elev_hist's
//     scheme) - integer counts, independent of scheduling.
//   * compose       : per pixel the measured value where the scan is kept, the generated one where an object was removed and G
//     keeps the ray, nothing elsewhere; the values' bits are copied, never recomputed.  Per-scan integer counts: wave ballots,
//     the waves' totals through LDS, one integer atomic per non-zero count per workgroup.
//   * cloud_remove  : the records of a cloud whose pixel is not removed, in input order, bit for bit: compact.h's ordered
//     two-launch compaction over RECORDS instead of pixels.  No atomics: two calls give the same bytes.
#include "common.h"
#include "compact.h"
#include "nearest.h"

namespace {

constexpr int RM_THREADS = 256;
constexpr int RM_MAX_R = 8;

__global__ __launch_bounds__(256) void label_resize_kernel(const unsigned char* __restrict__ in, long n, int Hs, int Ws, int H,
                                                           int W, unsigned char* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int w = (int)(i % W), h = (int)((i / W) % H);
  const long b = i / ((long)W * H);
  out[i] = in[(b * Hs + nearest_src(h, Hs, H)) * Ws + nearest_src(w, Ws, W)];
}

// grid (ceil(W / RM_THREADS), H, B)
__global__ __launch_bounds__(RM_THREADS) void remove_mask_kernel(const unsigned char* __restrict__ sem,
                                                                 const float* __restrict__ valid,
                                                                 const unsigned char* __restrict__ table, int H, int W, int r,
                                                                 unsigned char* __restrict__ remove,
                                                                 unsigned* __restrict__ class_pixels) {
  __shared__ unsigned char col[RM_THREADS + 2 * RM_MAX_R];   // entry j: column w0 - r + j (wrapped), rows h - r .. h + r ORed
  __shared__ unsigned bins[256];
  const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int w0 = blockIdx.x * RM_THREADS;
  const long img = (long)b * H * W;
  bins[tid] = 0u;   // (RM_THREADS == 256)
  const int h_lo = max(h - r, 0), h_hi = min(h + r, H - 1);
  for (int j = tid; j < RM_THREADS + 2 * r; j += RM_THREADS) {
    int w = (w0 - r + j) % W;   // |w0 - r + j| may exceed W on either side when the window is wider than the image
    if (w < 0) w += W;
    unsigned char f = 0;
    for (int hh = h_lo; hh <= h_hi; ++hh) {
      const long q = img + (long)hh * W + w;
      f |= (valid[q] != 0.f && table[sem[q]]) ? 1 : 0;
    }
    col[j] = f;
  }
  __syncthreads();
  const int w = w0 + tid;
  if (w < W) {
    unsigned char f = 0;
    for (int j = 0; j <= 2 * r; ++j) f |= col[tid + j];
    const long p = img + (long)h * W + w;
    remove[p] = f;
    if (valid[p] != 0.f) atomicAdd(&bins[sem[p]], 1u);
  }
  __syncthreads();
  const unsigned c = bins[tid];
  if (c) atomicAdd(&class_pixels[(long)b * 256 + tid], c);
}

// grid (ceil(HW / 256), B); counts [B,3] = removed, filled, in_front
__global__ __launch_bounds__(256) void compose_kernel(const unsigned* __restrict__ tgt_inv, const float* __restrict__ valid,
                                                      const unsigned* __restrict__ gen_inv, const float* __restrict__ keep,
                                                      int keep_is_depth, float tol, const unsigned char* __restrict__ remove,
                                                      const unsigned char* __restrict__ sem, int fill_label, long hw,
                                                      unsigned* __restrict__ inv_out, unsigned char* __restrict__ source,
                                                      unsigned char* __restrict__ sem_out, int* __restrict__ counts) {
  __shared__ int wsum[4][3];
  const int tid = threadIdx.x, b = blockIdx.y;
  const long px = (long)blockIdx.x * 256 + tid;
  bool removed = false, filled = false, front = false;
  if (px < hw) {
    const long p = (long)b * hw + px;
    const bool v = valid[p] != 0.f, rm = remove[p] != 0;
    const float kv = keep[p];
    const bool kp = keep_is_depth ? kv > tol : kv != 0.f;
    const unsigned t = tgt_inv[p], g = gen_inv[p];
    removed = rm && v;
    filled = rm && kp;
    front = filled && v && __uint_as_float(g) > __uint_as_float(t);
    const bool measured = !rm && v;
    inv_out[p] = measured ? t : filled ? g : 0u;
    source[p] = measured ? 1 : filled ? 2 : 0;
    sem_out[p] = measured ? sem[p] : filled ? (unsigned char)fill_label : 0;
  }
  const int c0 = __popcll(__ballot(removed)), c1 = __popcll(__ballot(filled)), c2 = __popcll(__ballot(front));
  if ((tid & 63) == 0) {
    wsum[tid >> 6][0] = c0;
    wsum[tid >> 6][1] = c1;
    wsum[tid >> 6][2] = c2;
  }
  __syncthreads();
  if (tid < 3) {
    const int s = wsum[0][tid] + wsum[1][tid] + wsum[2][tid] + wsum[3][tid];
    if (s) atomicAdd(&counts[b * 3 + tid], s);
  }
}

// is record n of cloud b kept?  (an idx outside [0, hw) took no part in the image: nothing can remove it, and it is never an
// address)
__device__ __forceinline__ bool record_kept(const int* __restrict__ ib, const unsigned char* __restrict__ rb, long n, int nb,
                                            long hw) {
  if (n >= nb) return false;
  const int id = ib[n];
  return id < 0 || id >= hw || rb[id] == 0;
}

__device__ __forceinline__ int cloud_len(const int* __restrict__ counts, long b, int N) {
  return counts ? min(max(counts[b], 0), N) : N;
}

// launch 1: chunk_counts[b][c] = the kept records among records [c CHUNK, min((c + 1) CHUNK, counts[b]))
__global__ __launch_bounds__(CP_THREADS) void cloud_count_kernel(const int* __restrict__ counts, const int* __restrict__ idx,
                                                                 const unsigned char* __restrict__ remove, int N, long hw,
                                                                 long nchunk, int* __restrict__ chunk_counts) {
  const long b = (long)blockIdx.x / nchunk, c = (long)blockIdx.x % nchunk;
  const int nb = cloud_len(counts, b, N);
  const int* ib = idx + b * N;
  const unsigned char* rb = remove + b * hw;
  cp_count_chunk(c, [&](int, long n) { return record_kept(ib, rb, n, nb, hw); }, chunk_counts + blockIdx.x);
}

// launch 2: the kept records of chunk c of cloud b, placed behind those of the chunks before it
__global__ __launch_bounds__(CP_THREADS) void cloud_place_kernel(const unsigned* __restrict__ rec, long rec_sb, int stride,
                                                                 const int* __restrict__ counts, const int* __restrict__ idx,
                                                                 const unsigned char* __restrict__ remove,
                                                                 const unsigned* __restrict__ labels, int N, long hw, long nchunk,
                                                                 const int* __restrict__ chunk_counts, uint4* __restrict__ out_rec,
                                                                 unsigned* __restrict__ out_lab, int* __restrict__ out_idx,
                                                                 int* __restrict__ out_counts) {
  const long b = (long)blockIdx.x / nchunk, c = (long)blockIdx.x % nchunk;
  const int nb = cloud_len(counts, b, N);
  const int* ib = idx + b * N;
  const unsigned char* rb = remove + b * hw;
  cp_place_chunk(
      chunk_counts + b * nchunk, c, [&](int, long n) { return record_kept(ib, rb, n, nb, hw); },
      [&](int k, int pos) {
        const long n = cp_pixel(c, k), j = b * N + pos;   // pos < the cloud's count <= N
        const unsigned* r = rec + b * rec_sb + n * stride;
        out_rec[j] = make_uint4(r[0], r[1], r[2], stride == 4 ? r[3] : 0u);   // the bits as they lie; column 3 = +0.0f for stride 3
        if (out_lab) out_lab[j] = labels[b * N + n];
        out_idx[j] = (int)n;
      },
      c == nchunk - 1 ? out_counts + b : nullptr);
}

}  // namespace

extern "C" {

int dg_label_resize(const unsigned char* sem, int B, int Hs, int Ws, int H, int W, unsigned char* out, void* s_) {
  if (!sem || !out || B <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0) return DG_EINVAL;
  const long n = (long)B * H * W;
  if ((n + 255) / 256 > 0x7fffffffL) return DG_EINVAL;
  label_resize_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)s_>>>(sem, n, Hs, Ws, H, W, out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_remove_mask(const unsigned char* sem, const float* valid, const unsigned char* table, int B, int H, int W, int r,
                   unsigned char* remove, unsigned* class_pixels, void* s_) {
  if (!sem || !valid || !table || !remove || !class_pixels || B <= 0 || B > 65535 || H <= 0 || H > 65535 || W <= 0)
    return DG_EINVAL;
  if (r < 0 || r > RM_MAX_R || (long)H * W > 0x7fffffffL) return DG_EINVAL;
  remove_mask_kernel<<<dim3((W + RM_THREADS - 1) / RM_THREADS, H, B), RM_THREADS, 0, (hipStream_t)s_>>>(
      sem, valid, table, H, W, r, remove, class_pixels);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_compose_removed(const float* tgt_inv, const float* valid, const float* gen_inv, const float* keep, int keep_is_depth,
                       float tol, const unsigned char* remove, const unsigned char* sem, int fill_label, int B, int H, int W,
                       float* inv_out, unsigned char* source, unsigned char* sem_out, int* counts, void* s_) {
  if (!tgt_inv || !valid || !gen_inv || !keep || !remove || !sem || !inv_out || !source || !sem_out || !counts) return DG_EINVAL;
  if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || fill_label < 0 || fill_label > 255) return DG_EINVAL;
  const long hw = (long)H * W;
  if (hw > 0x7fffffffL) return DG_EINVAL;
  compose_kernel<<<dim3((unsigned)((hw + 255) / 256), B), 256, 0, (hipStream_t)s_>>>(
      reinterpret_cast<const unsigned*>(tgt_inv), valid, reinterpret_cast<const unsigned*>(gen_inv), keep, keep_is_depth, tol,
      remove, sem, fill_label, hw, reinterpret_cast<unsigned*>(inv_out), source, sem_out, counts);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_cloud_remove(const float* rec, long rec_sb, int stride, const int* counts, const int* idx, const unsigned char* remove,
                    const unsigned* labels, int B, int N, int H, int W, int* chunk_counts, float* out_records,
                    unsigned* out_labels, int* out_index, int* out_counts, void* s_) {
  if (!rec || !idx || !remove || !chunk_counts || !out_records || !out_index || !out_counts || B <= 0 || N <= 0 || H <= 0 ||
      W <= 0)
    return DG_EINVAL;
  if ((stride != 3 && stride != 4) || rec_sb < (long)N * stride || (labels != nullptr) != (out_labels != nullptr)) return DG_EINVAL;
  if (((uintptr_t)out_records & 15) != 0) return DG_EINVAL;   // one 16-byte store per record
  const long hw = (long)H * W, nchunk = ((long)N + DG_EXPORT_CHUNK - 1) / DG_EXPORT_CHUNK;
  if (hw > 0x7fffffffL || (long)B * nchunk > 0x7fffffffL) return DG_EINVAL;   // int32 counts; one workgroup per chunk
  const int grid = (int)((long)B * nchunk);
  hipStream_t s = (hipStream_t)s_;
  cloud_count_kernel<<<grid, CP_THREADS, 0, s>>>(counts, idx, remove, N, hw, nchunk, chunk_counts);
  HIP_CHECK_RET(hipGetLastError());
  cloud_place_kernel<<<grid, CP_THREADS, 0, s>>>(reinterpret_cast<const unsigned*>(rec), rec_sb, stride, counts, idx, remove,
                                                 labels, N, hw, nchunk, chunk_counts, reinterpret_cast<uint4*>(out_records),
                                                 out_labels, out_index, out_counts);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

}  // extern "C"
