// Validation metrics that are not point-set distances, gfx950:
//   * grid_vote_kernel, jsd_kernel        : the JSD occupancy histogram and the divergence (utils/metrics/jsd.py).
//   * pyr_down_kernel, pyr_up_sub_kernel,
//     patches_kernel                      : the SWD descriptors' Laplacian pyramid and patch gathering (utils/metrics/swd.py).
// The point-set kernels live in one file per family: point_fps.hip, point_chamfer.hip, point_emd.hip.
#include "common.h"

namespace {

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

}  // namespace

extern "C" {

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

}  // extern "C"
