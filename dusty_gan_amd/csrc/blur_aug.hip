// The image end of the discriminator: BlurVH (forward, adjoint, R1's turn-around), DiffAugment (diffaug.h: forward, forward
// fused with BlurVH, adjoint) and the per-sample sums between them.  Images are fp32 [B,1,H,W]; feature maps are T.
#include "pointwise.h"
#include "diffaug.h"

// ----------------------------------------------------------------------------------------------------------
// BlurVH (models/ops/common.py:74-88): x [B,H,W] fp32 -> h0 [B,H,W,2] (ch0 = vertical [1,2,1]/4 with reflect rows,
// ch1 = horizontal [1,2,1]/4 with circular / reflect columns).
template <typename T>
__global__ void blur_fwd_kernel(const float* __restrict__ x, T* __restrict__ out, int B, int H, int W, int ring) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)B * H * W;
  if (idx >= total) return;
  const int xx = (int)(idx % W), y = (int)((idx / W) % H);
  const long base = idx - (long)y * W - xx;  // b*H*W
  const int yu = y == 0 ? 1 : y - 1, yd = y == H - 1 ? H - 2 : y + 1;
  int xl = xx - 1, xr = xx + 1;
  if (ring) { if (xl < 0) xl += W; if (xr >= W) xr -= W; }
  else      { if (xl < 0) xl = 1;  if (xr >= W) xr = W - 2; }
  const float c = x[idx];
  const float v = 0.25f * x[base + (long)yu * W + xx] + 0.5f * c + 0.25f * x[base + (long)yd * W + xx];
  const float h = 0.25f * x[base + (long)y * W + xl] + 0.5f * c + 0.25f * x[base + (long)y * W + xr];
  out[idx * 2 + 0] = (T)v;
  out[idx * 2 + 1] = (T)h;
}

// Adjoint of BlurVH: d [B,H,W,2] -> dx [B,H,W] fp32.
template <typename T>
__global__ void blur_bwd_kernel(const T* __restrict__ d, float* __restrict__ dx, int B, int H, int W, int ring) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)B * H * W;
  if (idx >= total) return;
  const int xx = (int)(idx % W), y = (int)((idx / W) % H);
  const long base = idx - (long)y * W - xx;
  auto D0 = [&](int yy, int xq) { return (float)d[(base + (long)yy * W + xq) * 2 + 0]; };
  auto D1 = [&](int yy, int xq) { return (float)d[(base + (long)yy * W + xq) * 2 + 1]; };
  float v = 0.5f * D0(y, xx);
  if (y > 0) v += 0.25f * D0(y - 1, xx);
  if (y < H - 1) v += 0.25f * D0(y + 1, xx);
  if (y == 1) v += 0.25f * D0(0, xx);          // row 0 read x[1] as its reflected upper neighbour
  if (y == H - 2) v += 0.25f * D0(H - 1, xx);  // row H-1 read x[H-2] as its reflected lower neighbour
  float h = 0.5f * D1(y, xx);
  if (ring) {
    h += 0.25f * D1(y, xx == 0 ? W - 1 : xx - 1) + 0.25f * D1(y, xx == W - 1 ? 0 : xx + 1);
  } else {
    if (xx > 0) h += 0.25f * D1(y, xx - 1);
    if (xx < W - 1) h += 0.25f * D1(y, xx + 1);
    if (xx == 1) h += 0.25f * D1(y, 0);
    if (xx == W - 2) h += 0.25f * D1(y, W - 1);
  }
  dx[idx] = v + h;
}

// Four pixels per thread (W % 4 == 0): 16-byte loads of the three rows, one 16-byte (bf16) / two (fp32) stores; the same
// expressions as the scalar kernels above, which remain for other widths.
// Grid = (row, sample): the row's neighbours and boundary cases are block-uniform and the per-quad work is 32-bit (the
// first version decoded a flat 64-bit quad index per thread and, in the adjoint, loaded each neighbour row under its own
// condition - one global round trip after the other).
template <typename T>
__global__ __launch_bounds__(256) void blur_fwd4_kernel(const float* __restrict__ x, T* __restrict__ out, int B, int H,
                                                        int W, int ring, const float* __restrict__ mean_src, int mean_n,
                                                        float* __restrict__ mean_acc) {
  if (mean_src && blockIdx.x == 0 && blockIdx.y == 0) {          // rider of block (0, 0): mean_acc[0] += mean(mean_src[0..n))
    __shared__ float red[16];                                    // (dg_mean_acc: the R1 penalty of the micro-batch)
    float sm = 0.f;
    for (int i = threadIdx.x; i < mean_n; i += 256) sm += mean_src[i];
    const float t = dg_block_sum(sm, red);
    if (threadIdx.x == 0) mean_acc[0] += t / mean_n;
  }
  const int y = blockIdx.x, W4 = W >> 2;
  const long base = (long)blockIdx.y * H * W;                    // b*H*W
  const int yu = y == 0 ? 1 : y - 1, yd = y == H - 1 ? H - 2 : y + 1;
  const float* rc = x + base + (long)y * W;
  const float* ru = x + base + (long)yu * W;
  const float* rd = x + base + (long)yd * W;
  for (int q4 = threadIdx.x; q4 < W4; q4 += 256) {
    const int x0 = q4 * 4;
    const float4 c4 = *(const float4*)(rc + x0);
    const float4 u4 = *(const float4*)(ru + x0);
    const float4 d4 = *(const float4*)(rd + x0);
    int xl = x0 - 1, xr = x0 + 4;
    if (ring) { if (xl < 0) xl += W; if (xr >= W) xr -= W; }
    else      { if (xl < 0) xl = 1;  if (xr >= W) xr = W - 2; }
    const float c[6] = {rc[xl], c4.x, c4.y, c4.z, c4.w, rc[xr]};
    const float u[4] = {u4.x, u4.y, u4.z, u4.w}, d[4] = {d4.x, d4.y, d4.z, d4.w};
    float o[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      o[2 * k] = 0.25f * u[k] + 0.5f * c[k + 1] + 0.25f * d[k];
      o[2 * k + 1] = 0.25f * c[k] + 0.5f * c[k + 1] + 0.25f * c[k + 2];
    }
    T* op = out + (base + (long)y * W + x0) * 2;
    if constexpr (sizeof(T) == 2) {
      Vec16<bf16>::store((bf16*)op, o);
    } else {
      *(float4*)op = make_float4(o[0], o[1], o[2], o[3]);
      *(float4*)(op + 4) = make_float4(o[4], o[5], o[6], o[7]);
    }
  }
}

// BlurVH's adjoint for NR consecutive rows ys .. ys + NR - 1 of one pixel quad (columns x0 .. x0 + 3): the NR + 2 source rows
// and the 2 NR ring neighbours of a thread are loaded TOGETHER, unconditionally (rows clamped into the image; what a clamped
// row contributes is never used) - row after row, each row's loads waited for before the next row's were issued: four to six
// dependent memory round trips per workgroup (round 6: blur_bwd4_kernel 8.9 us, 6.8 without its sums).  Same expressions in
// the same order as blur_bwd_kernel's: bit-identical results.  Rows outside [0, H) come back as garbage the caller skips.
template <typename T, int NR>
__device__ __forceinline__ void blur_adj_rows(const T* __restrict__ d, long base, int ys, int x0, int H, int W, int ring,
                                              float (&g)[NR][4]) {
  float rows[NR + 2][8];
  float el[NR], er[NR];
  auto clampy = [&](int yy) { return yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy); };
#pragma unroll
  for (int r = 0; r < NR + 2; ++r) {
    const T* p = d + (base + (long)clampy(ys - 1 + r) * W + x0) * 2;
    if constexpr (sizeof(T) == 2) {
      Vec16<bf16>::load((const bf16*)p, rows[r]);
    } else {
      const float4 a = *(const float4*)p, b2 = *(const float4*)(p + 4);
      rows[r][0] = a.x; rows[r][1] = a.y; rows[r][2] = a.z; rows[r][3] = a.w;
      rows[r][4] = b2.x; rows[r][5] = b2.y; rows[r][6] = b2.z; rows[r][7] = b2.w;
    }
  }
  // channel 1 of the pixels left and right of the quad (circular columns: wrapped; reflect columns: clamped - then unused
  // at the border): two 2- or 4-byte loads per row, unconditional like the rows'
  const int xl = ring ? (x0 == 0 ? W - 1 : x0 - 1) : (x0 == 0 ? 0 : x0 - 1);
  const int xr = ring ? (x0 + 3 == W - 1 ? 0 : x0 + 4) : (x0 + 4 > W - 1 ? W - 1 : x0 + 4);
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const long rowb = base + (long)clampy(ys + j) * W;
    el[j] = (float)d[(rowb + xl) * 2 + 1];
    er[j] = (float)d[(rowb + xr) * 2 + 1];
  }
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int y = ys + j;
    const float (&m)[8] = rows[j + 1];
    const float (&tu)[8] = rows[j];
    const float (&td)[8] = rows[j + 2];
    float v[4], h[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = 0.5f * m[2 * k];
    if (y > 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] += 0.25f * tu[2 * k]; }
    if (y < H - 1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] += 0.25f * td[2 * k]; }
    if (y == 1) {                                  // row 0 read x[1] as its reflected upper neighbour (row 0 IS tu here)
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] += 0.25f * tu[2 * k]; }
    if (y == H - 2) {                              // row H-1 read x[H-2] as its reflected lower neighbour (row H-1 IS td here)
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] += 0.25f * td[2 * k]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int xx = x0 + k;
      h[k] = 0.5f * m[2 * k + 1];
      const bool hasl = k > 0, hasr = k < 3;
      if (ring) {
        h[k] += 0.25f * (hasl ? m[2 * k - 1] : el[j]) + 0.25f * (hasr ? m[2 * k + 3] : er[j]);
      } else {
        if (xx > 0) h[k] += 0.25f * (hasl ? m[2 * k - 1] : el[j]);
        if (xx < W - 1) h[k] += 0.25f * (hasr ? m[2 * k + 3] : er[j]);
        if (xx == 1) h[k] += 0.25f * m[1];         // column 0 read x[1] as its reflected left neighbour (pixel 0 = this quad's first)
        if (xx == W - 2) h[k] += 0.25f * m[7];     // column W-1 read x[W-2] (pixel W-1 = this quad's last)
      }
      g[j][k] = v[k] + h[k];
    }
  }
}

// One block owns a band of NR consecutive rows of one sample (H % NR == 0; the launchers choose NR): blur_adj_rows forms the band,
// then one store and one sum per row.  ssq == nullptr: dx = oscale * g only.  ssq != nullptr && !use_win (R1): ssq[b] += sum of
// g^2 over the sample, g = the adjoint's result - the R1 penalty's per-sample |g|^2 and its tangent v = (gp / B) g in the pass
// that makes g.  use_win: ssq[b] += sum of g over the window of `win` instead (diffaug.h aug_in_window: the contrast term of
// DiffAugment's adjoint; win carries t_h, o_x, o_y only) - the pass that makes g also makes the sum its adjoint needs.
// One accumulator add per block: gridDim.x contributors per slot.
template <typename T, int NR>
__global__ __launch_bounds__(256) void blur_bwd4_kernel(const T* __restrict__ d, float* __restrict__ dx, int H, int W, int ring,
                                                        float oscale, float* __restrict__ ssq, AugP win, int use_win,
                                                        const DgDet det) {
  __shared__ float red[16];
  const int W4 = W >> 2, b = blockIdx.y;
  const long base = (long)b * H * W;
  const int y0 = blockIdx.x * NR;
  const AugSample ws = aug_window(win, b);        // (policy 0 without a window: nothing is read)
  float ssacc = 0.f;
  for (int q4 = threadIdx.x; q4 < W4; q4 += 256) {
    const int x0 = q4 * 4;
    float g[NR][4];
    blur_adj_rows<T, NR>(d, base, y0, x0, H, W, ring, g);
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int y = y0 + j;
      const float g0 = g[j][0], g1 = g[j][1], g2 = g[j][2], g3 = g[j][3];
      *(float4*)(dx + base + (long)y * W + x0) = make_float4(oscale * g0, oscale * g1, oscale * g2, oscale * g3);
      if (!use_win) {
        ssacc += g0 * g0 + g1 * g1 + g2 * g2 + g3 * g3;
      } else {
        const AugRow wr = aug_row<false>(win, ws, y);
        const float gq[4] = {g0, g1, g2, g3};
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (aug_in_window(wr, x0 + k)) ssacc += gq[k];
      }
    }
  }
  if (ssq) {
    const float sblk = dg_block_sum(ssacc, red);
    if (threadIdx.x == 0) dg_acc_add(&ssq[b], sblk, gridDim.x, det);
  }
}
// rows per block = per accumulator add on ssq[b]
template <typename T>
static void blur_bwd4_launch(const void* d, float* dx, int B, int H, int W, int ring, float oscale, float* ssq, int rows_pb,
                             const AugP& win, int use_win, hipStream_t s) {
  const dim3 grid(H / rows_pb, B);
  const DgDet det = dg_det_current();
  if (rows_pb == 4) blur_bwd4_kernel<T, 4><<<grid, 256, 0, s>>>((const T*)d, dx, H, W, ring, oscale, ssq, win, use_win, det);
  else if (rows_pb == 2) blur_bwd4_kernel<T, 2><<<grid, 256, 0, s>>>((const T*)d, dx, H, W, ring, oscale, ssq, win, use_win, det);
  else blur_bwd4_kernel<T, 1><<<grid, 256, 0, s>>>((const T*)d, dx, H, W, ring, oscale, ssq, win, use_win, det);
}
static void blur_bwd4_launch(const void* d, int dtype, float* dx, int B, int H, int W, int ring, float oscale, float* ssq,
                             int rows_pb, const AugP& win, int use_win, hipStream_t s) {
  if (dtype == DG_BF16) blur_bwd4_launch<bf16>(d, dx, B, H, W, ring, oscale, ssq, rows_pb, win, use_win, s);
  else blur_bwd4_launch<float>(d, dx, B, H, W, ring, oscale, ssq, rows_pb, win, use_win, s);
}
static int blur_rows_pb(int H) { return H % 4 == 0 ? 4 : (H % 2 == 0 ? 2 : 1); }

// ----------------------------------------------------------------------------------------------------------
// R1's turn-around at the image in ONE launch (round 6; trainers/dcgan_amp.py:218-235): g = BlurVH^T(e0) is the gradient of
// sum(y_real) w.r.t. the augmented real image, the penalty reads |g_b|^2, and the double backward's tangent v = oscale g goes
// straight back up through BlurVH (models/ops/common.py:74-88) - so g never needs to exist in memory: a block owns a band
// of R1T_ROWS rows of one sample, forms oscale g for the band and one halo row on either side in LDS (the same expressions,
// in the same order, as blur_bwd4_kernel), then BlurVH of those rows (blur_fwd4_kernel's expressions) into the tangent
// slot of h0.  ssq[b] += |g_b|^2 over the band's own rows; mean_acc[0] += the same / mean_n (the logged penalty: its mean
// over the batch is the sum of all blocks' shares - no second pass over ssq).  W % 4 == 0, H % R1T_ROWS == 0.
#define R1T_ROWS 4
template <typename T>
__global__ __launch_bounds__(256) void blur_r1_tangent_kernel(const T* __restrict__ d, T* __restrict__ out, int H, int W,
                                                              int ring, float oscale, float* __restrict__ ssq,
                                                              float* __restrict__ mean_acc, int mean_n, const DgDet det) {
  extern __shared__ float s_g[];                  // [R1T_ROWS + 2][W]: oscale * g of rows y0 - 1 .. y0 + R1T_ROWS
  __shared__ float red[16];
  const int W4 = W >> 2, b = blockIdx.y;
  const long base = (long)b * H * W;
  const int y0 = blockIdx.x * R1T_ROWS;
  float ssacc = 0.f;
  for (int q4 = threadIdx.x; q4 < W4; q4 += 256) {
    const int x0 = q4 * 4;
    float g[R1T_ROWS + 2][4];
    blur_adj_rows<T, R1T_ROWS + 2>(d, base, y0 - 1, x0, H, W, ring, g);   // rows y0 - 1 .. y0 + R1T_ROWS, their loads batched
#pragma unroll
    for (int r = 0; r < R1T_ROWS + 2; ++r) {
      const int y = y0 - 1 + r;
      if (y < 0 || y >= H) continue;              // (block-uniform: the rows beyond the image are never read below)
      const float g0 = g[r][0], g1 = g[r][1], g2 = g[r][2], g3 = g[r][3];
      *(float4*)(s_g + r * W + x0) = make_float4(oscale * g0, oscale * g1, oscale * g2, oscale * g3);
      if (r >= 1 && r <= R1T_ROWS) ssacc += g0 * g0 + g1 * g1 + g2 * g2 + g3 * g3;
    }
  }
  __syncthreads();
  for (int yy = 0; yy < R1T_ROWS; ++yy) {
    const int y = y0 + yy;
    const int yu = y == 0 ? 1 : y - 1, yd = y == H - 1 ? H - 2 : y + 1;
    const float* rc = s_g + (y - y0 + 1) * W;
    const float* ru = s_g + (yu - y0 + 1) * W;
    const float* rd = s_g + (yd - y0 + 1) * W;
    for (int q4 = threadIdx.x; q4 < W4; q4 += 256) {
      const int x0 = q4 * 4;
      const float4 c4 = *(const float4*)(rc + x0);
      const float4 u4 = *(const float4*)(ru + x0);
      const float4 d4 = *(const float4*)(rd + x0);
      int xl = x0 - 1, xr = x0 + 4;
      if (ring) { if (xl < 0) xl += W; if (xr >= W) xr -= W; }
      else      { if (xl < 0) xl = 1;  if (xr >= W) xr = W - 2; }
      const float c[6] = {rc[xl], c4.x, c4.y, c4.z, c4.w, rc[xr]};
      const float u[4] = {u4.x, u4.y, u4.z, u4.w}, dn[4] = {d4.x, d4.y, d4.z, d4.w};
      float o[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        o[2 * k] = 0.25f * u[k] + 0.5f * c[k + 1] + 0.25f * dn[k];
        o[2 * k + 1] = 0.25f * c[k] + 0.5f * c[k + 1] + 0.25f * c[k + 2];
      }
      T* op = out + (base + (long)y * W + x0) * 2;
      if constexpr (sizeof(T) == 2) {
        Vec16<bf16>::store((bf16*)op, o);
      } else {
        *(float4*)op = make_float4(o[0], o[1], o[2], o[3]);
        *(float4*)(op + 4) = make_float4(o[4], o[5], o[6], o[7]);
      }
    }
  }
  const float sblk = dg_block_sum(ssacc, red);
  if (threadIdx.x == 0) {
    // the sample's last band adds the sample's total to the batch mean: gridDim.y adds to that word, not gridDim.x gridDim.y
    // (512 adds to ONE word serialise memory-side: 9 us of this launch, scripts/bench_pointwise.py)
    float tot = 0.f;
    const int last = dg_acc_add_last(&ssq[b], sblk, gridDim.x, det, tot);
    if (mean_acc) {
      if (last == 1) dg_acc_add(mean_acc, tot / (float)mean_n, gridDim.y, det);
      else if (last < 0) atomicAdd(mean_acc, sblk / (float)mean_n);
    }
  }
}

// ----------------------------------------------------------------------------------------------------------
// Per-sample reductions: out[b] = sum_i f(x[b][i]) with f = identity (sq=0) or square (sq=1).  One block per
// (sample, slab); slabs are combined with atomics (out must be zeroed by the caller).
__global__ __launch_bounds__(256) void sample_sum_kernel(const float* __restrict__ x, long n, int sq,
                                                         float* __restrict__ out, const DgDet det) {
  __shared__ float red[16];
  const int b = blockIdx.y;
  const float* row = x + (long)b * n;
  float acc = 0.f;
  if ((n & 3) == 0 && (((size_t)row) & 15) == 0) {             // 16-byte loads
    for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (long)gridDim.x * blockDim.x * 4) {
      const float4 v = *(const float4*)(row + i);
      acc += sq ? v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w : v.x + v.y + v.z + v.w;
    }
  } else {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
      const float v = row[i];
      acc += sq ? v * v : v;
    }
  }
  const float s = dg_block_sum(acc, red);
  if (threadIdx.x == 0) dg_acc_add(&out[b], s, gridDim.x, det);
}

// ----------------------------------------------------------------------------------------------------------
// DiffAugment (utils/diff_augment.py:114-132, any p: the per-sample gates arrive as DG_AUG_OFF in t_h / o_x) on [B,1,H,W] fp32, one
// fused gather pass; its geometry and arithmetic are diffaug.h's.  xsum[b] = sum of x[b] (needed by contrast: mean of x + brightness).

// One block per image row (blockIdx.x = row, blockIdx.y = sample): everything that depends on the sample or the row is
// block-uniform, the per-pixel work is 32-bit (the first version decoded a flat 64-bit index per pixel: three 64-bit
// divisions cost more than the pixel's memory traffic - 12.9 us for 16.8 MB).
__global__ __launch_bounds__(256) void diffaug_fwd_kernel(AugP a, const float* __restrict__ x, const float* __restrict__ xsum,
                                                          float* __restrict__ y) {
  const int yy = blockIdx.x, b = blockIdx.y, W = a.W;
  const long HW = (long)a.H * W;
  float* yrow = y + (long)b * HW + (long)yy * W;
  const AugSample s = aug_sample(a, b);
  const AugRow r = aug_row<false>(a, s, yy);
  const float mean = aug_mean(a, s, (a.policy & 4) ? xsum[b] : 0.f);
  const float* xrow = x + (long)b * HW + (long)(r.ok ? r.y : 0) * W;
#pragma unroll 4
  for (int xx = threadIdx.x; xx < W; xx += 256) {
    const float v = aug_fwd_px(s, mean, xrow[aug_src_col(s, xx)]);   // always a valid address: loads of the unrolled trips batch
    yrow[xx] = aug_in_window(r, xx) ? v : 0.f;
  }
}

// DiffAugment + BlurVH in one pass (utils/diff_augment.py:114-132 -> models/ops/common.py:74-88): the augmented image is
// only ever the discriminator's input, so it is never written - every output pixel evaluates the augmentation at its five
// blur taps straight from the source image.  Up to two source sets in one launch (the D phase's real | fake halves,
// trainers/dcgan_amp.py:199-204): sample b < a[0].B reads set 0, the rest set 1.  Grid (row, sample), 4 pixels per thread.
struct AugSrc { AugP a; const float* x; const float* xsum; int parts; };
// The three source rows of an output row go through LDS with 16-byte loads (the translation wraps columns modulo W - 1,
// so the augmented row is a rotated copy: unaligned - read from LDS, not from global memory, where a first version with
// 14 scalar gathers per 4 pixels ran no faster than the two kernels it replaced).
// Round 6: a block owns a BAND of DAB_ROWS output rows of one sample and stages the DAB_ROWS + 2 source rows it needs once
// (one row per output row before: three staged rows per output row, 4096 short blocks per 64 images, 17 us for 34 MB).
#define DAB_ROWS 4
template <typename T>
__global__ __launch_bounds__(256) void diffaug_blur_fwd_kernel(AugSrc s0, AugSrc s1, T* __restrict__ out, int ring) {
  extern __shared__ float s_rows[];               // [DAB_ROWS + 2][W]: source rows of augmented rows y0 - 1 .. y0 + DAB_ROWS
  const int set = (int)blockIdx.y >= s0.a.B;
  const AugP& a = set ? s1.a : s0.a;
  const float* x = set ? s1.x : s0.x;
  const float* xsum = set ? s1.xsum : s0.xsum;
  const int parts = set ? s1.parts : s0.parts;
  const int b = (int)blockIdx.y - (set ? s0.a.B : 0);
  const int y0 = blockIdx.x * DAB_ROWS, H = a.H, W = a.W, W4 = a.W >> 2;
  const long HW = (long)H * W;
  const AugSample s = aug_sample(a, b);
  float sx = 0.f;
  if (a.policy & 4) {
    if (parts > 1) {                              // the producer's partial sums, added in index order (dg_step_prologue_fetch)
      for (int j = 0; j < parts; ++j) sx += xsum[(long)b * parts + j];
    } else sx = xsum[b];
  }
  const float mean = aug_mean(a, s, sx);
  // stage: LDS row r holds the source row of augmented row ya = y0 - 1 + r (rows outside the image are never read below; a
  // row the translation moved out of the image is staged as zeros), with brightness and contrast applied where the pixel is
  // STAGED (once per source pixel, not once per tap that reads it): diffaug_fwd_kernel's pixel.
  // The six rows' loads of a thread are issued TOGETHER (a first version staged row after row: hipcc kept each row's
  // load -> arithmetic -> LDS store a loop of its own, six dependent memory round trips per workgroup - 12 of the launch's 17 us).
  const float* srcr[DAB_ROWS + 2];
  bool okr[DAB_ROWS + 2], inr[DAB_ROWS + 2];
#pragma unroll
  for (int r = 0; r < DAB_ROWS + 2; ++r) {
    const int ya = y0 - 1 + r;
    const AugRow ar = aug_row<false>(a, s, ya);
    inr[r] = ya >= 0 && ya < H;
    okr[r] = ar.ok;
    srcr[r] = x + (long)b * HW + (long)(ar.ok ? ar.y : 0) * W;
  }
  for (int q4 = threadIdx.x; q4 < W4; q4 += 256) {
    float4 pq[DAB_ROWS + 2];
#pragma unroll
    for (int r = 0; r < DAB_ROWS + 2; ++r) pq[r] = *(const float4*)(srcr[r] + q4 * 4);   // (unconditional: srcr is always a valid
                                                                                            //  row - a predicated load costs a vmcnt(0))
#pragma unroll
    for (int r = 0; r < DAB_ROWS + 2; ++r) {
      if (!inr[r]) continue;
      float v[4] = {pq[r].x, pq[r].y, pq[r].z, pq[r].w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float t = aug_fwd_px(s, mean, v[q]);
        v[q] = okr[r] ? t : 0.f;
      }
      *(float4*)(s_rows + r * W + q4 * 4) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
  __syncthreads();
  for (int yy = 0; yy < DAB_ROWS; ++yy) {
    const int y = y0 + yy;
    // the three augmented rows of this output row (reflected at the border): staged row, cut-out columns
    const int yr[3] = {y == 0 ? 1 : y - 1, y, y == H - 1 ? H - 2 : y + 1};
    int c0[3], c1[3];
    const float* rowp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      rowp[k] = s_rows + (yr[k] - y0 + 1) * W;
      const AugRow ar = aug_row<false>(a, s, yr[k]);
      c0[k] = ar.c0;
      c1[k] = ar.c1;
    }
    auto aug = [&](int k, int xx) {               // augmented image at (row k of the three, column xx)
      return (xx >= c0[k] && xx < c1[k]) ? 0.f : rowp[k][aug_src_col(s, xx)];
    };
    T* orow = out + ((long)blockIdx.y * HW + (long)y * W) * 2;
    for (int q4 = threadIdx.x; q4 < W4; q4 += 256) {
      const int x0 = q4 * 4;
      int xl = x0 - 1, xr = x0 + 4;
      if (ring) { if (xl < 0) xl += W; if (xr >= W) xr -= W; }
      else      { if (xl < 0) xl = 1;  if (xr >= W) xr = W - 2; }
      const float c[6] = {aug(1, xl), aug(1, x0), aug(1, x0 + 1), aug(1, x0 + 2), aug(1, x0 + 3), aug(1, xr)};
      float o[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        o[2 * k] = 0.25f * aug(0, x0 + k) + 0.5f * c[k + 1] + 0.25f * aug(2, x0 + k);
        o[2 * k + 1] = 0.25f * c[k] + 0.5f * c[k + 1] + 0.25f * c[k + 2];
      }
      T* op = orow + x0 * 2;
      if constexpr (sizeof(T) == 2) {
        Vec16<bf16>::store((bf16*)op, o);
      } else {
        *(float4*)op = make_float4(o[0], o[1], o[2], o[3]);
        *(float4*)(op + 4) = make_float4(o[4], o[5], o[6], o[7]);
      }
    }
  }
}

// Backward pass 1: gsum[b] = sum over the augmented image of the gradient that reaches x2 (pre-translation
// image): every (y,x) not cut out and with a valid source row contributes once.  blockIdx.x strides the rows.
__global__ __launch_bounds__(256) void diffaug_bwd_sum_kernel(AugP a, const float* __restrict__ gy,
                                                              float* __restrict__ gsum, const DgDet det) {
  __shared__ float red[16];
  const int b = blockIdx.y, W = a.W;
  const long HW = (long)a.H * W;
  const AugSample s = aug_window(a, b);
  float acc = 0.f;
  for (int yy = blockIdx.x; yy < a.H; yy += gridDim.x) {
    const AugRow r = aug_row<false>(a, s, yy);
    const float* row = gy + (long)b * HW + (long)yy * W;
    for (int xx = threadIdx.x; xx < W; xx += 256)
      if (aug_in_window(r, xx)) acc += row[xx];
  }
  const float sblk = dg_block_sum(acc, red);
  if (threadIdx.x == 0) dg_acc_add(&gsum[b], sblk, gridDim.x, det);
}

// Backward pass 2 (gather form of the scatter): gx[b,r,c] from gy.  One block per image row, as the forward kernel.
__global__ __launch_bounds__(256) void diffaug_bwd_kernel(AugP a, const float* __restrict__ gy, const float* __restrict__ gsum,
                                                          float* __restrict__ gx) {
  const int row = blockIdx.x, b = blockIdx.y, W = a.W;
  const long HW = (long)a.H * W;
  float* out = gx + (long)b * HW + (long)row * W;
  const AugSample s = aug_sample(a, b);
  const AugRow r = aug_row<true>(a, s, row);
  const float gm = aug_adj_gm(a, s, (a.policy & 4) ? gsum[b] : 0.f);
  const float* grow = gy + (long)b * HW + (long)(r.ok ? r.y : 0) * W;
  const float gb = grow[W - 1];
#pragma unroll 4
  for (int c = threadIdx.x; c < W; c += 256) out[c] = aug_adj_px(a, s, r, grow, gb, gm, c);
}

// ----------------------------------------------------------------------------------------------------------
static inline bool blur4_ok(const void* a, const void* b, int H, int W) {   // the four-pixel forms
  return W % 4 == 0 && W >= 8 && H >= 2 && ((size_t)a & 15) == 0 && ((size_t)b & 15) == 0;
}

extern "C" {

// dg_blur_fwd + dg_mean_acc(mean_src, mean_n, mean_acc) as one launch (the R1 block: the tangent's BlurVH pass follows the
// kernel that produced the per-sample |g|^2 sums whose mean is logged).  DG_EUNSUPPORTED - nothing launched - unless the
// four-pixel form applies.
int dg_blur_fwd_mean(const float* x, void* out, int dtype, int B, int H, int W, int ring, const float* mean_src, int mean_n,
                     float* mean_acc, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  if (!mean_src || !mean_acc || mean_n < 1) return DG_EINVAL;
  if (!blur4_ok(x, out, H, W)) return DG_EUNSUPPORTED;
  if (dtype == DG_BF16) blur_fwd4_kernel<bf16><<<dim3(H, B), 256, 0, s>>>(x, (bf16*)out, B, H, W, ring, mean_src, mean_n, mean_acc);
  else blur_fwd4_kernel<float><<<dim3(H, B), 256, 0, s>>>(x, (float*)out, B, H, W, ring, mean_src, mean_n, mean_acc);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_blur_fwd(const float* x, void* out, int dtype, int B, int H, int W, int ring, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  const long n = (long)B * H * W;
  if (blur4_ok(x, out, H, W)) {
    if (dtype == DG_BF16) blur_fwd4_kernel<bf16><<<dim3(H, B), 256, 0, s>>>(x, (bf16*)out, B, H, W, ring, nullptr, 0, nullptr);
    else blur_fwd4_kernel<float><<<dim3(H, B), 256, 0, s>>>(x, (float*)out, B, H, W, ring, nullptr, 0, nullptr);
  } else if (dtype == DG_BF16) blur_fwd_kernel<bf16><<<nblk(n), 256, 0, s>>>(x, (bf16*)out, B, H, W, ring);
  else blur_fwd_kernel<float><<<nblk(n), 256, 0, s>>>(x, (float*)out, B, H, W, ring);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_blur_bwd(const void* d, int dtype, float* dx, int B, int H, int W, int ring, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  const long n = (long)B * H * W;
  if (blur4_ok(d, dx, H, W)) blur_bwd4_launch(d, dtype, dx, B, H, W, ring, 1.f, nullptr, 1, AugP{}, 0, s);
  else if (dtype == DG_BF16) blur_bwd_kernel<bf16><<<nblk(n), 256, 0, s>>>((const bf16*)d, dx, B, H, W, ring);
  else blur_bwd_kernel<float><<<nblk(n), 256, 0, s>>>((const float*)d, dx, B, H, W, ring);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

// BlurVH adjoint for the R1 chain: dx = oscale * g, ssq[b] += |g_b|^2 (ssq zeroed by the caller); DG_EUNSUPPORTED unless
// W % 4 == 0 and H W % 1024 == 0 (the caller then runs dg_blur_bwd + dg_sample_sum + dg_scale)
int dg_blur_bwd_r1(const void* d, int dtype, float* dx, float oscale, float* ssq, int B, int H, int W, int ring, void* s_) {
  if (!ssq) return DG_EINVAL;
  if (!blur4_ok(d, dx, H, W) || ((long)H * W) % 1024 != 0) return DG_EUNSUPPORTED;
  blur_bwd4_launch(d, dtype, dx, B, H, W, ring, oscale, ssq, blur_rows_pb(H), AugP{}, 0, (hipStream_t)s_);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

// dg_blur_bwd_r1 + dg_blur_fwd_mean as ONE launch: out[b] = BlurVH(oscale * BlurVH^T(d[b])) in `dtype` (the R1 tangent's first
// feature map from the real chain's last gradient map), ssq[b] += |BlurVH^T(d[b])|^2, mean_acc[0] += sum_b of that / mean_n
// (mean_acc optional).  ssq / mean_acc zeroed by the caller.  DG_EUNSUPPORTED - nothing launched - unless W % 4 == 0,
// H % 4 == 0 and the band's six image rows fit 64 KB of LDS.
int dg_blur_r1_tangent(const void* d, int dtype, void* out, float oscale, float* ssq, float* mean_acc, int mean_n, int B, int H,
                       int W, int ring, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  if (!d || !out || !ssq || B <= 0 || (mean_acc && mean_n < 1)) return DG_EINVAL;
  if (dtype != DG_BF16 && dtype != DG_F32) return DG_EINVAL;
  const size_t lds = (size_t)(R1T_ROWS + 2) * W * sizeof(float);
  if (W % 4 != 0 || W < 8 || H < 4 || H % R1T_ROWS != 0 || lds > 60 * 1024 || ((size_t)d & 15) != 0 || ((size_t)out & 15) != 0)
    return DG_EUNSUPPORTED;
  const dim3 grid(H / R1T_ROWS, B);
  const DgDet det = dg_det_current();
  if (dtype == DG_BF16) blur_r1_tangent_kernel<bf16><<<grid, 256, lds, s>>>((const bf16*)d, (bf16*)out, H, W, ring, oscale, ssq, mean_acc, mean_n, det);
  else blur_r1_tangent_kernel<float><<<grid, 256, lds, s>>>((const float*)d, (float*)out, H, W, ring, oscale, ssq, mean_acc, mean_n, det);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

static int sample_sum_impl(const float* x, int B, long n, int sq, float* out, bool zero, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  if (zero) { const int zrc = dg_zero_f32(out, B, s); if (zrc) return zrc; }
  unsigned gx = nblk(n, 256 * 8);
  if (gx > 64) gx = 64;
  if (gx < 1) gx = 1;
  sample_sum_kernel<<<dim3(gx, B), 256, 0, s>>>(x, n, sq, out, dg_det_current());
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_sample_sum(const float* x, int B, long n, int sq, float* out, void* s_) {
  return sample_sum_impl(x, B, n, sq, out, true, s_);
}
int dg_sample_sum_acc(const float* x, int B, long n, int sq, float* out, void* s_) {
  return sample_sum_impl(x, B, n, sq, out, false, s_);
}

// xsum: [B] workspace (per-sample sum of x), y: [B,H,W]
static int diffaug_fwd_impl(const float* x, const float* u_b, const float* u_c, const int* t_h, const int* t_w,
                            const int* o_x, const int* o_y, int policy, int B, int H, int W, float* xsum, float* y,
                            bool zero, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  const AugP a = make_aug(u_b, u_c, t_h, t_w, o_x, o_y, policy, B, H, W);
  if (policy & 4) {
    const int rc = sample_sum_impl(x, B, (long)H * W, 0, xsum, zero, s);
    if (rc) return rc;
  }
  diffaug_fwd_kernel<<<dim3(H, B), 256, 0, s>>>(a, x, xsum, y);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_diffaug_fwd(const float* x, const float* u_b, const float* u_c, const int* t_h, const int* t_w,
                   const int* o_x, const int* o_y, int policy, int B, int H, int W, float* xsum, float* y,
                   void* s_) {
  return diffaug_fwd_impl(x, u_b, u_c, t_h, t_w, o_x, o_y, policy, B, H, W, xsum, y, true, s_);
}
int dg_diffaug_fwd_acc(const float* x, const float* u_b, const float* u_c, const int* t_h, const int* t_w,
                       const int* o_x, const int* o_y, int policy, int B, int H, int W, float* xsum, float* y,
                       void* s_) {
  return diffaug_fwd_impl(x, u_b, u_c, t_h, t_w, o_x, o_y, policy, B, H, W, xsum, y, false, s_);
}

// xsum already holds the per-sample sums of x (dg_fetch_reals_sum / dg_head_post_fwd_sum): no pass of its own
int dg_diffaug_fwd_pre(const float* x, const float* u_b, const float* u_c, const int* t_h, const int* t_w,
                       const int* o_x, const int* o_y, int policy, int B, int H, int W, const float* xsum, float* y,
                       void* s_) {
  hipStream_t s = (hipStream_t)s_;
  const AugP a = make_aug(u_b, u_c, t_h, t_w, o_x, o_y, policy, B, H, W);
  diffaug_fwd_kernel<<<dim3(H, B), 256, 0, s>>>(a, x, xsum, y);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

// DiffAugment + BlurVH forward for one or two source sets (set k fills samples [k B, (k + 1) B) of `out`); xsum_k = the
// per-sample sums of x_k (dg_fetch_reals_sum / dg_head_post_fwd_sum).  DG_EUNSUPPORTED unless W % 4 == 0.
int dg_diffaug_blur_fwd(const DgAugSet* sets, int nsets, int policy, int B, int H, int W, int ring, void* out, int dtype,
                        void* s_) {
  hipStream_t s = (hipStream_t)s_;
  if (!sets || nsets < 1 || nsets > 2 || !out || B <= 0) return DG_EINVAL;
  if (W % 4 != 0 || W < 8 || H < 2 || ((size_t)out & 15) != 0) return DG_EUNSUPPORTED;
  for (int k = 0; k < nsets; ++k)
    if (((size_t)sets[k].x & 15) != 0) return DG_EUNSUPPORTED;       // 16-byte row loads
  AugSrc src[2];
  for (int k = 0; k < 2; ++k) {
    const DgAugSet& q = sets[k < nsets ? k : 0];
    if (!q.x || ((policy & 4) && !q.xsum)) return DG_EINVAL;
    src[k].a = make_aug(q.u_b, q.u_c, q.t_h, q.t_w, q.o_x, q.o_y, policy, B, H, W);
    src[k].x = q.x;
    src[k].xsum = q.xsum;
    src[k].parts = q.xsum_parts;
    if (q.xsum_parts < 0 || q.xsum_parts > 256) return DG_EINVAL;
  }
  if (H % DAB_ROWS != 0) return DG_EUNSUPPORTED;                     // bands of DAB_ROWS output rows
  const dim3 grid(H / DAB_ROWS, nsets * B);
  const size_t lds = (size_t)(DAB_ROWS + 2) * W * sizeof(float);
  if (lds > 60 * 1024) return DG_EUNSUPPORTED;
  if (dtype == DG_BF16) diffaug_blur_fwd_kernel<bf16><<<grid, 256, lds, s>>>(src[0], src[1], (bf16*)out, ring);
  else diffaug_blur_fwd_kernel<float><<<grid, 256, lds, s>>>(src[0], src[1], (float*)out, ring);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

// BlurVH adjoint that also accumulates what DiffAugment's adjoint needs from its input: gsum[b] += sum of dx[b] over the
// rows / columns whose gradient reaches the source image (gsum zeroed by the caller); then dg_diffaug_bwd_pre.
int dg_blur_bwd_augsum(const void* d, int dtype, float* dx, const int* t_h, const int* o_x, const int* o_y, int policy,
                       float* gsum, int B, int H, int W, int ring, void* s_) {
  if (!gsum) return DG_EINVAL;
  if (!blur4_ok(d, dx, H, W)) return DG_EUNSUPPORTED;
  const AugP win = make_aug(nullptr, nullptr, t_h, nullptr, o_x, o_y, policy, B, H, W);   // (the window: aug_window reads these three)
  blur_bwd4_launch(d, dtype, dx, B, H, W, ring, 1.f, gsum, blur_rows_pb(H), win, 1, (hipStream_t)s_);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

// DiffAugment's adjoint with gsum already made (dg_blur_bwd_augsum): the gather pass only
int dg_diffaug_bwd_pre(const float* gy, const float* u_b, const float* u_c, const int* t_h, const int* t_w,
                       const int* o_x, const int* o_y, int policy, int B, int H, int W, const float* gsum, float* gx,
                       void* s_) {
  hipStream_t s = (hipStream_t)s_;
  const AugP a = make_aug(u_b, u_c, t_h, t_w, o_x, o_y, policy, B, H, W);
  diffaug_bwd_kernel<<<dim3(H, B), 256, 0, s>>>(a, gy, gsum, gx);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

static int diffaug_bwd_impl(const float* gy, const float* u_b, const float* u_c, const int* t_h, const int* t_w,
                            const int* o_x, const int* o_y, int policy, int B, int H, int W, float* gsum, float* gx,
                            bool zero, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  const AugP a = make_aug(u_b, u_c, t_h, t_w, o_x, o_y, policy, B, H, W);
  if (policy & 4) {
    if (zero) { const int zrc = dg_zero_f32(gsum, B, s); if (zrc) return zrc; }
    unsigned gxn = (unsigned)((H + 3) / 4);                            // a block sums ~4 rows: one atomic per block
    if (gxn > 64) gxn = 64;
    diffaug_bwd_sum_kernel<<<dim3(gxn, B), 256, 0, s>>>(a, gy, gsum, dg_det_current());
  }
  diffaug_bwd_kernel<<<dim3(H, B), 256, 0, s>>>(a, gy, gsum, gx);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}
int dg_diffaug_bwd(const float* gy, const float* u_b, const float* u_c, const int* t_h, const int* t_w,
                   const int* o_x, const int* o_y, int policy, int B, int H, int W, float* gsum, float* gx,
                   void* s_) {
  return diffaug_bwd_impl(gy, u_b, u_c, t_h, t_w, o_x, o_y, policy, B, H, W, gsum, gx, true, s_);
}
int dg_diffaug_bwd_acc(const float* gy, const float* u_b, const float* u_c, const int* t_h, const int* t_w,
                       const int* o_x, const int* o_y, int policy, int B, int H, int W, float* gsum, float* gx,
                       void* s_) {
  return diffaug_bwd_impl(gy, u_b, u_c, t_h, t_w, o_x, o_y, policy, B, H, W, gsum, gx, false, s_);
}

}  // extern "C"
