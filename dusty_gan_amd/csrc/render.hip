// The picture log of a training run (gfx950): the bird's-eye view of a point cloud and the image grids.  Reference:
// utils/render.py:18-127 (render_point_clouds over bilinear_rasterizer) and train.py:28-34 (make_grid + colorize + TensorBoard's
// float -> byte conversion), there some forty whole-array torch temporaries and four float scatter_add_ per channel set.
//   * splat_accum / render_points : one thread per point forms the four neighbouring cells, the clamped "safe" indices and the
//     bilinear corner weights (zero where the clamp moved the index, zero below 1e-3) and adds value x weight at the clamped
//     cells.  The sums are 64-bit integers (24.40 fixed point, dg_fix40 of common.h) added with integer atomics: associative, so
//     the image depends neither on the order of the points nor on scheduling.  render_points fuses everything the reference does
//     before the splat (z flip, R, t, pinhole projection, the in-image mask on the normals only, exp(-3 depth) weights) and
//     splats (weight x normal, weight) as four channels in one pass.
//     The per-point arithmetic is DOUBLE on the float32 inputs: floor, the in-image mask and the 1e-3 cut are discontinuities, and
//     in double the decisions fall where the exact formula puts them (a few hundred flops per point against 16 atomics).
//     DEVIATION: a point with a non-finite coordinate (after projection: z' = 0 among them) is skipped - the reference's .long() of
//     NaN is undefined - and so is a term that is non-finite or outside the codec's window.
//   * splat_finish : words -> float [B,C,H,W], optionally channels 0..C-2 divided by (channel C-1 + 1e-8); zeroes the words.
//   * image_grid   : [B,1|3,H,W] float -> uint8 [Hg,Wg,3] laid out as make_grid(nrow=4, padding=2, pad_value=0), through the turbo
//     table (colour) or replicated / as is (plain).
// Global atomics, not an LDS image: an L x L x 4 image of 8-byte words is 8 MiB at L = 512, fifty times a CU's LDS, so a tiled form
// needs the points binned by tile first; the words of a pixel's four channels and of its right neighbour are 64 contiguous bytes.
#include "common.h"
#include "turbo_lut.h"

namespace {

inline int nblk(long n) { return (int)((n + 255) / 256); }

// one corner: value[c] x wt into the C words of cell (hs, ws); wt = 0 where the clamp moved the index or wt < 1e-3
__device__ __forceinline__ void splat_corner(double wt, double hs, double ws, const double* val, int C, int W,
                                             unsigned long long* __restrict__ img) {
  if (!(wt >= 1e-3)) return;
  unsigned long long* cell = img + ((long)hs * W + (long)ws) * C;
  for (int c = 0; c < C; ++c) dg_fix40_add(cell + c, val[c] * wt);
}

// bilinear_rasterizer's body for one point (render.py:79-124); img = this sample's [H,W,C] words
__device__ __forceinline__ void splat_point(double h, double w, const double* val, int C, int H, int W,
                                            unsigned long long* __restrict__ img) {
  if (!(fabs(h) < INFINITY && fabs(w) < INFINITY)) return;   // NaN or infinite: skipped
  const double h_t = floor(h), h_b = h_t + 1.0, w_l = floor(w), w_r = w_l + 1.0;
  const double h_ts = fmin(fmax(h_t, 0.0), (double)(H - 1)), h_bs = fmin(fmax(h_b, 0.0), (double)(H - 1));
  const double w_ls = fmin(fmax(w_l, 0.0), (double)(W - 1)), w_rs = fmin(fmax(w_r, 0.0), (double)(W - 1));
  const double wh_t = h_t == h_ts ? h_b - h : 0.0, wh_b = h_b == h_bs ? h - h_t : 0.0;
  const double ww_l = w_l == w_ls ? w_r - w : 0.0, ww_r = w_r == w_rs ? w - w_l : 0.0;
  splat_corner(wh_t * ww_l, h_ts, w_ls, val, C, W, img);
  splat_corner(wh_t * ww_r, h_ts, w_rs, val, C, W, img);
  splat_corner(wh_b * ww_l, h_bs, w_ls, val, C, W, img);
  splat_corner(wh_b * ww_r, h_bs, w_rs, val, C, W, img);
}

__global__ __launch_bounds__(256) void splat_accum_kernel(const float* __restrict__ coords, const float* __restrict__ values,
                                                          long total, long N, int C, int H, int W,
                                                          unsigned long long* __restrict__ acc) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  double val[4] = {0.0, 0.0, 0.0, 0.0};
  for (int c = 0; c < C; ++c) val[c] = (double)values[i * C + c];
  splat_point((double)coords[2 * i], (double)coords[2 * i + 1], val, C, H, W, acc + (i / N) * ((long)H * W * C));
}

// render_point_clouds up to the splat (render.py:26-62); R [3,3] (R_bs = 0) or [B,3,3] (R_bs = 9), t [3] or [B,3], both nullable
__global__ __launch_bounds__(256) void render_points_kernel(const float* __restrict__ xyz, const float* __restrict__ normals,
                                                            long total, long N, int L, const float* __restrict__ R, long R_bs,
                                                            const float* __restrict__ t, long t_bs, double focal,
                                                            unsigned long long* __restrict__ acc) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long b = i / N;
  double x = (double)xyz[3 * i], y = (double)xyz[3 * i + 1], z = -(double)xyz[3 * i + 2];
  if (R) {   // xyz @ R
    const float* r = R + b * R_bs;
    const double x1 = x * r[0] + y * r[3] + z * r[6], y1 = x * r[1] + y * r[4] + z * r[7], z1 = x * r[2] + y * r[5] + z * r[8];
    x = x1; y = y1; z = z1;
  }
  if (t) {
    const float* tt = t + b * t_bs;
    x += tt[0]; y += tt[1]; z += tt[2];
  }
  const double depth = sqrt(x * x + y * y + z * z);
  if (!(depth > 1e-8)) return;                      // weight 0: every term is zero
  const double wt = exp(-3.0 * depth);
  const double u0 = (x / z * focal + 0.5) * (double)L, u1 = (y / z * focal + 0.5) * (double)L;
  const double lim = (double)(L - 1);
  const double m = (0.0 < u0 && u0 < lim && 0.0 < u1 && u1 < lim) ? wt : 0.0;   // the mask is on the normals only
  const double val[4] = {m * (double)normals[3 * i], m * (double)normals[3 * i + 1], m * (double)normals[3 * i + 2], wt};
  splat_point((double)L - u0, (double)L - u1, val, 4, L, L, acc + b * ((long)L * L * 4));
}

__global__ __launch_bounds__(256) void splat_finish_kernel(unsigned long long* __restrict__ acc, long total, long HW, int C,
                                                           int normalize, float* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  unsigned long long* cell = acc + i * C;
  double v[4];
  for (int c = 0; c < C; ++c) {
    v[c] = dg_fix40_value((long long)cell[c]);
    cell[c] = 0ull;
  }
  const double den = normalize ? v[C - 1] + 1e-8 : 1.0;
  const long b = i / HW, p = i - b * HW;
  for (int c = 0; c < C; ++c) out[(b * C + c) * HW + p] = (float)(normalize && c < C - 1 ? v[c] / den : v[c]);
}

__device__ __forceinline__ unsigned char to_byte(float v) {   // clip(v 255, 0, 255) truncated; NaN -> 0
  return (unsigned char)fminf(fmaxf(v * 255.f, 0.f), 255.f);
}

__global__ __launch_bounds__(256) void image_grid_kernel(const float* __restrict__ x, long sb, int B, int C, int H, int W,
                                                         float scale, int color, int xmaps, int Wg, long total,
                                                         unsigned char* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int gy = (int)(i / Wg), gx = (int)(i - (long)gy * Wg);
  const int ky = gy / (H + 2), oy = gy % (H + 2) - 2, kx = gx / (W + 2), ox = gx % (W + 2) - 2;
  const int k = ky * xmaps + kx;
  const bool inside = oy >= 0 && ox >= 0 && kx < xmaps && k < B;
  const float* px = x + (long)k * sb + (long)oy * W + ox;
  const long HW = (long)H * W;
  float r, g, b;
  if (color) {   // channel 0 through Normalize(0, 1) and the table; the padding (0) is coloured too
    const float v = inside ? px[0] * scale : 0.f;
    if (v != v) {
      r = g = b = 0.f;
    } else {
      const float f = v * 256.f;
      const int idx = f < 0.f ? 0 : (f >= 256.f ? 255 : (int)f);
      r = DG_TURBO_LUT[3 * idx]; g = DG_TURBO_LUT[3 * idx + 1]; b = DG_TURBO_LUT[3 * idx + 2];
    }
  } else {
    r = inside ? px[0] * scale : 0.f;
    g = inside && C == 3 ? px[HW] * scale : r;
    b = inside && C == 3 ? px[2 * HW] * scale : r;
  }
  out[3 * i] = to_byte(r);
  out[3 * i + 1] = to_byte(g);
  out[3 * i + 2] = to_byte(b);
}

}  // namespace

extern "C" {

int dg_splat_accum(const float* coords, const float* values, int B, long N, int C, int H, int W, unsigned long long* acc,
                   void* s_) {
  if (!coords || !values || !acc || B <= 0 || N <= 0 || C < 1 || C > 4 || H <= 0 || W <= 0) return DG_EINVAL;
  if (N > DG_FIX40_MAX_TERMS || (long)H * W > 0x7FFFFFFFl) return DG_EUNSUPPORTED;
  const long total = (long)B * N;
  splat_accum_kernel<<<nblk(total), 256, 0, (hipStream_t)s_>>>(coords, values, total, N, C, H, W, acc);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_render_points(const float* xyz, const float* normals, int B, long N, int L, const float* R, int R_batched, const float* t,
                     int t_batched, double focal, unsigned long long* acc, void* s_) {
  if (!xyz || !normals || !acc || B <= 0 || N <= 0 || L < 2 || L > 32768) return DG_EINVAL;
  if (N > DG_FIX40_MAX_TERMS) return DG_EUNSUPPORTED;
  const long total = (long)B * N;
  render_points_kernel<<<nblk(total), 256, 0, (hipStream_t)s_>>>(xyz, normals, total, N, L, R, R_batched ? 9 : 0, t,
                                                                 t_batched ? 3 : 0, focal, acc);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_splat_finish(unsigned long long* acc, int B, int C, int H, int W, int normalize, float* out, void* s_) {
  if (!acc || !out || B <= 0 || C < 1 || C > 4 || H <= 0 || W <= 0 || (normalize && C < 2)) return DG_EINVAL;
  const long hw = (long)H * W, total = (long)B * hw;
  splat_finish_kernel<<<nblk(total), 256, 0, (hipStream_t)s_>>>(acc, total, hw, C, normalize, out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_image_grid(const float* x, long sample_stride, int B, int C, int H, int W, float scale, int color, unsigned char* out,
                  void* s_) {
  if (!x || !out || B <= 0 || (C != 1 && C != 3) || H <= 0 || W <= 0 || sample_stride < (long)C * H * W) return DG_EINVAL;
  const int xmaps = B < 4 ? B : 4, ymaps = (B + xmaps - 1) / xmaps;
  const long Hg = (long)ymaps * (H + 2) + 2, Wg = (long)xmaps * (W + 2) + 2;
  if (Wg > 0x7FFFFFFFl || Hg > 0x7FFFFFFFl) return DG_EINVAL;
  image_grid_kernel<<<nblk(Hg * Wg), 256, 0, (hipStream_t)s_>>>(x, sample_stride, B, C, H, W, scale, color, xmaps, (int)Wg,
                                                                Hg * Wg, out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_turbo_lut(float* host_out) {
  if (!host_out) return DG_EINVAL;
  for (int i = 0; i < 256 * 3; ++i) host_out[i] = DG_TURBO_LUT[i];
  return DG_OK;
}

}  // extern "C"
