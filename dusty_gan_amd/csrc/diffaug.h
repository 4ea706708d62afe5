// DiffAugment's geometry and arithmetic, written ONCE (utils/diff_augment.py:114-132, any p) for every kernel that evaluates it:
// the forward gathers and the adjoint's sum and gather (blur_aug.hip), the BlurVH adjoint's window sum (blur_aug.hip) and the
// head post-processing's backward, which applies the adjoint gather on the fly (head_post.hip, HeadGradAug).  Every one of the
// reference's quirks lives here and nowhere else: the applied factor is u * u, the translation wraps columns
// modulo W - 1, so that output columns 0 and W - 1 read the same source column, and shifted-out rows read zero.
// policy bits: 1 brightness, 2 saturation (identity for one channel), 4 contrast, 8 translation, 16 cutout.
// Per-sample parameters: u_b, u_c (the uniform(-1,1) draws), t_h, t_w, o_x, o_y ints.
// The gate of p < 1 (rand_translation / rand_cutout restore y[~mask] = x[~mask], :53-102) is per SAMPLE and travels in those
// arrays: t_h[b] == DG_AUG_OFF switches the translation off for sample b, o_x[b] == DG_AUG_OFF the cutout - the stage is then
// what it is outside the policy, the exact identity (a shift by 0 would not be: the wrap modulo W - 1 folds column W - 1 onto
// column 0).  So whatever chooses between "the stage runs" and "it does not" below chooses on AugSample::tr / ::cut, never on the
// policy bit.  The colour stages have no gate: the reference overwrites their Bernoulli draw.
#pragma once
#include "common.h"

struct AugP {
  const float *u_b, *u_c;
  const int *t_h, *t_w, *o_x, *o_y;
  int policy, B, H, W, cut_h, cut_w;
};
static AugP make_aug(const float* u_b, const float* u_c, const int* t_h, const int* t_w, const int* o_x,
                     const int* o_y, int policy, int B, int H, int W) {
  AugP a;
  a.u_b = u_b; a.u_c = u_c; a.t_h = t_h; a.t_w = t_w; a.o_x = o_x; a.o_y = o_y;
  a.policy = policy; a.B = B; a.H = H; a.W = W;
  a.cut_h = (int)(H * 0.5 + 0.5);  // utils/diff_augment.py:85
  a.cut_w = (int)(W * 0.5 + 0.5);
  return a;
}

// ---- the per-sample part.  A stage that is not in the policy leaves its identity: no shift, br = 0, cc = 1 (r0 / cl are
//      read under AugSample::cut only: aug_row).
struct AugSample {
  int th, tw, wm;  // row shift; column shift t_w mod wm, non-negative; the column modulus: W - 1 under translation (the
                   // reference's wrap), W without it (never reached: no wrap)
  int r0, cl;      // the cut-out box [r0, r0 + cut_h) x [cl, cl + cut_w), in the augmented image's coordinates
  bool tr, cut;    // the stage runs for THIS sample: in the policy and not gated off (block- or wave-uniform in every caller:
                   // the sample index is, so the compares below stay on the scalar side)
  float br, cc;    // brightness 0.5 u^2, contrast 1 + 0.5 u^2
};
// which pixels of the augmented image come from the source image at all: the row shift and the box (t_h, o_x, o_y only - the
// BlurVH adjoint's window sum has no other parameter; both sentinels arrive in these)
__device__ __forceinline__ AugSample aug_window(const AugP& a, int b) {
  AugSample s = {0, 0, a.W, 0, 0, false, false, 0.f, 1.f};
  if (a.policy & 8) {
    const int th = a.t_h[b];
    s.tr = th != DG_AUG_OFF;
    s.th = s.tr ? th : 0;
  }
  if (a.policy & 16) {
    const int ox = a.o_x[b];
    s.cut = ox != DG_AUG_OFF;
    if (s.cut) { s.r0 = ox - a.cut_h / 2; s.cl = a.o_y[b] - a.cut_w / 2; }
  }
  return s;
}
__device__ __forceinline__ AugSample aug_sample(const AugP& a, int b) {
  AugSample s = aug_window(a, b);
  if (s.tr) {
    const int Wm1 = a.W - 1;
    s.wm = Wm1;
    s.tw = a.t_w[b] % Wm1;
    if (s.tw < 0) s.tw += Wm1;                     // (x + t_w) mod (W - 1) = x + tw, minus W - 1 once at most
  }
  if (a.policy & 1) { const float u = a.u_b[b]; s.br = 0.5f * u * u; }
  if (a.policy & 4) { const float u = a.u_c[b]; s.cc = 1.f + 0.5f * u * u; }
  return s;
}
// contrast's pivot, the mean of the brightened image, from the sample's sum of x (0 without contrast: the pixel below is then
// the identity), and its adjoint's constant term from the window sum of the gradient
__device__ __forceinline__ float aug_mean(const AugP& a, const AugSample& s, float xsum) {
  return (a.policy & 4) ? xsum / (float)((long)a.H * a.W) + s.br : 0.f;
}
__device__ __forceinline__ float aug_adj_gm(const AugP& a, const AugSample& s, float gsum) {
  return (a.policy & 4) ? (1.f - s.cc) * gsum / (float)((long)a.H * a.W) : 0.f;
}

// ---- the per-row part.  Forward: augmented row y reads source row y + t_h.  Adjoint: source row y receives from augmented row
//      y - t_h.  `y` = that other row, `ok` = it lies in the image, [c0, c1) = the cut-out columns of the AUGMENTED row of the
//      pair (empty outside the box).
struct AugRow { int y; bool ok; int c0, c1; };
template <bool kAdjoint>
__device__ __forceinline__ AugRow aug_row(const AugP& a, const AugSample& s, int y) {
  AugRow r;
  r.y = kAdjoint ? y - s.th : y + s.th;
  r.ok = r.y >= 0 && r.y < a.H;
  const int ya = kAdjoint ? r.y : y;
  const bool cut = s.cut && ya >= s.r0 && ya < s.r0 + a.cut_h;
  r.c0 = cut ? s.cl : 0;
  r.c1 = cut ? s.cl + a.cut_w : 0;
  return r;
}
// source column of augmented column x
__device__ __forceinline__ int aug_src_col(const AugSample& s, int x) {
  int sx = x + s.tw;
  if (sx >= s.wm) sx -= s.wm;
  return sx;
}

// ---- the forward pixel: brightness, then contrast about the mean (a stage outside the policy is exact: + 0, 0 + 1 (v - 0))
__device__ __forceinline__ float aug_fwd_px(const AugSample& s, float mean, float v) {
  v += s.br;
  return mean + s.cc * (v - mean);
}

// ---- the adjoint's window: does the gradient at column x of forward row `r` of the augmented image reach the source image?
//      (diffaug_bwd_sum_kernel and the BlurVH adjoint's window sum add exactly these)
__device__ __forceinline__ bool aug_in_window(const AugRow& r, int x) { return r.ok && !(x >= r.c0 && x < r.c1); }

// ---- the adjoint-gather pixel (gather form of the forward's scatter): the gradient at column c of the source row whose adjoint
//      row is `r`.  grow = row (r.ok ? r.y : 0) of gy and gb = grow[W - 1]: valid addresses whatever the predicates say, so
//      that the loads of unrolled trips batch.
__device__ __forceinline__ float aug_adj_px(const AugP& a, const AugSample& s, const AugRow& r, const float* __restrict__ grow,
                                            float gb, float gm, int c) {
  const int W = a.W;
  float g2 = 0.f;  // gradient w.r.t. the pre-translation image at column c
  if (s.tr) {
    int w1 = c - s.tw;                                               // (c - t_w) mod (W - 1)
    if (w1 < 0) w1 += W - 1;
    const float ga = grow[w1];
    if (r.ok && c <= W - 2) {
      if (!(w1 >= r.c0 && w1 < r.c1)) g2 += ga;
      // columns 0 and W-1 of the output both read source column (t_w mod (W-1))
      if (w1 == 0 && !(W - 1 >= r.c0 && W - 1 < r.c1)) g2 += gb;
    }
  } else {
    const float ga = grow[c];
    if (!(c >= r.c0 && c < r.c1)) g2 = ga;
  }
  return (a.policy & 4) ? s.cc * g2 + gm : g2;
}

// Where head_post_bwd_kernel (head_post.hip) gets d loss / d depth of a pixel quad from when DiffAugment's adjoint gather is
// applied on the fly to the BlurVH adjoint's output gy (W % 4 == 0, so a quad lies in one row): the generator's upstream
// gradient is then never written.
struct HeadGradAug {
  AugP a;
  const float* gy;
  const float* gsum;
  template <int PX>
  __device__ __forceinline__ void operator()(int b, long p, long HW, float (&o)[PX]) const {
    static_assert(PX == 4, "the adjoint gather serves the four-pixel backward only");
    const int W = a.W;
    const int row = (int)(p / W), q0 = (int)(p - (long)row * W);
    const AugSample s = aug_sample(a, b);
    const AugRow r = aug_row<true>(a, s, row);
    const float gm = aug_adj_gm(a, s, (a.policy & 4) ? gsum[b] : 0.f);
    const float* grow = gy + (long)b * HW + (long)(r.ok ? r.y : 0) * W;
    const float gb = grow[W - 1];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = aug_adj_px(a, s, r, grow, gb, gm, q0 + k);
  }
};
