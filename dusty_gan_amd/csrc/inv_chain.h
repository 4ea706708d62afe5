// One pixel of "gradient on a generated point -> gradient on the head's outputs" in the inversion's EVAL-mode graph, written
// once: inv_chamfer_grad_kernel and inv_points_grad_kernel (inversion.hip) differ only in where the point gradient gP comes
// from.  gP = d loss_b / d P_p is chained through Coordinate.inv_to_xyz (utils/lidar.py:61-68: the ray's direction from the
// angle grid, d (depth / max_depth) / d inv), the closed-interval clamp and tanh_to_sigmoid (utils/__init__.py:168) to
// g = d loss_b / d (masked depth), then through head_px_bwd<arch> (models/dusty.py:45-59,77-91,107-127): the depth channel
// through mask and tanh, the pixel confidence through the straight-through Gumbel sigmoid under the fixed noise, dusty2's
// image channel 0 (eval: a plain threshold).  add: the gradient is added to what `draw` holds (a term written before).
#pragma once
#include "head_post.h"

// A: the kernel's argument struct.  It carries depth [B,HW] (the masked depth, tanh domain), angle [2,HW], gout [B,nheads,HW],
// noise_pixel [B,HW], mask [B,arch,HW], arch, nheads, cp, add, inv_tau, drop_const, max_d, tol, s_depth, s_conf, HW and the
// outputs draw (planar fp32) / draw_pm (bf16 pixel-major, the planar value rounded).  span = 1 / min_d - 1 / max_d.
template <class A>
__device__ __forceinline__ void inv_point_chain(const A a, int b, long p, long bp, float span, float gx, float gy, float gz) {
  const long HW = a.HW;
  const float pitch = a.angle[p], yaw = a.angle[HW + p];
  const float cpt = cosf(pitch), spt = sinf(pitch), cy = cosf(yaw), sy_ = sinf(yaw);
  const float dot = gx * (cpt * cy) + gy * (cpt * sy_) + gz * spt;
  const float tm = a.depth[bp];                       // the masked depth, tanh domain
  const float raw01 = (tm + 1.f) / 2.f;
  const float inv = fminf(fmaxf(raw01, 0.f), 1.f);
  const bool pass = raw01 >= 0.f && raw01 <= 1.f;     // clamp(0, 1) passes the gradient on the closed interval
  const bool valid = fabsf(inv - 0.f) > a.tol;        // the LiDAR's drop_const is 0 (utils/lidar.py:12)
  const float dep = 1.f / (inv * span + 1.f / a.max_d);
  const float g = (valid && pass) ? 0.5f * (-(span * dep * dep) / a.max_d) * dot : 0.f;
  const float* go = a.gout + (long)b * a.nheads * HW + p;
  const float t = go[0];
  float d0, d1, d2;
  if (a.arch == 0) {
    head_px_bwd<0>(t, g, 0.f, 0.f, 1.f, 1.f, a.inv_tau, a.drop_const, d0, d1, d2);
  } else if (a.arch == 1) {
    head_px_bwd<1>(t, g, go[HW] + a.noise_pixel[bp], 0.f, a.mask[bp], 1.f, a.inv_tau, a.drop_const, d0, d1, d2);
  } else {
    const float* mk = a.mask + (long)b * 2 * HW + p;
    head_px_bwd<2>(t, g, go[HW] + a.noise_pixel[bp], 0.f, mk[0], mk[HW], a.inv_tau, a.drop_const, d0, d1, d2);
    d2 = 0.f;
  }
  float v[3] = {d0 * a.s_depth, d1 * a.s_conf, d2 * a.s_conf};
  if (a.add) {
    const float* q = a.draw + (long)b * a.nheads * HW + p;
    for (int c = 0; c < a.nheads && c < 3; ++c) v[c] += q[c * HW];
  }
  if (a.draw) {
    float* q = a.draw + (long)b * a.nheads * HW + p;
    for (int c = 0; c < a.nheads; ++c) q[c * HW] = c < 3 ? v[c] : 0.f;
  }
  if (a.draw_pm) {
    bf16* q = a.draw_pm + bp * a.cp;
    for (int c = 0; c < a.cp; ++c) q[c] = (bf16)((c < 3 && c < a.nheads) ? v[c] : 0.f);
  }
}
