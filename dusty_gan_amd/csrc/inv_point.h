// One pixel of "generated inverse depth -> point on the sensor's angle grid" (utils/__init__.py:168 and
// Coordinate.inv_to_xyz / revert_depth / pol_to_xyz, utils/lidar.py:38-65), written once: inv_to_xyz_kernel
// (lidar_io.hip) stores the unit-space point map with it and export_points_kernel (synthesis.hip) the compacted metric
// records, so what counts as a valid pixel and where its point lies cannot differ between the two.
#pragma once
#include "common.h"

// the [0,1] inverse depth of a raw input value: from_tanh applies tanh_to_sigmoid(.).clamp_(0, 1) first
__device__ __forceinline__ float dg_inv01(float inv, int from_tanh) {
  if (from_tanh) {  // tanh_to_sigmoid(.).clamp_(0, 1)  utils/__init__.py:168
    inv = (inv + 1.f) / 2.f;
    inv = fminf(fmaxf(inv, 0.f), 1.f);
  }
  return inv;
}

// lidar.py:59: a pixel holds a point when its inverse depth is further than tol from the drop constant
__device__ __forceinline__ bool dg_inv_valid(float inv01, float drop_const, float tol) {
  return fabsf(inv01 - drop_const) > tol;
}

// the unit-space point (metres / max_d) of a pixel; an invalid pixel's point is the origin
__device__ __forceinline__ void dg_inv_point(float inv, bool valid, float min_d, float max_d, float pitch, float yaw,
                                             float& x, float& y, float& z) {
  const float disp = inv * (1.f / min_d - 1.f / max_d) + 1.f / max_d;          // revert_depth :40-43
  float d = 1.f / disp;
  d = (d - min_d) / (max_d - min_d);                                           // :45-46
  d = d * (max_d - min_d) + min_d;                                             // :61
  d = d / max_d;                                                               // :62
  d = valid ? d : 0.f;                                                         // :63
  const float cp = cosf(pitch), sp = sinf(pitch), cy = cosf(yaw), sy = sinf(yaw);
  x = d * cp * cy;                                                             // pol_to_xyz :49-56
  y = d * cp * sy;
  z = d * sp;
}
