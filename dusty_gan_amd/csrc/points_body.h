// The per-point body of the point-cloud projection, written once: points_depth.hip's search (the weighted sums) and
// raydrop.hip's pixel winner (the nearest return) must agree on which points take part and on a point's range, bit for bit.
// Reference: Coordinate.points_to_depth, utils/lidar.py:78-84.  DOUBLE arithmetic on the float32 coordinates: the range test is
// a discontinuity.
#pragma once

// one record -> its range d_u = |xyz| in unit space (r2 = x^2 + y^2 on the way)
__device__ __forceinline__ double pd_range(const float* __restrict__ rec, double& x, double& y, double& z, double& r2) {
  x = (double)rec[0]; y = (double)rec[1]; z = (double)rec[2];
  r2 = x * x + y * y;
  return sqrt(r2 + z * z);
}
// one record -> does the point take part?  (u, v) as the search uses them; wd = w d_u and w as the sums take them
__device__ __forceinline__ bool pd_point(const float* __restrict__ rec, double min_depth, double max_depth, double tau, float& u,
                                         float& v, double& wd, double& w) {
  double x, y, z, r2;
  const double d_u = pd_range(rec, x, y, z, r2), d_m = d_u * max_depth;
  if (!(d_m > min_depth && d_m < max_depth)) return false;   // non-finite coordinates and the origin fail here too
  u = (float)atan2(z, sqrt(r2));
  v = (float)atan2(y, x);
  w = exp(-tau * d_u);
  wd = w * d_u;
  return true;
}
