// C-ABI door to the reference's own device kernels for furthest point sampling and the approximate earth mover's
// distance (utils/sampling/fps/furthest_point_sampling.cu, utils/metrics/distance/emd/earth_mover_distance.cu), built for
// gfx950 from the hipified sources that oracle/Makefile.ref generates under oracle/_ref/src/ (git-ignored).  Test
// infrastructure only: tests/golden/make_fps_emd_golden.py records what these kernels return, tests/test_gpu_metrics.py
// replays the same cases through them where the library is present.  Nothing of the reference is copied here - this
// file includes the generated sources and forwards to them.  Both sources synchronise with __syncthreads() only (no
// shuffles, no warp-size assumptions), so running them on 64-lane waves is meaningful.
//
// All pointers are DEVICE pointers; every door synchronises the device before it returns and hands back the HIP error
// code (0 = hipSuccess).
#include "fps/furthest_point_sampling.hip"
#include "emd/earth_mover_distance.hip"

extern "C" {

// xyz [b,n,3], temp [b,n] (the caller fills it with 1e10, as furthest_point_sampling.cpp does), idx [b,m] int32.
// Goes through the reference's launcher: its opt_n_threads() block-size switch is part of what is pinned.
int ref_fps(int b, int n, int m, const float* xyz, float* temp, int* idx) {
  furthest_point_sampling_kernel_wrapper(b, n, m, xyz, temp, idx);
  return (int)hipDeviceSynchronize();
}

// xyz1 [b,n,3], xyz2 [b,m,3], match [b,m,n], cost [b]; the launch shape <<<32, 512>>> is that of ApproxMatchForward and
// MatchCostForward.  temp: the reference allocates b * (n + m) * 2 floats but indexes it by BLOCK (32 of them) and
// reads ratioL[k] for k up to the next multiple of 512 past n before it tests k < n, so the caller passes at least
// 32 * (n + m) * 2 + 512 floats.
int ref_emd(int b, int n, int m, const float* xyz1, const float* xyz2, float* match, float* temp, float* cost) {
  hipLaunchKernelGGL((approxmatch<float>), dim3(32), dim3(512), 0, 0, b, n, m, xyz1, xyz2, match, temp);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((matchcost<float>), dim3(32), dim3(512), 0, 0, b, n, m, xyz1, xyz2, match, cost);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return (int)hipDeviceSynchronize();
}

}  // extern "C"
