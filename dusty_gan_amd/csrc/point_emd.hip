// Earth mover's distance between point clouds (the reference's native CUDA extension
// utils/metrics/distance/emd/earth_mover_distance.cu), gfx950:
//   * emd_sweeps      : the approximate matching's annealing levels, one device body for both kernels.
//   * emd_kernel      : the matching cost of all pairs or of the diagonal pairing (dg_emd).
//   * emd_grad_kernel : the cost and its gradient to both clouds, `match` held constant (dg_emd_grad).
#include "common.h"

namespace {

// Earth mover's distance, approximate matching (utils/metrics/distance/emd/earth_mover_distance.cu:28-190 approxmatch,
// :218-262 matchcost): ten annealing levels exp(-4^j d^2), j = 7 .. -1, then 0; per level the three sweeps of the
// reference (left ratios, right consumption, matched mass).  The match matrix is never stored: matchcost is linear in
// it, so the cost sum_{k,l} match[l][k] d^2(k,l) is accumulated while the mass is produced.  One workgroup per cloud
// pair, both clouds and the four mass vectors in LDS.  (i, j) = (blockIdx.y, blockIdx.x), or the diagonal pairing
// (i = j) when `paired`.
// The sweeps are one device body for dg_emd and dg_emd_grad.  GRAD adds the gradient of matchcost with `match` held constant
// (matchcostgrad1 / matchcostgrad2, :305-388): match = sum over the levels of w, and both gradients are linear in it, so they
// are accumulated while the mass is produced, like the cost:
//   ga[k] = gscale * sum_levels sum_l w (A_k - B_l)      in the third sweep, by the thread that owns k;
//   gb[l] = gscale * sum_levels sum_k w (B_l - A_k)      in a FOURTH sweep per level, where a thread owns l and forms w again
//                                                        with the third sweep's product order (the same match bits).
// The accumulators are the output rows themselves: one thread owns row k (row l) in every level, adds the level's share to it
// and scales it after the last, so there are no atomics, no [m,n] buffer and no LDS beyond dg_emd's.  A level's share is
// summed in registers from zero and added to the row once: the steep levels leave large entries, and the later levels' small
// terms added to them one at a time would each be rounded at the row's magnitude (on 520 x 1030 points one running sum over
// all levels lay 5e-6 from the float64 gradient, the per-level sums 6e-7, which is the error of `match` itself).  The fourth sweep
// reads what the third leaves alone (the points, ratioL, ratioR), so it follows it without a barrier.
// Returns the thread's share of the cost; GRAD = false is dg_emd's arithmetic, statement for statement.
template <bool GRAD>
__device__ __forceinline__ float emd_sweeps(const float* __restrict__ a, int n, const float* __restrict__ b, int m,
                                            unsigned char* lds, float* __restrict__ ga, float* __restrict__ gb,
                                            float gscale) {
  float4* p1 = (float4*)lds;                // [n]
  float4* p2 = p1 + n;                      // [m]
  float* remainL = (float*)(p2 + m);        // [n]
  float* remainR = remainL + n;             // [m]
  float* ratioL = remainR + m;              // [n]
  float* ratioR = ratioL + n;               // [m]
  const int tid = threadIdx.x, nt = blockDim.x;
  const float multiL = n >= m ? 1.f : (float)(m / n), multiR = n >= m ? (float)(n / m) : 1.f;
  for (int k = tid; k < n; k += nt) { p1[k] = make_float4(a[k * 3], a[k * 3 + 1], a[k * 3 + 2], 0.f); remainL[k] = multiL; }
  for (int l = tid; l < m; l += nt) { p2[l] = make_float4(b[l * 3], b[l * 3 + 1], b[l * 3 + 2], 0.f); remainR[l] = multiR; }
  __syncthreads();
  float cost = 0.f;
  for (int lev = 7; lev >= -2; --lev) {
    const float level = lev == -2 ? 0.f : -powf(4.0f, (float)lev);
    for (int k = tid; k < n; k += nt) {
      const float4 x = p1[k];
      float suml = 1e-9f;
      for (int l = 0; l < m; ++l) {
        const float4 q = p2[l];
        const float d = (q.x - x.x) * (q.x - x.x) + (q.y - x.y) * (q.y - x.y) + (q.z - x.z) * (q.z - x.z);
        suml += __expf(level * d) * remainR[l];
      }
      ratioL[k] = remainL[k] / suml;
    }
    __syncthreads();
    for (int l = tid; l < m; l += nt) {
      const float4 q = p2[l];
      float sumr = 0.f;
      for (int k = 0; k < n; ++k) {
        const float4 x = p1[k];
        const float d = (q.x - x.x) * (q.x - x.x) + (q.y - x.y) * (q.y - x.y) + (q.z - x.z) * (q.z - x.z);
        sumr += __expf(level * d) * ratioL[k];
      }
      const float r = remainR[l];
      sumr *= r;
      const float consumption = fminf(r / (sumr + 1e-9f), 1.0f);
      ratioR[l] = consumption * r;
      remainR[l] = fmaxf(0.0f, r - sumr);
    }
    __syncthreads();
    for (int k = tid; k < n; k += nt) {
      const float4 x = p1[k];
      const float rl = ratioL[k];
      float suml = 0.f;
      float gx = 0.f, gy = 0.f, gz = 0.f;   // this level's share, summed on its own (see above)
      for (int l = 0; l < m; ++l) {
        const float4 q = p2[l];
        const float d = (q.x - x.x) * (q.x - x.x) + (q.y - x.y) * (q.y - x.y) + (q.z - x.z) * (q.z - x.z);
        const float w = __expf(level * d) * rl * ratioR[l];
        cost += w * d;       // matchcost (:218-262): match[l][k] * d, summed over levels
        suml += w;
        if (GRAD) { gx += w * (x.x - q.x); gy += w * (x.y - q.y); gz += w * (x.z - q.z); }
      }
      remainL[k] = fmaxf(0.0f, remainL[k] - suml);
      if (GRAD) {
        if (lev != 7) { gx += ga[k * 3]; gy += ga[k * 3 + 1]; gz += ga[k * 3 + 2]; }
        const float sc = lev == -2 ? gscale : 1.f;   // the reference scales after the sum
        ga[k * 3] = gx * sc; ga[k * 3 + 1] = gy * sc; ga[k * 3 + 2] = gz * sc;
      }
    }
    if (GRAD) {
      for (int l = tid; l < m; l += nt) {
        const float4 q = p2[l];
        const float rr = ratioR[l];
        float gx = 0.f, gy = 0.f, gz = 0.f;
        for (int k = 0; k < n; ++k) {
          const float4 x = p1[k];
          const float d = (q.x - x.x) * (q.x - x.x) + (q.y - x.y) * (q.y - x.y) + (q.z - x.z) * (q.z - x.z);
          const float w = __expf(level * d) * ratioL[k] * rr;
          gx += w * (q.x - x.x); gy += w * (q.y - x.y); gz += w * (q.z - x.z);
        }
        if (lev != 7) { gx += gb[l * 3]; gy += gb[l * 3 + 1]; gz += gb[l * 3 + 2]; }
        const float sc = lev == -2 ? gscale : 1.f;
        gb[l * 3] = gx * sc; gb[l * 3 + 1] = gy * sc; gb[l * 3 + 2] = gz * sc;
      }
    }
    __syncthreads();
  }
  return cost;
}

__global__ __launch_bounds__(512) void emd_kernel(const float* __restrict__ A, int n, const float* __restrict__ Bc,
                                                  int m, int Nb, int paired, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char emd_lds[];
  __shared__ float red[16];
  const int j = blockIdx.x, i = paired ? blockIdx.x : blockIdx.y;
  const float cost = emd_sweeps<false>(A + (long)i * n * 3, n, Bc + (long)j * m * 3, m, emd_lds, nullptr, nullptr, 0.f);
  const float tot = dg_block_sum(cost, red);
  if (threadIdx.x == 0) out[paired ? (long)i : (long)i * Nb + j] = tot;
}

// dg_emd_grad: pair i = blockIdx.x.  gscale = 2 grad_cost[i] (the 2 of d|p - q|^2, exact).
__global__ __launch_bounds__(512) void emd_grad_kernel(const float* __restrict__ A, int n, const float* __restrict__ Bc, int m,
                                                       const float* __restrict__ grad_cost, float* __restrict__ cost_out,
                                                       float* __restrict__ gradA, float* __restrict__ gradB) {
  extern __shared__ __attribute__((aligned(16))) unsigned char emd_lds[];
  __shared__ float red[16];
  const long i = blockIdx.x;
  const float gscale = 2.f * (grad_cost ? grad_cost[i] : 1.f);
  const float cost = emd_sweeps<true>(A + i * n * 3, n, Bc + i * m * 3, m, emd_lds, gradA + i * n * 3, gradB + i * m * 3, gscale);
  const float tot = dg_block_sum(cost, red);
  if (threadIdx.x == 0 && cost_out) cost_out[i] = tot;
}

}  // namespace

extern "C" {

int dg_emd(const float* A, int Na, int n, const float* Bc, int Nb, int m, int paired, float* out, void* s_) {
  if (!A || !Bc || !out || Na <= 0 || Nb <= 0 || n <= 0 || m <= 0) return DG_EINVAL;
  if (paired && Na != Nb) return DG_EINVAL;
  const size_t lds = (size_t)(n + m) * (16 + 8);
  if (lds > 150 * 1024) return DG_EUNSUPPORTED;
  static bool opted = false;
  if (!opted) {
    HIP_CHECK_RET(hipFuncSetAttribute((const void*)emd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
    opted = true;
  }
  const dim3 grid(Nb, paired ? 1 : Na);
  if (grid.y > 65535) return DG_EUNSUPPORTED;
  emd_kernel<<<grid, 512, lds, (hipStream_t)s_>>>(A, n, Bc, m, Nb, paired, out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_emd_grad(const float* A, int n, const float* Bc, int m, int B, const float* grad_cost, float* cost, float* gradA,
                float* gradB, void* s_) {
  if (!A || !Bc || !gradA || !gradB || B <= 0 || n <= 0 || m <= 0) return DG_EINVAL;
  const size_t lds = (size_t)(n + m) * (16 + 8);   // dg_emd's: the gradient rows are the accumulators
  if (lds > 150 * 1024) return DG_EUNSUPPORTED;
  static bool opted = false;
  if (!opted) {
    HIP_CHECK_RET(hipFuncSetAttribute((const void*)emd_grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
    opted = true;
  }
  emd_grad_kernel<<<B, 512, lds, (hipStream_t)s_>>>(A, n, Bc, m, grad_cost, cost, gradA, gradB);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

}  // extern "C"
