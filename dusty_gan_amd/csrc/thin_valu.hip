// The VALU + LDS kernels of the thin family (picked in conv_thin.hip): the fp32 modes, and shapes the matrix-core kernels refuse.
//   thin_smallk : MODE_S2, K <= 4 input channels -> N = 64*j output channels
//                 Down1 forward / R1 tangent (K = 2, models/gans/dcgan_eqlr.py:90) and Head backward-data (K = 1..3)
//   thin_smalln : MODE_UP, K = 64*j input channels -> N <= 4 output channels
//                 Head forward (dcgan_eqlr.py:29-46) and Down1 backward-data (N = 2)
//   thin_wgrad_down / thin_wgrad_up : weight gradients of the same two layers
// They stage the input rows they need in LDS once (coalesced), keep the workgroup inside ONE output row so the
// reflect / reflect-adjoint tap list is uniform, and write whole 128-B channel rows per pixel.
#include "thin.h"

// ---------------------------------------------------------------------------------------------------------
// thin_smallk: block = (b, coarse row Y), walking the row's 64-column tiles; thread = 4 pixels x 4 channels (N == 64 per pass).
// (Round 5: one block per TILE re-loaded the pass's 16 x K x 64 weights and rebuilt the tap list for every 64 pixels and made
// three dependent round trips to memory per 16 KB of output - 141 us for Down1 forward at 64 samples in the fp32x3 mode.  A block
// now keeps weights and taps for the whole row and has the next tile's input window in flight, in registers, while it computes.)
template <int KMAX>
__global__ __launch_bounds__(256) void thin_smallk_kernel(ConvP p, int tiles_x, int n_base) {
  __shared__ float s_in[6][2 * SK_PX + 2][KMAX];  // up to 6 source rows x 130 fine columns x K
  __shared__ float s_w[16][KMAX][64];
  __shared__ int s_tap[1 + 2 * 6];
  __shared__ float s_db[64];
  const int tid = threadIdx.x;
  const int Y = blockIdx.x % p.Hc, b = blockIdx.x / p.Hc;
  const int Wf = 2 * p.Wc;
  if (tid == 0) {
    int nt = 0;
    for (int i = 0; i < 6; ++i) {
      int r, ky;
      if (dg_tap1d(MODE_S2, p.adj, 0, Y, p.Hc, i, r, ky)) { s_tap[1 + 2 * nt] = r; s_tap[2 + 2 * nt] = ky; ++nt; }
    }
    s_tap[0] = nt;
  }
  if (tid < 64) s_db[tid] = 0.f;
  // weights [tap][k][n] for this pass's 64 output channels
  for (int i = tid; i < 16 * p.K * 64; i += 256) {
    const int n = i & 63, k = (i >> 6) % p.K, t = i / (64 * p.K);
    s_w[t][k][n] = dg_ld(p.w, (long)t * p.w_st + (long)k * p.w_sk + (long)(n_base + n) * p.w_sn, p.w_dtype);
  }
  __syncthreads();
  const int ntap = s_tap[0];
  const int ncol = 2 * SK_PX + 2;
  // the window of a tile: element i = (tap row t, column c, channel k), NPRE per thread; decoded once (the tile only moves c)
  constexpr int NPRE = (6 * (2 * SK_PX + 2) * KMAX + 255) / 256;
  const int nst = ntap * ncol * p.K;
  int pc[NPRE], pl[NPRE];                         // window column, LDS index
  long pg_[NPRE];                                  // source offset without the column
  float pre[NPRE];
#pragma unroll
  for (int u = 0; u < NPRE; ++u) {
    const int i = tid + 256 * u;
    const int k = i % p.K, c = (i / p.K) % ncol, t = min(i / (p.K * ncol), 5);
    pc[u] = c;
    pl[u] = (t * ncol + c) * KMAX + k;
    pg_[u] = (long)b * p.in_sb + (long)s_tap[1 + 2 * (i < nst ? t : 0)] * Wf * p.in_sp + (long)k * p.in_sk;
  }
  auto fetch = [&](int xt) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < NPRE; ++u) {
      if (tid + 256 * u >= nst) continue;
      int col = 2 * xt * SK_PX - 1 + pc[u];
      if (col < 0) col += Wf; else if (col >= Wf) col -= Wf;
      pre[u] = dg_ld(p.in, pg_[u] + (long)col * p.in_sp, p.in_dtype);
    }
  };
  fetch(0);
  const int cg = tid & 15, pg = tid >> 4;  // 4 channels, 4 pixels
  const int n = n_base + cg * 4;
  float bias[4] = {0.f, 0.f, 0.f, 0.f};
  if (p.bias)
    for (int j = 0; j < 4; ++j) bias[j] = p.bias[(n + j) % p.bias_mod];
  float colsum[4] = {0.f, 0.f, 0.f, 0.f};
  const bool x2fast = p.out_dtype == DG_BF16X2 && p.out_sn == 1;   // four consecutive channels: 8 bytes of hi, 8 bytes of lo
  for (int xt = 0; xt < tiles_x; ++xt) {
  const int n0 = xt * SK_PX;
  __syncthreads();                                // (the previous tile's reads of s_in are done)
#pragma unroll
  for (int u = 0; u < NPRE; ++u)
    if (tid + 256 * u < nst) (&s_in[0][0][0])[pl[u]] = pre[u];
  __syncthreads();
  if (xt + 1 < tiles_x) fetch(xt + 1);            // in flight during this tile's arithmetic and stores
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int t = 0; t < ntap; ++t) {
    const int ky = s_tap[2 + 2 * t];
#pragma unroll
    for (int kx = 0; kx < 4; ++kx) {
      for (int k = 0; k < p.K; ++k) {
        const float4 w = *(const float4*)&s_w[ky * 4 + kx][k][cg * 4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float a = s_in[t][2 * (pg * 4 + i) + kx][k];
          acc[i][0] += a * w.x; acc[i][1] += a * w.y; acc[i][2] += a * w.z; acc[i][3] += a * w.w;
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int X = n0 + pg * 4 + i;
    const long o = (long)b * p.out_sb + ((long)Y * p.Wc + X) * p.out_sp + (long)n * p.out_sn;
    if (x2fast) {
      const long q = dg_x2_index(o);
      uint2 ah = make_uint2(0, 0);
      if (p.epi == EPI_MASK) ah = *(const uint2*)((const unsigned short*)p.aux + q);   // (the sign lives in the hi half)
      const unsigned aw[4] = {ah.x << 16, ah.x & 0xffff0000u, ah.y << 16, ah.y & 0xffff0000u};
      unsigned hw[4], lw[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v = dg_epilogue(acc[i][j], p.scale, p.epi, bias[j], __builtin_bit_cast(float, aw[j]));
        const bf16 h = (bf16)v;
        hw[j] = __builtin_bit_cast(unsigned short, h);
        lw[j] = __builtin_bit_cast(unsigned short, (bf16)(v - (float)h));
        colsum[j] += v;
      }
      *(uint2*)((unsigned short*)p.out + q) = make_uint2(hw[0] | (hw[1] << 16), hw[2] | (hw[3] << 16));
      *(uint2*)((unsigned short*)p.out + q + 64) = make_uint2(lw[0] | (lw[1] << 16), lw[2] | (lw[3] << 16));
      continue;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float auxv = p.epi == EPI_MASK ? dg_ld(p.aux, o + j * p.out_sn, p.out_dtype) : 0.f;
      const float v = dg_epilogue(acc[i][j], p.scale, p.epi, bias[j], auxv);
      dg_st(p.out, o + j * p.out_sn, p.out_dtype, v);
      colsum[j] += v;
    }
  }
  }   // tiles of the row
  if (p.dbias) {
    // the block's 64 channel sums in a fixed order (16 pixel groups per channel through LDS), then - with the caller's staging
    // scratch (DgConv.dbias_ws, zero on entry and left zero) - order-independent across blocks: 32.32 fixed-point integer
    // adds onto 64 staging words, a ticket, and the LAST block adds the totals onto dbias once (round 5: the fp32 modes'
    // bias gradients of Down1 / Up3 were float atomics in arrival order)
    __syncthreads();                              // (s_in is dead: its first 16 x 64 floats hold the partial rows)
    float* part = &s_in[0][0][0];
#pragma unroll
    for (int j = 0; j < 4; ++j) part[pg * 64 + cg * 4 + j] = colsum[j];
    __syncthreads();
    if (tid < 64) {
      float v = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) v += part[r * 64 + tid];
      v *= p.rowscale ? p.rowscale[b] : 1.f;
      long long q;
      if (p.dbias_ws && dg_fix1(v, q)) atomicAdd((unsigned long long*)p.dbias_ws + tid, (unsigned long long)q);
      else atomicAdd(&p.dbias[(n_base + tid) % p.bias_mod], v);
    }
    if (p.dbias_ws && dg_block_ticket_last(dg_thin_ws_ticket(p.dbias_ws), gridDim.x) && tid < 64)
      atomicAdd(&p.dbias[(n_base + tid) % p.bias_mod],
                dg_fix1_value((long long)atomicExch((unsigned long long*)p.dbias_ws + tid, 0ull)));
  }
}

// ---------------------------------------------------------------------------------------------------------
// thin_smalln: block = (b, coarse row m), looping over 64-column tiles -> the 2 x 128 fine outputs of each tile.
// Each of the 4 waves owns one output parity (py,px): its tap weights are wave-uniform (LDS broadcast reads in the
// bf16 build, where v_dot2c_f32_bf16 does 2 MACs per VALU instruction with no converts; plain loads + v_fmac in the
// fp32 build).  Input rows m-1, m, m+1 of the tile are staged in LDS once.
// Weights: the T shadow laid out [tap][n][k] (k contiguous).
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

// X2 (T = float): the input is DG_BF16X2 - the staged pixel rows are the same 4 K bytes, read as hi + lo pairs
template <typename T, int N, bool X2 = false>
__global__ __launch_bounds__(256) void thin_smalln_kernel(ConvP p) {
  static_assert(!X2 || sizeof(T) == 4, "DG_BF16X2 input: the fp32 build");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int ES = sizeof(T);
  const int K = p.K;
  const int rowb = K * ES + 16;                  // padded LDS pixel stride
  const int tid = threadIdx.x;
  const int m = blockIdx.x % p.Hc, b = blockIdx.x / p.Hc;
  const int cpr = K * ES / 16;                   // 16-B chunks per pixel
  const T* in = (const T*)p.in;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int py = wave >> 1, px = wave & 1;
  const int Y = 2 * m + py;
  // this wave's taps (wave-uniform): up to 3 row taps (2 regular + 1 reflect-adjoint extra) x 2 column taps
  int trow[3], tky[3], nrow = 0;
  for (int i = 0; i < 4; ++i) {
    int r, ky;
    if (nrow < 3 && dg_tap1d(MODE_UP, p.adj, 0, Y, p.Hc, i, r, ky)) { trow[nrow] = r - (m - 1); tky[nrow] = ky; ++nrow; }
  }
  const int dcol[2] = {px == 0 ? 0 : 1, px == 0 ? -1 : 0};
  const int kxs[2] = {px == 0 ? 1 : 0, px == 0 ? 3 : 2};
  // bf16: the whole [16][N][K] weight block lives in LDS behind the input strip (wave-uniform reads broadcast)
  unsigned char* s_w = smem + 3 * (SN_PX + 2) * rowb;
  if constexpr (ES == 2) {
    for (int i = tid; i < 16 * N * K / 8; i += 256) {
      const int k8 = i % (K / 8), j = (i / (K / 8)) % N, t = i / (K / 8 * N);
      *(uint4*)(s_w + ((t * N + j) * K + k8 * 8) * 2) =
          *(const uint4*)((const T*)p.w + (long)t * p.w_st + (long)j * p.w_sn + k8 * 8);
    }
  }
  for (int n0 = 0; n0 < p.Wc; n0 += SN_PX) {
    __syncthreads();
    for (int i = tid; i < 3 * (SN_PX + 2) * cpr; i += 256) {
      const int ch = i % cpr, c = (i / cpr) % (SN_PX + 2), rr = i / (cpr * (SN_PX + 2));
      const int r = m - 1 + rr;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (r >= 0 && r < p.Hc) {
        int col = n0 - 1 + c;
        if (col < 0) col += p.Wc; else if (col >= p.Wc) col -= p.Wc;
        v = *(const uint4*)(in + (long)b * p.in_sb + ((long)r * p.Wc + col) * p.in_sp + ch * (16 / ES));
      }
      *(uint4*)(smem + ((rr * (SN_PX + 2) + c) * rowb) + ch * 16) = v;
    }
    __syncthreads();
    float acc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.f;
    for (int ti = 0; ti < nrow; ++ti) {
#pragma unroll
      for (int jx = 0; jx < 2; ++jx) {
        const unsigned char* src = smem + ((trow[ti] * (SN_PX + 2) + lane + 1 + dcol[jx]) * rowb);
        const T* wt = (const T*)p.w + (long)(tky[ti] * 4 + kxs[jx]) * p.w_st;  // [n][k] of this tap, uniform
        if constexpr (X2) {
          for (int k0 = 0; k0 < K; k0 += 8) {
            const unsigned char* q = src + (k0 >> 6) * 256 + (k0 & 63) * 2;
            const uint4 h = *(const uint4*)q, l = *(const uint4*)(q + 128);
            const unsigned hw[4] = {h.x, h.y, h.z, h.w}, lw[4] = {l.x, l.y, l.z, l.w};
            float a8[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              a8[2 * e] = __builtin_bit_cast(float, hw[e] << 16) + __builtin_bit_cast(float, lw[e] << 16);
              a8[2 * e + 1] = __builtin_bit_cast(float, hw[e] & 0xffff0000u) + __builtin_bit_cast(float, lw[e] & 0xffff0000u);
            }
#pragma unroll
            for (int j = 0; j < N; ++j) {
              const float* wq = (const float*)(wt + (long)j * p.w_sn + k0);
#pragma unroll
              for (int e = 0; e < 8; ++e) acc[j] += a8[e] * wq[e];
            }
          }
        } else
        for (int k0 = 0; k0 < K; k0 += 16 / ES) {
          const uint4 raw = *(const uint4*)(src + k0 * ES);
          if constexpr (ES == 2) {
            const unsigned a4[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
            for (int j = 0; j < N; ++j) {
              const uint4 wr = *(const uint4*)(s_w + (((tky[ti] * 4 + kxs[jx]) * N + j) * K + k0) * 2);
              const unsigned wq[4] = {wr.x, wr.y, wr.z, wr.w};
#pragma unroll
              for (int q = 0; q < 4; ++q)
                acc[j] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, a4[q]),
                                                         __builtin_bit_cast(bf16x2, wq[q]), acc[j], false);
            }
          } else {
            const float a4[4] = {__builtin_bit_cast(float, raw.x), __builtin_bit_cast(float, raw.y),
                                 __builtin_bit_cast(float, raw.z), __builtin_bit_cast(float, raw.w)};
#pragma unroll
            for (int j = 0; j < N; ++j) {
              const float* wq = (const float*)(wt + (long)j * p.w_sn + k0);
#pragma unroll
              for (int q = 0; q < 4; ++q) acc[j] += a4[q] * wq[q];
            }
          }
        }
      }
    }
    const int X = 2 * (n0 + lane) + px;
    const long o = (long)b * p.out_sb + ((long)Y * (2 * p.Wc) + X) * p.out_sp;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const float sc = p.nscale ? p.scale * p.nscale[j] : p.scale;
      const float v = acc[j] * sc + (p.bias ? p.bias[j % p.bias_mod] : 0.f);
      dg_st(p.out, o + (long)j * p.out_sn, p.out_dtype, v);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// thin_wgrad_down: wmode 0 with Ci <= 4 (Down1: Ci = 2), Co == 64 per pass.
// block = a range of (b, m) coarse rows; thread = (co = tid & 63, ky = tid >> 6): per coarse pixel it reads its
// gradient value once and the 4 x Ci input taps of its kernel row from LDS (wave-uniform address -> broadcast).
template <int CMAX>
__global__ __launch_bounds__(256) void thin_wgrad_down_kernel(WgradP p, int co_base) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* s_a = (float*)smem;  // [4 ky][2*Wc + 2][CMAX]
  const int tid = threadIdx.x;
  const int co = tid & 63, ky = tid >> 6;
  const int Wf = 2 * p.Wc, ncol = Wf + 2;
  const long units = (long)p.B * p.Hc;
  const long u0 = units * blockIdx.x / gridDim.x, u1 = units * (blockIdx.x + 1) / gridDim.x;
  float tot[4][CMAX];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < CMAX; ++c) tot[i][c] = 0.f;
  for (long u = u0; u < u1; ++u) {
    const int b = (int)(u / p.Hc), m = (int)(u % p.Hc);
    __syncthreads();
    if (CMAX == 2 && p.Ci == 2 && p.a_dtype == DG_F32 && p.a_sc == 1 && p.a_sp == 2 && p.a_sb % 4 == 0 && ((size_t)p.a & 15) == 0) {
      // the two-channel fp32 image (Down1 in the fp32 modes): a row is 2 Wf contiguous floats - 16-byte loads of two pixels
      // instead of a scalar load with two integer divisions per element (32 per thread and row set at Wf = 1024)
      const float* A = (const float*)p.a + (long)b * p.a_sb;
      for (int i = tid; i < 4 * (Wf / 2); i += 256) {
        const int j = i % (Wf / 2), kk = i / (Wf / 2);
        int ra, rg;
        dg_wgrad1d(0, 0, m, p.Hc, kk, ra, rg);
        const float4 v = *(const float4*)(A + ((long)ra * Wf + 2 * j) * 2);
        float* d = s_a + ((long)kk * ncol + 2 * j + 1) * 2;          // (column cc lives at LDS column cc + 1: 8-byte aligned)
        *(float2*)d = make_float2(v.x, v.y);
        *(float2*)(d + 2) = make_float2(v.z, v.w);
      }
      if (tid < 8) {                                                  // the circular halo: column -1 = Wf - 1, column Wf = 0
        const int kk = tid >> 1, hi = tid & 1;
        int ra, rg;
        dg_wgrad1d(0, 0, m, p.Hc, kk, ra, rg);
        const float2 v = *(const float2*)(A + ((long)ra * Wf + (hi ? 0 : Wf - 1)) * 2);
        *(float2*)(s_a + ((long)kk * ncol + (hi ? Wf + 1 : 0)) * 2) = v;
      }
    } else
    for (int i = tid; i < 4 * ncol * p.Ci; i += 256) {
      const int c = i % p.Ci, col = (i / p.Ci) % ncol, kk = i / (p.Ci * ncol);
      int ra, rg;
      dg_wgrad1d(0, 0, m, p.Hc, kk, ra, rg);
      int cc = col - 1;
      if (cc < 0) cc += Wf; else if (cc >= Wf) cc -= Wf;
      s_a[(kk * ncol + col) * CMAX + c] =
          dg_ld(p.a, (long)b * p.a_sb + ((long)ra * Wf + cc) * p.a_sp + (long)c * p.a_sc, p.a_dtype);
    }
    __syncthreads();
    float acc[4][CMAX];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < CMAX; ++c) acc[i][c] = 0.f;
    const long gb = (long)b * p.g_sb + (long)m * p.Wc * p.g_sp + (long)(co_base + co) * p.g_sc;
    const float* row = s_a + (long)ky * ncol * CMAX;
    auto walk = [&](auto loadg) __attribute__((always_inline)) {
#pragma unroll 4
      for (int x = 0; x < p.Wc; ++x) {
        const float g = loadg(x);
        // input columns 2x-1 .. 2x+2 live at LDS columns 2x .. 2x+3
#pragma unroll
        for (int kx = 0; kx < 4; ++kx)
#pragma unroll
          for (int c = 0; c < CMAX; ++c) acc[kx][c] += g * row[(2 * x + kx) * CMAX + c];
      }
    };
    if (p.g_dtype == DG_BF16X2 && p.g_sc == 1 && p.g_sp % 64 == 0) {
      // split-bf16 gradient rows: the pixel stride is whole channel groups, so the (hi, lo) pair of this thread's channel
      // moves by a constant 2 g_sp halves per pixel (the generic dg_ld redoes the 64-bit index split per element)
      const unsigned short* gq = (const unsigned short*)p.g + dg_x2_index(gb);
      const long gs2 = 2 * p.g_sp;
      walk([&](int x) {
        const unsigned short* q = gq + (long)x * gs2;
        return __builtin_bit_cast(float, (unsigned)q[0] << 16) + __builtin_bit_cast(float, (unsigned)q[64] << 16);
      });
    } else {
      walk([&](int x) { return dg_ld(p.g, gb + (long)x * p.g_sp, p.g_dtype); });
    }
    const float rs = p.rowscale ? p.rowscale[b] : 1.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < CMAX; ++c) tot[i][c] += rs * acc[i][c];
  }
  // p.ws: the block's partial tile with plain stores (summed by dg_wgrad_reduce in a fixed order) instead of atomics on dw
  float* wsb = p.ws ? p.ws + (long)blockIdx.x * 16 * p.Ci * p.Co : nullptr;
#pragma unroll
  for (int kx = 0; kx < 4; ++kx)
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < p.Ci) {
        const long o = ((long)(ky * 4 + kx) * p.Ci + c) * p.Co + co_base + co;
        if (wsb) wsb[o] = tot[kx][c] * p.scale; else atomicAdd(&p.dw[o], tot[kx][c] * p.scale);
      }
}

// ---------------------------------------------------------------------------------------------------------
// thin_wgrad_up: wmode 1 with Co <= 4 (Head: Co = 1..3), Ci == 64 per pass.
// thread = (ci = tid & 63, ky = tid >> 6); the gradient rows (fine grid, <= 4 channels, any layout) go to LDS.
template <int NMAX>
__global__ __launch_bounds__(256) void thin_wgrad_up_kernel(WgradP p, int ci_base) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* s_g = (float*)smem;  // [2 py][2*Wc][NMAX]
  const int tid = threadIdx.x;
  const int ci = tid & 63, ky = tid >> 6;
  const int Wf = 2 * p.Wc;
  const long units = (long)p.B * p.Hc;
  const long u0 = units * blockIdx.x / gridDim.x, u1 = units * (blockIdx.x + 1) / gridDim.x;
  const int py = (ky == 0 || ky == 2) ? 1 : 0;
  float tot[4][NMAX];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < NMAX; ++c) tot[i][c] = 0.f;
  for (long u = u0; u < u1; ++u) {
    const int b = (int)(u / p.Hc), m = (int)(u % p.Hc);
    __syncthreads();
    for (int i = tid; i < 2 * Wf * p.Co; i += 256) {
      const int col = i % Wf, c = (i / Wf) % p.Co, pp = i / (Wf * p.Co);
      s_g[(pp * Wf + col) * NMAX + c] =
          dg_ld(p.g, (long)b * p.g_sb + ((long)(2 * m + pp) * Wf + col) * p.g_sp + (long)c * p.g_sc, p.g_dtype);
    }
    __syncthreads();
    int ra, rg;
    dg_wgrad1d(1, 0, m, p.Hc, ky, ra, rg);
    const long ab = (long)b * p.a_sb + (long)ra * p.Wc * p.a_sp + (long)(ci_base + ci) * p.a_sc;
    const float* grow = s_g + (long)py * Wf * NMAX;
    float acc[4][NMAX];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < NMAX; ++c) acc[i][c] = 0.f;
    // sliding window over the input row: a[x-1], a[x], a[x+1] (circular)
    auto walk = [&](auto loada) __attribute__((always_inline)) {
      float am = loada(p.Wc - 1);
      float a0 = loada(0);
#pragma unroll 8   // (measured in the fp32x3 step: 4 -> 113 us, 8 -> 95 us, 16 -> 115 us; thin_wgrad_down: 2 / 4 / 8 -> 247 / 164 / 206 us)
      for (int x = 0; x < p.Wc; ++x) {
        const int xn = x + 1 == p.Wc ? 0 : x + 1;
        const float ap = loada(xn);
        // kx=1: (px 0, a[x]); kx=3: (px 0, a[x-1]); kx=0: (px 1, a[x+1]); kx=2: (px 1, a[x])
#pragma unroll
        for (int c = 0; c < NMAX; ++c) {
          const float g0 = grow[(2 * x) * NMAX + c], g1 = grow[(2 * x + 1) * NMAX + c];
          acc[1][c] += a0 * g0;
          acc[3][c] += am * g0;
          acc[0][c] += ap * g1;
          acc[2][c] += a0 * g1;
        }
        am = a0;
        a0 = ap;
      }
    };
    if (p.a_dtype == DG_BF16X2 && p.a_sc == 1 && p.a_sp % 64 == 0) {   // (as in thin_wgrad_down: constant stride between pairs)
      const unsigned short* aq = (const unsigned short*)p.a + dg_x2_index(ab);
      const long as2 = 2 * p.a_sp;
      walk([&](int x) {
        const unsigned short* q = aq + (long)x * as2;
        return __builtin_bit_cast(float, (unsigned)q[0] << 16) + __builtin_bit_cast(float, (unsigned)q[64] << 16);
      });
    } else {
      walk([&](int x) { return dg_ld(p.a, ab + (long)x * p.a_sp, p.a_dtype); });
    }
    const float rs = p.rowscale ? p.rowscale[b] : 1.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < NMAX; ++c) tot[i][c] += rs * acc[i][c];
  }
  float* wsb = p.ws ? p.ws + (long)blockIdx.x * 16 * p.Ci * p.Co : nullptr;   // (as thin_wgrad_down)
#pragma unroll
  for (int kx = 0; kx < 4; ++kx)
#pragma unroll
    for (int c = 0; c < NMAX; ++c)
      if (c < p.Co) {
        const long o = ((long)(ky * 4 + kx) * p.Ci + ci_base + ci) * p.Co + c;
        if (wsb) wsb[o] = tot[kx][c] * p.scale; else atomicAdd(&p.dw[o], tot[kx][c] * p.scale);
      }
}

template <typename T, bool X2>
static auto smalln_fn(int n) {
  return n == 1 ? thin_smalln_kernel<T, 1, X2> : (n == 2 ? thin_smalln_kernel<T, 2, X2> : thin_smalln_kernel<T, 3, X2>);
}

int thin_conv_valu_launch(const ConvP* p, const ThinConvPick& k, hipStream_t s) {
  if (k.kernel == THIN_SMALLK) {                   // a block walks the tiles of one output row
    const auto fn = k.ta == 2 ? thin_smallk_kernel<2> : thin_smallk_kernel<4>;
    for (int nb = 0; nb < p->N; nb += 64)
      if (const int rc = thin_launch(fn, k.grid, 0, s, *p, k.tiles_x, nb)) return rc;
    return DG_OK;
  }
  if (k.lds > 64 * 1024) return DG_EUNSUPPORTED;   // (the one bound checked at launch only: the plan says THIN for such a shape)
  const auto fn = k.ta == DG_BF16 ? smalln_fn<bf16, false>(k.tb)
                                  : (k.ta == DG_BF16X2 ? smalln_fn<float, true>(k.tb) : smalln_fn<float, false>(k.tb));
  return thin_launch(fn, k.grid, k.lds, s, *p);
}

int thin_wgrad_valu_launch(const WgradP* p, const ThinWgradPick& k, hipStream_t s) {
  const auto fn = k.kernel == THIN_WGRAD_UP_VALU ? thin_wgrad_up_kernel<4>
                                                 : (k.ta == 2 ? thin_wgrad_down_kernel<2> : thin_wgrad_down_kernel<4>);
  for (int i = 0; i < k.passes; ++i)               // one pass per 64 channels of the wide side
    if (const int rc = thin_launch(fn, k.grid, k.lds, s, *p, 64 * i)) return rc;
  return DG_OK;
}
