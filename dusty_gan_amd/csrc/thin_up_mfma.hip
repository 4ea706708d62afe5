// thin_up_mfma, its prep kernels and the device-global fragment tables they fill (bf16 and split-bf16; picked in conv_thin.hip).
#include "thin.h"
#include "mfma_common.h"
#include "thin_up_frag.h"

// ---------------------------------------------------------------------------------------------------------
// thin_up_mfma (bf16 in, K = 64 input channels -> N <= 4 output channels, MODE_UP): Head forward and Down1
// backward-data on the matrix cores (models/gans/dcgan_eqlr.py:29-47 Head, :75-82 Down's input gradient).
// One coarse input pixel produces 2 x 2 fine outputs x N channels = at most 16 values, each a dot product over a
// subset of the 3 x 3 input neighbourhood x 64 channels.  That is a GEMM with
//   M' = 16 rows (py, n, px),   K = (row offset dr, column offset dc, ci) = 9 x 64,   N' = coarse pixels,
// run as v_mfma_f32_16x16x32_bf16 (18 per 16 pixels).  The weight operand - zero where a parity does not use a
// neighbour, summed where the reflected rows of models/ops/common.py:9-20 fold two taps onto one source row,
// adjoint extras included - only depends on the boundary class of the image row (interior / first / last): a prep
// launch builds the 3 x 18 fragments from dg_tap1d into a device-global table and every wave keeps its class's 18
// fragments in 72 VGPRs.  The activation rows m-1, m, m+1 of a 64-pixel tile are staged in LDS with full-line
// loads (the layout thin_smalln uses) and read back as B fragments, one ds_read_b128 per MFMA.
// Output row m' = (py * N + n) * 2 + px, so a lane's accumulator pairs are the two column parities of one output
// row: planar fp32 outputs are written as float2, 128 contiguous bytes per 16 lanes.
// The table is one per device: launches that use it must be ordered on one stream (they are: the step is one stream).
__device__ __attribute__((aligned(16))) unsigned char g_up_frag[UP_FRAG_BYTES];  // [class][frag][64 lanes][16 B]
__device__ __attribute__((aligned(16))) unsigned char g_up_frag_lo[UP_FRAG_BYTES];   // (X2: the lo halves of the folded fp32 weights)

// class 0 interior (built at m = 1), 1 first row, 2 last row (thin_up_frag.h)
__global__ __launch_bounds__(256) void thin_up_prep_kernel(ConvP p) {
  const bf16* w = (const bf16*)p.w;
  up_frag_element(blockIdx.y, blockIdx.x * 256 + threadIdx.x, p.N, p.Hc, p.adj,
                  [&](int tap, int n, int ci) { return (float)w[(long)tap * p.w_st + (long)n * p.w_sn + ci]; }, g_up_frag);
}
// X2 (fp32 weights, split-bf16 input): both tables, blockIdx.z = 0 hi / 1 lo
__global__ __launch_bounds__(256) void thin_up_prep_x2_kernel(ConvP p) {
  const float* w = (const float*)p.w;
  auto ld = [&](int tap, int n, int ci) { return w[(long)tap * p.w_st + (long)n * p.w_sn + ci]; };
  if (blockIdx.z == 0) up_frag_element<false>(blockIdx.y, blockIdx.x * 256 + threadIdx.x, p.N, p.Hc, p.adj, ld, g_up_frag);
  else up_frag_element<true>(blockIdx.y, blockIdx.x * 256 + threadIdx.x, p.N, p.Hc, p.adj, ld, g_up_frag_lo);
}

// One block = (sample, segment of TU_RS image rows, 64-pixel column tile) and walks DOWN its rows with a ring of four
// staged input rows in LDS: output row m reads rows m-1, m, m+1 from the ring while row m+2 is in flight in registers
// (3 sixteen-byte pieces per thread) and is written into the slot nobody reads - ONE barrier per row, every input row
// fetched once per segment (10 rows for 8) instead of three times, and everything the epilogue needs from global memory
// (scale, bias) fetched once in front of the loop.  The first version - one block per image row, all three rows staged
// per tile - made one round trip to memory PER PIECE (a loop the compiler did not unroll: load, s_waitcnt vmcnt(0),
// ds_write) plus two per epilogue, ~5 us per tile; pipelining that design took it from 40 to 30 us, and it stayed bound
// by the 3x re-read.
// X2 (round 5, the fp32x3 mode's Head forward / Down1 backward-data): the input is DG_BF16X2 (a pixel = 128 bytes of hi + 128 bytes
// of lo), the weights fp32: rows are staged with both halves, the weight fragments exist twice (hi / lo of the folded fp32
// weights, thin_up_prep_x2_kernel) and every k-step is three matrix instructions, w_hi x_hi + w_hi x_lo + w_lo x_hi.
template <bool X2>
__global__ __launch_bounds__(256) void thin_up_mfma_kernel(ConvP p, int tiles_x, int nseg) {
  constexpr int PPP = X2 ? 16 : 8;                                   // 16-byte pieces per pixel
  constexpr int RB = PPP * 16 + 16;                                  // LDS pixel stride: the pixel's bytes + 16 B
  constexpr int RPX = TU_PX + 2, ROWB = RPX * RB;                    // a staged row: the tile's pixels + halo
  constexpr int NLD = (RPX * PPP + 255) / 256;                       // 16-byte pieces per thread and row (the last partial)
  __shared__ __attribute__((aligned(16))) unsigned char s_in[4 * ROWB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = p.N, Wc = p.Wc, Hc = p.Hc;
  // XCD-aware, bijective block remap (blocks id and id+8 share an XCD): the column tiles and row segments of one sample
  // - which share halo columns / rows - land on ONE XCD's L2
  const int nwg = gridDim.x, id = blockIdx.x;
  const int q8 = nwg >> 3, r8 = nwg & 7, xcd = id & 7;
  const int logical = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (id >> 3);
  const int xt = logical % tiles_x, sg = (logical / tiles_x) % nseg, b = logical / (tiles_x * nseg);
  const int m0 = sg * TU_RS, m1 = m0 + TU_RS < Hc ? m0 + TU_RS : Hc;
  const char* in = (const char*)p.in + (long)b * p.in_sb * (X2 ? 4 : 2);
  const int col = lane & 15, kg = lane >> 4;
  const unsigned spb = (unsigned)p.in_sp * (X2 ? 4u : 2u);           // bytes per pixel
  unsigned goff[NLD], loff[NLD];                                     // piece u of a row: pixel tid / PPP + (256 / PPP) u, piece tid % PPP
#pragma unroll
  for (int u = 0; u < NLD; ++u) {
    const int px = tid / PPP + (256 / PPP) * u;
    int cc = xt * TU_PX - 1 + px;
    if (cc < 0) cc += Wc; else if (cc >= Wc) cc -= Wc;
    goff[u] = (unsigned)cc * spb + (tid % PPP) * 16;
    loff[u] = px * RB + (tid % PPP) * 16;
  }
  const bool last_ok = tid / PPP + (256 / PPP) * (NLD - 1) < RPX;
  auto fetch_row = [&](int r, tw_u32x4 (&st)[NLD]) __attribute__((always_inline)) {
    r = r < 0 ? 0 : (r >= Hc ? Hc - 1 : r);                          // rows outside the grid carry zero weights
    const char* row = in + (unsigned)(r * Wc) * spb;
#pragma unroll
    for (int u = 0; u < NLD; ++u)
      if (u < NLD - 1 || last_ok) st[u] = *(const tw_u32x4*)(row + goff[u]);
  };
  auto put_row = [&](int r, const tw_u32x4 (&st)[NLD]) __attribute__((always_inline)) {   // row r lives in slot (r + 1) & 3
    unsigned char* dst = s_in + ((r + 1) & 3) * ROWB;
#pragma unroll
    for (int u = 0; u < NLD; ++u)
      if (u < NLD - 1 || last_ok) *(tw_u32x4*)(dst + loff[u]) = st[u];
  };
  tw_u32x4 st[NLD];
  {
    tw_u32x4 sa[NLD], sb[NLD];
    fetch_row(m0 - 1, sa); fetch_row(m0, sb); fetch_row(m0 + 1, st);   // first: the block's longest round trip
    put_row(m0 - 1, sa); put_row(m0, sb); put_row(m0 + 1, st);
  }
  // epilogue constants of this lane's two output rows q = 2 kg + h  (q = py * N + n)
  float e_sc[2], e_bias[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int q = 2 * kg + h, n = q < 2 * N ? q % N : 0;
    e_sc[h] = p.nscale ? p.scale * p.nscale[n] : p.scale;
    e_bias[h] = p.bias ? p.bias[n % p.bias_mod] : 0.f;
  }
  const bool tsum = p.tanh_sum_parts != nullptr;                     // (DgConv.tanh_sum_parts: launcher-checked N == 1, fp32 out)
  float lsum = 0.f;
  int cls = -1;
  tw_bf16x8 fa[18], fal[X2 ? 18 : 1];
  // the caller's fragments (kept current with its shadows) or the ones thin_up_prep_kernel has just built
  const unsigned char* frags = (p.up_frag && !X2) ? (const unsigned char*)p.up_frag : g_up_frag;
  __syncthreads();
  const int xl = wave * 16 + col;                                    // this lane's pixel inside the tile
  const int x = xt * TU_PX + xl;
  for (int m = m0; m < m1; ++m) {
    const bool more = m + 1 < m1;
    if (more) fetch_row(m + 2, st);                                  // in flight during the MFMAs and stores below
    const int mcls = m == 0 ? 1 : (m == Hc - 1 ? 2 : 0);             // boundary class of the row: its weight fragments
    if (mcls != cls) {                                               // (block-uniform; at most twice per block)
      cls = mcls;
#pragma unroll
      for (int f = 0; f < 18; ++f) fa[f] = *(const tw_bf16x8*)(frags + ((cls * 18 + f) * 64 + lane) * 16);
      if constexpr (X2) {
#pragma unroll
        for (int f = 0; f < 18; ++f) fal[f] = *(const tw_bf16x8*)(g_up_frag_lo + ((cls * 18 + f) * 64 + lane) * 16);
      }
    }
    tw_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
      const unsigned char* rowp = s_in + ((m + rr) & 3) * ROWB + xl * RB + kg * 16;   // row m - 1 + rr
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const tw_bf16x8 b0 = *(const tw_bf16x8*)(rowp + d * RB);
        const tw_bf16x8 b1 = *(const tw_bf16x8*)(rowp + d * RB + 64);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[(rr * 3 + d) * 2 + 0], b0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[(rr * 3 + d) * 2 + 1], b1, acc, 0, 0, 0);
        if constexpr (X2) {
          const tw_bf16x8 l0 = *(const tw_bf16x8*)(rowp + d * RB + 128);
          const tw_bf16x8 l1 = *(const tw_bf16x8*)(rowp + d * RB + 192);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[(rr * 3 + d) * 2 + 0], l0, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[(rr * 3 + d) * 2 + 1], l1, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fal[(rr * 3 + d) * 2 + 0], b0, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fal[(rr * 3 + d) * 2 + 1], b1, acc, 0, 0, 0);
        }
      }
    }
    // D: column = pixel (lane & 15), rows 4 kg + j  ->  m' = 4 kg + j = (py * N + n) * 2 + px
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int q = 2 * kg + h;
      if (q >= 2 * N) continue;
      const int py = q / N, n = q % N;
      float v0 = acc[2 * h] * e_sc[h] + e_bias[h], v1 = acc[2 * h + 1] * e_sc[h] + e_bias[h];
      if (tsum) { v0 = dg_tanh(v0); v1 = dg_tanh(v1); lsum += v0 + v1; }   // the depth head: tanh + the image's sum (N == 1)
      const long o = (long)b * p.out_sb + ((long)(2 * m + py) * (2 * Wc) + 2 * x) * p.out_sp + (long)n * p.out_sn;
      if (p.out_dtype == DG_F32 && p.out_sp == 1) {
        *(float2*)((float*)p.out + o) = make_float2(v0, v1);
      } else {
        dg_st(p.out, o, p.out_dtype, v0);
        dg_st(p.out, o + p.out_sp, p.out_dtype, v1);
      }
    }
    if (more) put_row(m + 2, st);                                    // slot (m + 3) & 3 = the slot of row m - 2: not read this step
    __syncthreads();                                                 // row m + 2 visible; row m - 1's slot free for row m + 3
  }
  if (tsum) {                                                        // this workgroup's share of sample b's image sum: stored, not
    const float t = dg_block_sum(lsum, (float*)s_in);                // added (a fixed order at the reader: bit-reproducible)
    if (tid == 0) p.tanh_sum_parts[logical] = t;
  }
}

// the checks of this CALL's arguments (the shape passed the pick), then the prep launch unless the caller brings fragments
int thin_up_mfma_launch(const ConvP* p, const ThinConvPick& k, hipStream_t s) {
  if (p->tanh_sum_parts && !k.sum_parts) return DG_EINVAL;
  if (p->up_frag && ((size_t)p->up_frag & 15)) return DG_EINVAL;
  if (k.grid >= (1L << 31)) return DG_EUNSUPPORTED;
  if (k.ta) thin_up_prep_x2_kernel<<<dim3(UP_FRAG_BLOCKS, 3, 2), 256, 0, s>>>(*p);
  else if (!p->up_frag) thin_up_prep_kernel<<<dim3(UP_FRAG_BLOCKS, 3), 256, 0, s>>>(*p);
  // (a column-walker variant with an LDS-DMA row ring that fetched every input row once instead of three times measured
  //  within noise of this kernel on the step - 0.277 vs 0.282 ms for the family - and was removed in round 2)
  return thin_launch(k.ta ? thin_up_mfma_kernel<true> : thin_up_mfma_kernel<false>, k.grid, 0, s, *p, k.tiles_x, k.nseg);
}
