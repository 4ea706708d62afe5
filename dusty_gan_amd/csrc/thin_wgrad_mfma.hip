// The matrix-core weight gradients of the thin family (bf16; picked in conv_thin.hip): thin_wgrad_down_mfma (Down1) and
// thin_wgrad_up_mfma (Head).  Their memory schedules are written out by hand (fixed-count unrolled load batches, the next
// row / group in flight in registers, nothing but the prefetch outstanding when a wait comes): hipcc does not unroll a
// staging loop with a run-time trip count.
#include "thin.h"
#include "mfma_common.h"

// ---------------------------------------------------------------------------------------------------------
// thin_wgrad_down_mfma (bf16, Ci == 2, Co == 64): Down1's weight gradient on the matrix cores.
//   dW[(ky,kx,ci) = 32][co = 64] = sum_pixels A[pixel][(ky,kx,ci)] * G[pixel][co]
// GEMM view: M = 32 (one MFMA tile), N = 64 (two tiles), K = coarse pixels.  A block owns ROWS_PB consecutive
// coarse rows of one sample; the 4 input rows a coarse row touches are staged in LDS as (ci0,ci1) dwords and each
// wave walks a quarter of the row in 16-pixel K steps: the A fragment (8 consecutive pixels of one (tap,ci)) is
// gathered from the staged rows, the G fragment comes from a wave-private [16][64] LDS tile through the
// transposing read ds_read_b64_tr_b16.  Waves are reduced through LDS, then one fp32 atomic per element per block.
#define WG_GS 4                                  // K steps (16 pixels each) whose gradient tiles a wave fetches at once

// Memory schedule (round 2; the first version made one global round trip per staged dword batch and per K step - loops
// hipcc does not unroll: load, s_waitcnt vmcnt(0), ds_write): the four input rows of a coarse row are fetched as NPT
// sixteen-byte pieces per thread, the NEXT row's pieces in flight while the current row is computed; a wave requests the
// gradient tiles of WG_GS K steps (2 x 16 B per lane each) in one batch before the row's barrier, so a row costs about one
// exposed round trip instead of ~24.  LDS row layout: pixel c at dword c + 4 (16-byte aligned pieces), the circular halo
// pixels -1 / Wf at dwords 3 / Wf + 4.  The cross-wave reduction buffer aliases the staging area (32 KB per block).
template <int NPT>
__global__ __launch_bounds__(256) void thin_wgrad_down_mfma_kernel(WgradP p, int rows_pb) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int Wf = 2 * p.Wc, ncol = Wf + 8;
  unsigned* s_a = (unsigned*)smem;                                   // [4 ky][ncol] dwords = (ci0, ci1)
  unsigned char* s_g = smem + (size_t)4 * ncol * 4;                  // [4 waves][16 px][144 B]
  float* s_red = (float*)smem;                                       // [4 waves][32][64] fp32 - after the row loop
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long units = (long)p.B * p.Hc;
  const long u0 = (long)blockIdx.x * rows_pb;
  const bf16* A = (const bf16*)p.a;
  const bf16* G = (const bf16*)p.g;
  // lane roles
  const int lr = lane & 31, lh = lane >> 5;
  const int m_ky = lr >> 3, m_kx = (lr >> 1) & 3, m_ci = lr & 1;     // A row of this lane: m = (ky*4+kx)*2+ci
  const int g16 = lane >> 4, i16 = lane & 15;
  const int kh = g16 >> 1, cb = g16 & 1, q = i16 >> 2, pp = i16 & 3; // transposing-read roles (see wgrad_mfma.hip)
  unsigned char* my_g = s_g + wave * 16 * 144;
  tw_f32x16 acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
  const int seg = p.Wc / 4;                                          // pixels per wave per row
  const int npc = Wf / 4;                                            // 16-byte pieces per staged row (4 rows: Wf pieces)
  tw_u32x4 sa[NPT];
  unsigned sh = 0;
  auto fetch_a = [&](long u) __attribute__((always_inline)) {
    const int b = (int)(u / p.Hc), Y = (int)(u % p.Hc);
    const bf16* img = A + (long)b * p.a_sb;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      const int i = tid + 256 * k;
      if (i < Wf) {
        const int kk = i / npc, pc = i % npc;
        int ra, rg;
        dg_wgrad1d(0, 0, Y, p.Hc, kk, ra, rg);
        sa[k] = *(const tw_u32x4*)(img + ((long)ra * Wf + 4 * pc) * 2);
      }
    }
    if (tid < 8) {                                                   // halo: pixel Wf - 1 in front, pixel 0 behind
      int ra, rg;
      dg_wgrad1d(0, 0, Y, p.Hc, tid >> 1, ra, rg);
      sh = *(const unsigned*)(img + ((long)ra * Wf + ((tid & 1) ? 0 : Wf - 1)) * 2);
    }
  };
  auto put_a = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      const int i = tid + 256 * k;
      if (i < Wf) *(tw_u32x4*)(s_a + (i / npc) * ncol + 4 + 4 * (i % npc)) = sa[k];
    }
    if (tid < 8) s_a[(tid >> 1) * ncol + ((tid & 1) ? Wf + 4 : 3)] = sh;
  };
  const long uend = u0 + rows_pb < units ? u0 + rows_pb : units;
  // the K steps of the block's rows in groups of WG_GS: group gq = (row u0 + gq / gpr, steps (gq % gpr) * WG_GS ...)
  const int spr = seg / 16, gpr = (spr + WG_GS - 1) / WG_GS, ngr = (int)(uend - u0) * gpr;
  auto load_group = [&](int gq, tw_u32x4 (&gt)[WG_GS][2]) __attribute__((always_inline)) {
    const long u = u0 + gq / gpr;
    const int s0 = (gq % gpr) * WG_GS;
    const int b = (int)(u / p.Hc), Y = (int)(u % p.Hc);
    const int bg = p.g_mod > 0 ? b % p.g_mod : b;                    // (one launch over real | fake | tangent input samples)
    const bf16* grow = G + (long)bg * p.g_sb + ((long)Y * p.Wc + wave * seg + 16 * s0) * p.g_sp;
    // the gradient tiles of the group's K steps: G[xb .. xb+15][0..63] (128 B per pixel) = 2 x (64 lanes x 16 B) each
#pragma unroll
    for (int st = 0; st < WG_GS; ++st)
      if (s0 + st < spr) {
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          const int c = lane + 64 * v, row = c >> 3, part = c & 7;
          gt[st][v] = *(const tw_u32x4*)(grow + (long)(16 * st + row) * p.g_sp + part * 8);
        }
      }
  };
  const bf16* s_a16 = (const bf16*)s_a;
  auto run_group = [&](int gq, const tw_u32x4 (&gt)[WG_GS][2]) __attribute__((always_inline)) {
    if (gq % gpr == 0) {                                             // first group of a row: its staged input rows
      __syncthreads();                                               // (the previous row's gathers are done)
      put_a();
      __syncthreads();
      if (u0 + gq / gpr + 1 < uend) fetch_a(u0 + gq / gpr + 1);      // in flight during this row's K steps
    }
    const int s0 = (gq % gpr) * WG_GS;
#pragma unroll
    for (int st = 0; st < WG_GS; ++st) {
      if (s0 + st >= spr) break;
      const int xb = wave * seg + 16 * (s0 + st);
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        const int c = lane + 64 * v, row = c >> 3, part = c & 7;
        *(tw_u32x4*)(my_g + row * 144 + part * 16) = gt[st][v];
      }
      // A fragment: pixels xb + 8 lh + j, j = 0..7, of this lane's (ky,kx,ci): fine column 2 x + kx - 1 -> dword + 4
      tw_bf16x8 fa;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        fa[j] = s_a16[((long)m_ky * ncol + 2 * (xb + 8 * lh + j) + m_kx + 3) * 2 + m_ci];
#pragma unroll
      for (int jt = 0; jt < 2; ++jt) {
        const unsigned char* ptr = my_g + (8 * kh + q) * 144 + (jt * 32 + 16 * cb + 4 * pp) * 2;
        const tw_bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((tw_bf16x4 __attribute__((address_space(3)))*)(ptr));
        const tw_bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((tw_bf16x4 __attribute__((address_space(3)))*)(ptr + 4 * 144));
        const tw_bf16x8 fg = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        acc[jt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fg, acc[jt], 0, 0, 0);
      }
    }
  };
  // two register sets of gradient tiles: the next group's loads are in flight while the current group computes
  tw_u32x4 gta[WG_GS][2], gtb[WG_GS][2];
  fetch_a(u0);
  load_group(0, gta);
  for (int gq = 0; gq < ngr; gq += 2) {
    if (gq + 1 < ngr) load_group(gq + 1, gtb);
    run_group(gq, gta);
    if (gq + 2 < ngr) load_group(gq + 2, gta);
    if (gq + 1 < ngr) run_group(gq + 1, gtb);
  }
  // reduce the 4 waves, then one atomic per element.  D layout: col = lane & 31 (co), row = (e&3)+8(e>>2)+4 lh (m)
  const int b0 = (int)(u0 / p.Hc);
  const float sc = p.scale * (p.rowscale ? p.rowscale[b0] : 1.f);
  __syncthreads();
#pragma unroll
  for (int jt = 0; jt < 2; ++jt)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int mrow = (e & 3) + 8 * (e >> 2) + 4 * lh;
      s_red[(wave * 32 + mrow) * 64 + jt * 32 + lr] = acc[jt][e];
    }
  __syncthreads();
  // p.ws: the block's partial tile with plain stores (summed by dg_wgrad_reduce, fixed order) instead of 2048 atomics on
  // the 8 KB every block of the launch adds into
  float* wsb = p.ws ? p.ws + (long)blockIdx.x * 2048 : nullptr;
  for (int i = tid; i < 32 * 64; i += 256) {
    const float v = s_red[i] + s_red[2048 + i] + s_red[4096 + i] + s_red[6144 + i];
    if (wsb) wsb[i] = v * sc; else atomicAdd(&p.dw[i], v * sc);
  }
}

// ---------------------------------------------------------------------------------------------------------
// thin_wgrad_up_mfma (bf16, Ci == 64, Co <= 2, gradient pixel-major [fine pixel][2]): Head's weight gradient on the
// matrix cores.   dW[(ky,kx,co) = 32][ci = 64] = sum over input pixels (r, xi) of  Bm[(ky,kx,co)][r, xi] * a[r, xi][ci]
// The sum runs over INPUT pixels, so the 64-channel operand `a` is tap-independent and is read exactly once; the tap
// structure sits in the thin operand: for input row r a block builds the 32 "im2col" rows
//     Bm[(ky,kx,co)][xi] = g[fine row 2 (r - d_ky) + par_ky][fine col 2 ((xi - d_kx) mod Wc) + par_kx][co]
// in LDS (zero where r - d_ky leaves the grid; the two reflected rows of models/ops/common.py:9-20 add their mirror
// row: r = 1 takes fine row 0 through ky = 3, r = Hc-2 takes fine row 2Hc-1 through ky = 0 - the inverse of
// dg_wgrad1d(1, ...)).  Each wave then walks its share of the row in 16-pixel K steps: Bm fragment by one
// ds_read_b128, the `a` fragment from a wave-private [16][64] tile through the transposing read.  Waves are reduced
// through LDS, then one fp32 atomic per element per block.
#define WGU_GS 4                                 // K steps (16 pixels each) whose `a` tiles a wave fetches at once
#define WGU_TB 4                                 // im2col tasks per thread whose gradient dwords are fetched at once

// Memory schedule: the `a` tiles come in groups of WGU_GS K steps, the next group's loads in flight while the current
// one is computed, and the gradient dwords of WGU_TB im2col tasks per thread are requested in one batch (the first
// version made one global round trip per K step and per task: load, s_waitcnt vmcnt(0), ds_write).
// NP = 2 (gradient padded to four channels, Co = 3 or 4: the dusty2 head): both channel pairs in one pass - the 64-channel
// operand, its staging and its transposing reads are shared by the two pairs' MFMAs (a second pass read it again: 54 + 34 us
// for the three-head gradient against 39 us for one pair).
template <int NP>
__global__ __launch_bounds__(256) void thin_wgrad_up_mfma_kernel(WgradP p, int gpair) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int TB = NP == 2 ? WGU_TB / 2 : WGU_TB;                  // (the same dwords in flight per thread)
  const int Wc = p.Wc, Wf = 2 * p.Wc;
  const int RSB = Wc * 2 + 16;                                       // im2col row stride (bytes), +16 B: bank spread
  unsigned char* s_b = smem;                                         // [NP][32 n][RSB]
  unsigned char* s_t = smem + (size_t)NP * 32 * RSB;                 // [4 waves][16 px][144 B]
  float* s_red = (float*)smem;                                       // [4 waves][NP 32][64] fp32 (aliases s_b at the end)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long u0 = (long)blockIdx.x * WGU_ROWS_PB;
  const bf16* A = (const bf16*)p.a;
  const unsigned* G = (const unsigned*)p.g + gpair;                  // one dword = channels (2 gpair, 2 gpair + 1) of a fine pixel
  const int gsd = (int)p.g_sp / 2;                                   // dwords per fine pixel (1: two channels, 2: four)
  const int lr = lane & 31, lh = lane >> 5;
  const int g16 = lane >> 4, i16 = lane & 15;
  const int kh = g16 >> 1, cb = g16 & 1, q = i16 >> 2, pp = i16 & 3; // transposing-read roles (see wgrad_mfma.hip)
  unsigned char* my_t = s_t + wave * 16 * 144;
  tw_f32x16 acc[NP][2];
#pragma unroll
  for (int pr = 0; pr < NP; ++pr)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[pr][j][e] = 0.f;
  const int nchunk = Wc / 8;
  const int b = (int)(u0 / p.Hc);
  // the K steps of the block's rows in groups of WGU_GS: a wave's step k of a row is the 16 pixels at wave * 16 + 64 k
  const int spr = Wc / 64, gpr = (spr + WGU_GS - 1) / WGU_GS, ngr = WGU_ROWS_PB * gpr;
  tw_u32x4 nxt[WGU_GS][2];
  auto load_group = [&](int gq) __attribute__((always_inline)) {
    const int r = (int)((u0 + gq / gpr) % p.Hc), s0 = (gq % gpr) * WGU_GS;
    const bf16* arow = A + (long)b * p.a_sb + (long)r * Wc * p.a_sp;
    // a[xb .. xb+15][0..63] (128 B per pixel) = 2 x (64 lanes x 16 B) per step
#pragma unroll
    for (int st = 0; st < WGU_GS; ++st)
      if (s0 + st < spr) {
        const int xb = wave * 16 + 64 * (s0 + st);
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          const int c = lane + 64 * v, row = c >> 3, part = c & 7;
          nxt[st][v] = *(const tw_u32x4*)(arow + (long)(xb + row) * p.a_sp + part * 8);
        }
      }
  };
  load_group(0);
  for (int gq = 0; gq < ngr; ++gq) {
    const int r = (int)((u0 + gq / gpr) % p.Hc), s0 = (gq % gpr) * WGU_GS;
    if (gq % gpr == 0) {
      __syncthreads();
      // ---- im2col rows of input row r: task = (tap, chunk of 8 input pixels), both co at once; TB tasks per thread
      //      and batch: all their gradient dwords are requested before the first is packed
      const unsigned* Gb = G + (long)b * (p.g_sb / 2);
      for (int tb = tid; tb < 16 * nchunk; tb += 256 * TB) {
        unsigned gv[TB][8][NP];
#pragma unroll
        for (int k = 0; k < TB; ++k) {
          const int t = tb + 256 * k;
          if (t < 16 * nchunk) {
            const int tap = t / nchunk, xi0 = (t % nchunk) * 8;
            const int ky = tap >> 2, kx = tap & 3;
            const int dky = ky == 0 ? 1 : (ky == 3 ? -1 : 0), pky = (ky == 0 || ky == 2) ? 1 : 0;
            const int dkx = kx == 0 ? 1 : (kx == 3 ? -1 : 0), pkx = (kx == 0 || kx == 2) ? 1 : 0;
            const int m = r - dky;
            int fr0 = (m >= 0 && m < p.Hc) ? 2 * m + pky : -1;           // fine row of the regular term
            if (fr0 < 0) {                                               // only the mirror term of a reflected row is left
              if (ky == 3 && r == 1) fr0 = 0;
              if (ky == 0 && r == p.Hc - 2) fr0 = 2 * p.Hc - 1;
            }
            const unsigned* g0 = Gb + (long)(fr0 < 0 ? 0 : fr0) * Wf * gsd;   // (fr0 < 0: loaded, not used)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              int x = xi0 + j - dkx;
              if (x < 0) x += Wc; else if (x >= Wc) x -= Wc;
              if (NP == 1) {
                gv[k][j][0] = g0[(2 * x + pkx) * gsd];
              } else {                                                   // (gsd == 2: the pixel's four channels in 8 bytes)
                const uint2 t2 = *(const uint2*)(g0 + (2 * x + pkx) * 2);
                gv[k][j][0] = t2.x; gv[k][j][NP - 1] = t2.y;
              }
            }
          }
        }
#pragma unroll
        for (int k = 0; k < TB; ++k) {
          const int t = tb + 256 * k;
          if (t < 16 * nchunk) {
            const int tap = t / nchunk, xi0 = (t % nchunk) * 8;
            const int ky = tap >> 2, kx = tap & 3;
            const int dky = ky == 0 ? 1 : (ky == 3 ? -1 : 0);
            const int dkx = kx == 0 ? 1 : (kx == 3 ? -1 : 0), pkx = (kx == 0 || kx == 2) ? 1 : 0;
            const int m = r - dky;
            const bool reg_ok = m >= 0 && m < p.Hc;
            int fr1 = -1;                                                // mirror term of the reflected rows
            if (ky == 3 && r == 1) fr1 = 0;
            if (ky == 0 && r == p.Hc - 2) fr1 = 2 * p.Hc - 1;
            const bool any = reg_ok || fr1 >= 0;
            if (!reg_ok) fr1 = -1;                                       // (the mirror row then IS gv)
#pragma unroll
            for (int pr = 0; pr < NP; ++pr) {
              unsigned lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};       // co0 / co1 of the pair, 8 bf16 each
              if (any) {
                const unsigned* g1 = fr1 >= 0 ? Gb + (long)fr1 * Wf * gsd + pr : nullptr;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                  unsigned v = gv[k][j][pr];
                  if (g1) {                                              // sum of two gradient rows, rounded once to bf16
                    int x = xi0 + j - dkx;
                    if (x < 0) x += Wc; else if (x >= Wc) x -= Wc;
                    const unsigned w2 = g1[(2 * x + pkx) * gsd];
                    const float s0f = __builtin_bit_cast(float, v << 16) + __builtin_bit_cast(float, w2 << 16);
                    const float s1f = __builtin_bit_cast(float, v & 0xffff0000u) + __builtin_bit_cast(float, w2 & 0xffff0000u);
                    const bf16 h0 = (bf16)s0f, h1 = (bf16)s1f;
                    v = (unsigned)__builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
                  }
                  const unsigned c0 = v & 0xffffu, c1 = v >> 16;
                  if (j & 1) { lo[j >> 1] |= c0 << 16; hi[j >> 1] |= c1 << 16; }
                  else { lo[j >> 1] = c0; hi[j >> 1] = c1; }
                }
              }
              *(uint4*)(s_b + (size_t)(pr * 32 + tap * 2 + 0) * RSB + xi0 * 2) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
              *(uint4*)(s_b + (size_t)(pr * 32 + tap * 2 + 1) * RSB + xi0 * 2) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
            }
          }
        }
      }
      __syncthreads();
    }
    tw_u32x4 cur[WGU_GS][2];
#pragma unroll
    for (int st = 0; st < WGU_GS; ++st)
#pragma unroll
      for (int v = 0; v < 2; ++v) cur[st][v] = nxt[st][v];
    if (gq + 1 < ngr) load_group(gq + 1);                            // in flight during this group's K steps
#pragma unroll
    for (int st = 0; st < WGU_GS; ++st) {
      if (s0 + st >= spr) break;
      const int xb = wave * 16 + 64 * (s0 + st);
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        const int c = lane + 64 * v, row = c >> 3, part = c & 7;
        *(tw_u32x4*)(my_t + row * 144 + part * 16) = cur[st][v];
      }
      tw_bf16x8 fa[NP];
#pragma unroll
      for (int pr = 0; pr < NP; ++pr) fa[pr] = *(const tw_bf16x8*)(s_b + (size_t)(pr * 32 + lr) * RSB + (xb + 8 * lh) * 2);
#pragma unroll
      for (int jt = 0; jt < 2; ++jt) {
        const unsigned char* ptr = my_t + (8 * kh + q) * 144 + (jt * 32 + 16 * cb + 4 * pp) * 2;
        const tw_bf16x4 l4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((tw_bf16x4 __attribute__((address_space(3)))*)(ptr));
        const tw_bf16x4 h4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((tw_bf16x4 __attribute__((address_space(3)))*)(ptr + 4 * 144));
        const tw_bf16x8 fg = __builtin_shufflevector(l4, h4, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
        for (int pr = 0; pr < NP; ++pr) acc[pr][jt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[pr], fg, acc[pr][jt], 0, 0, 0);
      }
    }
  }
  // reduce the 4 waves, then one atomic per element.  D layout: col = lane & 31 (ci), row = (e&3)+8(e>>2)+4 lh (n)
  const float sc = p.scale * (p.rowscale ? p.rowscale[b] : 1.f);
  __syncthreads();
  constexpr int WS = NP * 32 * 64;                                   // a wave's partial tile
#pragma unroll
  for (int pr = 0; pr < NP; ++pr)
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int nrow = (e & 3) + 8 * (e >> 2) + 4 * lh;
        s_red[wave * WS + (pr * 32 + nrow) * 64 + jt * 32 + lr] = acc[pr][jt][e];
      }
  __syncthreads();
  float* wsb = p.ws ? p.ws + (long)blockIdx.x * 16 * 64 * p.Co : nullptr;   // (single-pass launches only: the partial tile)
  for (int i = tid; i < WS; i += 256) {
    const int n = i >> 6, ci = i & 63, tap = (n & 31) >> 1, co = 2 * (gpair + (n >> 5)) + (n & 1);
    if (co >= p.Co) continue;
    const float v = s_red[i] + s_red[WS + i] + s_red[2 * WS + i] + s_red[3 * WS + i];
    const long o = ((long)tap * p.Ci + ci) * p.Co + co;
    if (wsb) wsb[o] = v * sc; else atomicAdd(&p.dw[o], v * sc);
  }
}

int thin_wgrad_mfma_launch(const WgradP* p, const ThinWgradPick& k, hipStream_t s) {
  if (k.kernel == THIN_WGRAD_DOWN_MFMA) {
    const auto fn = k.ta == 1 ? thin_wgrad_down_mfma_kernel<1>
                              : (k.ta == 4 ? thin_wgrad_down_mfma_kernel<4> : thin_wgrad_down_mfma_kernel<16>);
    return thin_launch(fn, k.grid, k.lds, s, *p, k.rows_pb);
  }
  // <2>: Co = 3 / 4 on the four-channel copy, both channel pairs in one pass; <1>: one pass per pair of gradient channels
  const auto fn = k.ta == 2 ? thin_wgrad_up_mfma_kernel<2> : thin_wgrad_up_mfma_kernel<1>;
  for (int gpair = 0; gpair < k.passes; ++gpair)
    if (const int rc = thin_launch(fn, k.grid, k.lds, s, *p, gpair)) return rc;
  return DG_OK;
}
