// Bandwidth-bound "thin" conv passes of the two layers with <= 4 channels on one side (Down1, Head): which kernel a
// descriptor gets and with what geometry, decided once per pass (thin.h) for the plan and the launch alike.
//
//   VALU + LDS fall-backs (fp32 mode, shapes the MFMA kernels refuse), thin_valu.hip:
//   thin_smallk, thin_smalln, thin_wgrad_down, thin_wgrad_up
//
//   bf16 on the matrix cores (what the benchmark step runs):
//   thin_s2_mfma (thin_s2_mfma.hip), thin_up_mfma + thin_up_prep (thin_up_mfma.hip),
//   thin_wgrad_down_mfma, thin_wgrad_up_mfma (thin_wgrad_mfma.hip)
#include "thin.h"

// ---------------------------------------------------------------------------------------------------------
// the family's accepted set ...
static bool conv_thin_ok(const ConvP* p) {
  if (!p->ring || p->mode == MODE_GEMM) return false;
  if (p->mode == MODE_S2)  // small K -> wide N
    return p->K <= 4 && p->N % 64 == 0 && p->Wc % SK_PX == 0 && !p->nscale && (!p->dbias || p->bias_mod >= p->N);
  // MODE_UP: wide K -> small N; weights = the T shadow [tap][n][k]; no mask / bias-grad epilogue
  // (N == 4: refused, although thin_up_mfma itself takes it)
  if (p->N > 3 || p->Wc % SN_PX != 0 || p->in_sk != 1 || p->w_sk != 1) return false;
  const int es = p->in_dtype == DG_BF16 ? 2 : 4;
  const bool x2 = p->in_dtype == DG_BF16X2;       // (split-bf16 input rows, fp32 weights and output)
  if (x2 && (p->K % 64 != 0 || p->in_sp % 64 != 0 || p->in_sb % 64 != 0 || ((size_t)p->in & 255) || p->out_dtype == DG_BF16X2)) return false;
  if ((p->K * es) % 16 != 0 || p->w_dtype != (x2 ? DG_F32 : p->in_dtype)) return false;
  return p->epi == EPI_LINEAR && !p->dbias;
}
// ... and, inside it, the shapes the two matrix-core kernels take
static bool conv_s2_mfma_ok(const ConvP* p) {
  if (p->mode != MODE_S2 || !p->ring || p->nscale) return false;
  if (p->in_dtype != DG_BF16 || p->out_dtype != DG_BF16 || p->w_dtype != DG_BF16) return false;
  if (p->N != 64 || p->K > 4 || p->Wc % 32 != 0 || p->Hc < 4) return false;
  const int cp = p->in_sp;  // padded channel count of the input tensor
  if ((cp != 2 && cp != 4) || p->K > cp || p->in_sk != 1 || p->w_sk != 1 || p->out_sn != 1 || p->out_sp != 64) return false;
  if (p->dbias && p->bias_mod != 64) return false;
  if (p->bias && p->scale == 0.f) return false;  // (the bias is the accumulators' start value bias / scale: round-4 advice)
  return p->out_sb % 64 == 0;                    // (a tile's output and its mask bits are addressed as whole 64-channel pixels)
}
static bool conv_up_mfma_ok(const ConvP* p) {
  if (p->mode != MODE_UP || !p->ring) return false;
  const bool x2 = p->in_dtype == DG_BF16X2;        // split-bf16 input, fp32 weights, fp32 / bf16 output (the fp32x3 mode)
  if (x2 ? (p->w_dtype != DG_F32 || p->out_dtype == DG_BF16X2 || p->in_sp % 64 != 0 || p->in_sb % 64 != 0 || ((size_t)p->in & 255))
         : (p->in_dtype != DG_BF16 || p->w_dtype != DG_BF16)) return false;
  if (p->K != 64 || p->N < 1 || p->N > 4 || p->Wc % TU_PX != 0 || p->Hc < 2) return false;
  if (p->in_sk != 1 || p->w_sk != 1 || p->in_sp % 8 != 0 || p->in_sb % 8 != 0) return false;
  return p->epi == EPI_LINEAR && !p->dbias;
}

int thin_conv_pick(const ConvP* p, ThinConvPick* k) {
  *k = ThinConvPick{};
  if (!conv_thin_ok(p)) return DG_EUNSUPPORTED;
  if (conv_s2_mfma_ok(p)) {
    // CP = the input's padded channel count; MB: the saved 1-bit leaky-relu masks, 1 written, 2 read instead of aux
    k->kernel = THIN_S2_MFMA, k->ta = (int)p->in_sp;
    k->tb = (p->epi == EPI_LRELU && p->mask_out) ? 1 : ((p->epi == EPI_MASK && p->mask_in) ? 2 : 0);
    k->tiles_x = p->Wc / 32, k->ntiles = (long)p->B * p->Hc * k->tiles_x;
    k->grid = (k->ntiles + 3) / 4 > thin_s2_mfma_cap ? thin_s2_mfma_cap : (k->ntiles + 3) / 4;
    k->thin_mfma = 1, k->mask_bits = 3;
    k->dbias_rows = (int)k->grid;                 // its grid = the partial rows it writes to DgConv.dbias_part
  } else if (conv_up_mfma_ok(p)) {
    k->kernel = THIN_UP_MFMA, k->ta = p->in_dtype == DG_BF16X2;
    k->tiles_x = p->Wc / TU_PX, k->nseg = (p->Hc + TU_RS - 1) / TU_RS;
    k->grid = (long)p->B * k->nseg * k->tiles_x;
    k->thin_mfma = 2;
    // its workgroups per sample = the partial sums it stores for DgConv.tanh_sum_parts, where it takes it
    if (p->N == 1 && p->out_dtype == DG_F32 && p->out_sp == 1) k->sum_parts = k->nseg * k->tiles_x;
  } else if (p->mode == MODE_S2) {
    k->kernel = THIN_SMALLK, k->ta = p->K <= 2 ? 2 : 4;
    k->tiles_x = p->Wc / SK_PX, k->grid = (long)p->B * p->Hc;
  } else {
    const int es = p->in_dtype == DG_BF16 ? 2 : 4;
    k->kernel = THIN_SMALLN, k->ta = p->in_dtype, k->tb = p->N;
    k->grid = (long)p->B * p->Hc;
    k->lds = (size_t)3 * (SN_PX + 2) * (p->K * es + 16) + (es == 2 ? (size_t)16 * p->N * p->K * 2 : 0);
  }
  return DG_OK;
}

int thin_conv_launch(const ConvP* p, const ThinConvPick& k, hipStream_t s) {
  if (k.kernel == THIN_CONV_NONE) return DG_EUNSUPPORTED;
  if (k.kernel == THIN_S2_MFMA) return thin_s2_mfma_launch(p, k, s);
  return k.kernel == THIN_UP_MFMA ? thin_up_mfma_launch(p, k, s) : thin_conv_valu_launch(p, k, s);
}

// ---------------------------------------------------------------------------------------------------------
// shapes the two matrix-core weight-gradient kernels take (Down1: 2 -> 64 channels; Head: 64 -> <= 4 channels, pixel-major
// gradient padded to 2 or 4 channels), and their LDS: the staged rows + gradient tiles, aliased by the cross-wave reduction
static bool wgrad_down_mfma_ok(const WgradP* p) {
  return p->wmode == 0 && p->a_dtype == DG_BF16 && p->g_dtype == DG_BF16 && p->Ci == 2 && p->Co == 64 && p->a_sc == 1 &&
         p->g_sc == 1 && p->a_sp == 2 && p->g_sp == 64 && p->Wc % 64 == 0 && p->Hc % WG_ROWS_PB == 0 && 2 * p->Wc <= 4096 &&
         p->a_sb % 8 == 0 && ((size_t)p->a & 15) == 0 && p->g_sb % 8 == 0 && ((size_t)p->g & 15) == 0;
}
static size_t wgrad_down_mfma_lds(const WgradP* p) {
  const size_t lds = (size_t)4 * (2 * p->Wc + 8) * 4 + 4 * 16 * 144, red = (size_t)4 * 32 * 64 * 4;
  return lds < red ? red : lds;
}
static bool wgrad_up_mfma_ok(const WgradP* p) {
  return p->wmode == 1 && p->a_dtype == DG_BF16 && p->g_dtype == DG_BF16 && p->Ci == 64 && p->a_sc == 1 &&
         p->a_sp == 64 && p->g_sc == 1 && (p->g_sp == 2 || p->g_sp == 4) && p->Co <= p->g_sp && p->g_sb % 2 == 0 &&
         p->Wc % 64 == 0 && p->Hc >= 2 && p->Hc % WGU_ROWS_PB == 0 && p->a_sb % 8 == 0 && ((size_t)p->a & 15) == 0;
}
static size_t wgrad_up_mfma_lds(const WgradP* p, int np) {
  const size_t lds = (size_t)np * 32 * (p->Wc * 2 + 16) + 4 * 16 * 144, red = (size_t)4 * np * 32 * 64 * 4;
  return lds < red ? red : lds;
}

int thin_wgrad_pick(const WgradP* p, ThinWgradPick* k) {
  *k = ThinWgradPick{};
  const size_t lds_max = 160 * 1024;
  if (!p->ring || (p->wmode == 0 ? (p->Ci > 4 || p->Co % 64 != 0) : (p->wmode != 1 || p->Co > 4 || p->Ci % 64 != 0)))
    return DG_EUNSUPPORTED;
  // the VALU kernels' staged rows bound the family's accepted set, whichever kernel runs
  const size_t valu_lds = p->wmode == 0 ? (size_t)4 * (2 * p->Wc + 2) * (p->Ci <= 2 ? 2 : 4) * sizeof(float)
                                        : (size_t)2 * 2 * p->Wc * 4 * sizeof(float);
  if (valu_lds > lds_max) return DG_EUNSUPPORTED;
  const long units = (long)p->B * p->Hc;
  long nb;                                                             // workgroups of a launch
  int np = (p->Co > 2 && p->g_sp == 4) ? 2 : 1;                        // thin_wgrad_up_mfma: channel pairs per pass ...
  if (wgrad_up_mfma_lds(p, np) > lds_max) np = 1;                      // (... very wide maps: one)
  if (wgrad_down_mfma_ok(p) && wgrad_down_mfma_lds(p) <= lds_max) {
    const int Wf = 2 * p->Wc;
    k->kernel = THIN_WGRAD_DOWN_MFMA, k->ta = Wf <= 256 ? 1 : (Wf <= 1024 ? 4 : 16), k->lds = wgrad_down_mfma_lds(p);
    // rows per block: every block ends in 2048 partial sums for the same 8 KB; 4 rows once 2 rows give >= 1024 blocks
    k->rows_pb = (units >= 2048 && p->Hc % 4 == 0) ? 4 : WG_ROWS_PB;
    k->passes = 1, nb = units / k->rows_pb;
    k->takes_gmod = true;                                              // only this kernel has the sample map
  } else if (wgrad_up_mfma_ok(p) && wgrad_up_mfma_lds(p, np) <= lds_max) {
    k->kernel = THIN_WGRAD_UP_MFMA, k->ta = np, k->lds = wgrad_up_mfma_lds(p, np);
    k->passes = np == 2 ? 1 : (p->Co + 1) / 2, nb = units / WGU_ROWS_PB;
  } else {
    k->kernel = p->wmode == 0 ? THIN_WGRAD_DOWN_VALU : THIN_WGRAD_UP_VALU, k->ta = (p->wmode == 0 && p->Ci <= 2) ? 2 : 4;
    k->lds = valu_lds, k->passes = (p->wmode == 0 ? p->Co : p->Ci) / 64, nb = units < 1024 ? units : 1024;
  }
  k->grid = (unsigned)nb;
  // The workspace form (DgWgrad.ws: plain-store partial tiles of 16 Ci Co floats, one per block, summed by dg_wgrad_reduce):
  // the matrix-core kernels' single-pass launches and the VALU kernels without a sample map
  const bool mfma = k->kernel == THIN_WGRAD_DOWN_MFMA || k->kernel == THIN_WGRAD_UP_MFMA;
  if ((mfma ? k->passes == 1 : !p->g_mod) && nb > 0 && nb <= 65536) k->splits = (int)nb;
  return DG_OK;
}

int thin_wgrad_launch(const WgradP* p, const ThinWgradPick& k, hipStream_t s) {
  if (k.kernel == THIN_WGRAD_NONE) return DG_EUNSUPPORTED;
  if ((p->ws && !k.splits) || (p->g_mod && !k.takes_gmod)) return DG_EUNSUPPORTED;   // (this call's arguments, not the shape)
  const bool mfma = k.kernel == THIN_WGRAD_DOWN_MFMA || k.kernel == THIN_WGRAD_UP_MFMA;
  return mfma ? thin_wgrad_mfma_launch(p, k, s) : thin_wgrad_valu_launch(p, k, s);
}
