// extern "C" dispatchers of the conv-like passes (include/dusty_gan_hip.h): one selector per pass (select_conv,
// select_wgrad) turns a `force` request into the kernel that runs; every entry point selects, then launches or describes.
#include "common.h"
#include "thin.h"

int dg_conv_direct_launch(const ConvP* p, hipStream_t stream);
int dg_lrelu_bits_launch(const ConvP* p, hipStream_t stream);
int dg_conv_mfma_launch(const ConvP* p, hipStream_t stream, int force, int fp32x3, int wg_cap, DgConvPlan* plan);
int dg_wgrad_mfma_dma_supported(const WgradP* p);
int dg_wgrad_mfma_dma_launch(const WgradP* p, int accumulate, int pairs, hipStream_t stream, DgWgradPlan* plan);
int dg_wgrad_mfma_dma_group_launch(const WgradP* items, int n, int pairs, int rounds, hipStream_t stream, DgWgradPlan* plans);
int dg_proj_stream_supported(const ConvP* p);
int dg_proj_stream_launch(const ConvP* p, hipStream_t stream, DgConvPlan* plan);
int dg_wgrad_mfma_ws_splits(const WgradP* p, int accumulate);
int dg_wgrad_direct_ws_splits(const WgradP* p);
int dg_wgrad_direct_launch(const WgradP* p, hipStream_t stream);
int dg_wgrad_mfma_launch(const WgradP* p, int accumulate, hipStream_t stream, int x3);

// `force` carries one flag bit beside the request code: DG_FORCE_FP32X3 (include/dusty_gan_hip.h) - fp32 operands through
// split-bf16 matrix instructions (mfma_common.h).  Per CALL, so two engines of different precision in one process do not
// share a setting (rounds 3-4 had a process-wide dg_set_fp32_split).
namespace {

enum ConvKernel { CONV_DIRECT, CONV_THIN, CONV_MFMA, CONV_PROJ_STREAM };

// The kernel dg_conv(p, force) runs, or the refusal.  CONV_MFMA stands for the MFMA family: dg_conv_mfma_launch takes the
// request code and picks the kernel (its auto rule needs the geometry).  plan != NULL: cleared once the arguments pass.
// The saved-mask fields: mask_out is honoured behind EVERY kernel (natively by the ping-pong conv and the thin matrix-core
// MODE_S2 kernel - DgConvPlan.mask_bits & 1 - otherwise by one packing launch over the output, conv_dispatch), mask_in only
// by kernels that take bits (the others read aux, which stays mandatory).
int select_conv(const DgConv* p, int force_flags, ConvKernel* k, ThinConvPick* thin, DgConvPlan* plan) {
  if (p && (p->mask_out || p->mask_in)) {
    if (p->mask_out && p->epi != EPI_LRELU) return DG_EINVAL;
    if (p->mask_in && p->epi != EPI_MASK) return DG_EINVAL;
    if (p->out_sn != 1 || p->N % 8 != 0 || p->out_sp % 8 != 0 || p->out_sb % 8 != 0) return DG_EUNSUPPORTED;
  }
  if (!p || !p->in || !p->out || !p->w) return DG_EINVAL;
  if (p->B <= 0 || p->K <= 0 || p->N <= 0) return DG_EINVAL;
  if (p->mode != MODE_GEMM && (p->Hc < 2 || p->Wc < 2)) return DG_EINVAL;
  if (p->epi == EPI_MASK && !p->aux) return DG_EINVAL;
  if (p->bias && p->bias_mod <= 0) return DG_EINVAL;
  if (p->dbias && p->bias_mod <= 0) return DG_EINVAL;
  if (plan) *plan = DgConvPlan{};
  const int force = force_flags & ~DG_FORCE_FP32X3;
  const bool mfma_ok = !p->nscale && dg_conv_mfma_supported(p), thin_ok = thin_conv_pick(p, thin) == DG_OK;
  const bool proj_ok = dg_proj_stream_supported(p);   // Proj forward (bf16, K = 512, B <= 32): replaces the general MFMA kernel
  bool ok = true;
  if (force == DG_FORCE_AUTO) *k = proj_ok ? CONV_PROJ_STREAM : (mfma_ok ? CONV_MFMA : (thin_ok ? CONV_THIN : CONV_DIRECT));
  else if (force == DG_FORCE_PROJ_STREAM) *k = CONV_PROJ_STREAM, ok = proj_ok;
  else if (force == DG_FORCE_MFMA || force == DG_FORCE_LOCKSTEP || force == DG_FORCE_PINGPONG ||
           force == DG_FORCE_PINGPONG_SINGLE) *k = CONV_MFMA, ok = mfma_ok;
  else if (force == DG_FORCE_THIN) *k = CONV_THIN, ok = thin_ok;
  else *k = CONV_DIRECT;
  return ok ? DG_OK : DG_EUNSUPPORTED;
}

// launch kernel k, or (plan != NULL) describe the launch
int conv_run(const DgConv* p, ConvKernel k, const ThinConvPick& thin, int force_flags, int wg_cap, hipStream_t s, DgConvPlan* plan) {
  if (k == CONV_PROJ_STREAM) return dg_proj_stream_launch(p, s, plan);
  if (k == CONV_MFMA)
    return dg_conv_mfma_launch(p, s, force_flags & ~DG_FORCE_FP32X3, (force_flags & DG_FORCE_FP32X3) ? 1 : 0, wg_cap, plan);
  if (!plan) return k == CONV_THIN ? thin_conv_launch(p, thin, s) : dg_conv_direct_launch(p, s);
  plan->family = k == CONV_THIN ? DG_CONV_FAMILY_THIN : DG_CONV_FAMILY_DIRECT;
  if (k == CONV_THIN)
    plan->thin_mfma = thin.thin_mfma, plan->mask_bits = thin.mask_bits, plan->dbias_rows = thin.dbias_rows, plan->sum_parts = thin.sum_parts;
  return DG_OK;
}

int conv_dispatch(const DgConv* p, int force_flags, int wg_cap, hipStream_t s, DgConvPlan* plan) {
  ConvKernel k;
  ThinConvPick thin;
  int rc = select_conv(p, force_flags, &k, &thin, plan);
  if (rc || plan || !p->mask_out) return rc ? rc : conv_run(p, k, thin, force_flags, wg_cap, s, plan);
  DgConvPlan pl{};
  rc = conv_run(p, k, thin, force_flags, wg_cap, nullptr, &pl);
  if (rc == DG_OK) rc = conv_run(p, k, thin, force_flags, wg_cap, s, nullptr);
  if (rc == DG_OK && !(pl.mask_bits & 1)) rc = dg_lrelu_bits_launch(p, s);
  return rc;
}

struct WgradKernel {
  int variant;      // DG_WGRAD_VARIANT_*
  int pairs;        // DG_WGRAD_VARIANT_DMA: W-tap pairs 0 by the K range, 1 always, 2 never
  int splits;       // the other kernels: partial tiles of the workspace form (0: the launch has none)
  long ws_floats;
  bool takes_gmod;  // the kernel honours DgWgrad.g_mod
  bool zero_dw;     // dg_wgrad zero-fills dw in front of it (overwrite without a workspace: the kernel only adds)
  ThinWgradPick thin;   // DG_WGRAD_VARIANT_THIN / _THIN_MFMA: the kernel and its launch
};

// The kernel dg_wgrad(p, accumulate, force) runs, or the refusal.  Whether it takes this call's `ws` / `g_mod` is for the
// launch to check: dg_wgrad_plan describes the kernel whatever they are.
int select_wgrad(const DgWgrad* p, int accumulate, int force_flags, WgradKernel* k) {
  if (!p || !p->a || !p->g || !p->dw) return DG_EINVAL;
  if (p->B <= 0 || p->Ci <= 0 || p->Co <= 0 || p->Hc <= 0 || p->Wc <= 0) return DG_EINVAL;
  const int force = force_flags & ~DG_FORCE_FP32X3;
  ThinWgradPick thin;
  const bool mfma_ok = dg_wgrad_mfma_supported(p), thin_ok = thin_wgrad_pick(p, &thin) == DG_OK;
  const bool pairs = force == DG_FORCE_WG_DMA_PAIRS || force == DG_FORCE_WG_DMA_NOPAIRS;
  *k = WgradKernel{};
  // bf16 Down / Up layers: the LDS-DMA ring version (wgrad_mfma_dma.hip), with the workspace form and the sample map of its
  // own; DG_FORCE_WG_REGSTAGED asks for the register-staged kernel instead
  if ((force == DG_FORCE_AUTO || force == DG_FORCE_MFMA || pairs) && mfma_ok && dg_wgrad_mfma_dma_supported(p)) {
    k->variant = DG_WGRAD_VARIANT_DMA, k->takes_gmod = true;
    k->pairs = force == DG_FORCE_WG_DMA_PAIRS ? 1 : (force == DG_FORCE_WG_DMA_NOPAIRS ? 2 : 0);
    return DG_OK;
  }
  if (force == DG_FORCE_AUTO)
    k->variant = mfma_ok ? DG_WGRAD_VARIANT_MFMA : (thin_ok ? DG_WGRAD_VARIANT_THIN : DG_WGRAD_VARIANT_DIRECT);
  else if (force == DG_FORCE_MFMA || force == DG_FORCE_WG_REGSTAGED) k->variant = mfma_ok ? DG_WGRAD_VARIANT_MFMA : 0;
  else if (force == DG_FORCE_THIN) k->variant = thin_ok ? DG_WGRAD_VARIANT_THIN : 0;
  else if (!pairs) k->variant = DG_WGRAD_VARIANT_DIRECT;
  if (!k->variant) return DG_EUNSUPPORTED;
  // the workspace form of the other kernels (round 6: their fp32 atomics summed in arrival order): one partial tile per
  // block of the thin kernels (Down1, Head), per K split of the register-staged MFMA kernel (the fp32 modes' fat layers)
  // and of the direct kernel (narrow nets; not under a sample map, nor when the request was some other pass's code);
  // the sample map: Down1's thin matrix-core kernel
  if (k->variant == DG_WGRAD_VARIANT_THIN) {
    if (thin.kernel == THIN_WGRAD_DOWN_MFMA || thin.kernel == THIN_WGRAD_UP_MFMA) k->variant = DG_WGRAD_VARIANT_THIN_MFMA;
    k->thin = thin, k->takes_gmod = thin.takes_gmod, k->splits = thin.splits;
  } else if (k->variant == DG_WGRAD_VARIANT_MFMA) k->splits = dg_wgrad_mfma_ws_splits(p, accumulate);
  else if ((force == DG_FORCE_AUTO || force == DG_FORCE_DIRECT) && !p->g_mod) k->splits = dg_wgrad_direct_ws_splits(p);
  k->ws_floats = k->splits * (long)(p->wmode == 2 ? 1 : 16) * p->Ci * p->Co;   // (the thin kernels: wmode 0 / 1)
  k->zero_dw = !accumulate && !p->ws && k->variant != DG_WGRAD_VARIANT_MFMA;   // (workspace form: the reduce overwrites dw)
  return DG_OK;
}

int wgrad_dispatch(const DgWgrad* p, int accumulate, int force_flags, hipStream_t s, DgWgradPlan* plan) {
  WgradKernel k;
  const int rc = select_wgrad(p, accumulate, force_flags, &k);
  if (rc == DG_EINVAL) return rc;
  if (plan) *plan = DgWgradPlan{k.variant, k.splits ? k.splits : 1, k.ws_floats, 0};   // (a refusal: variant 0)
  if (rc) return rc;
  if (k.variant == DG_WGRAD_VARIANT_DMA) return dg_wgrad_mfma_dma_launch(p, accumulate, k.pairs, s, plan);
  if (plan) return DG_OK;
  if ((p->ws && !k.splits) || (p->g_mod && !k.takes_gmod)) return DG_EUNSUPPORTED;
  if (k.variant == DG_WGRAD_VARIANT_MFMA) return dg_wgrad_mfma_launch(p, accumulate, s, (force_flags & DG_FORCE_FP32X3) ? 1 : 0);
  const int zrc = k.zero_dw ? dg_zero_f32(p->dw, (long)(p->wmode == 2 ? 1 : 16) * p->Ci * p->Co, s) : DG_OK;
  if (zrc) return zrc;
  return k.variant == DG_WGRAD_VARIANT_DIRECT ? dg_wgrad_direct_launch(p, s) : thin_wgrad_launch(p, k.thin, s);
}

// every item on the LDS-DMA kernel, as one launch
int wgrad_group_dispatch(const DgWgrad* items, int n, int force_flags, int rounds, hipStream_t stream, DgWgradPlan* plans) {
  if (!items || n < 1) return DG_EINVAL;
  WgradKernel k{};
  for (int i = 0; i < n; ++i) {
    const int rc = select_wgrad(&items[i], 1, force_flags, &k);
    if (rc || k.variant != DG_WGRAD_VARIANT_DMA) return rc ? rc : DG_EUNSUPPORTED;
  }
  return dg_wgrad_mfma_dma_group_launch(items, n, k.pairs, rounds, stream, plans);
}

}  // namespace

extern "C" {

const char* dg_version(void) { return "dusty_gan_hip 0.1 (gfx950)"; }

int dg_conv(const DgConv* p, int force, void* stream) { return conv_dispatch(p, force, 0, (hipStream_t)stream, nullptr); }
int dg_conv_ex(const DgConv* p, int force, int wg_cap, void* stream) {
  return conv_dispatch(p, force, wg_cap, (hipStream_t)stream, nullptr);
}
int dg_conv_plan(const DgConv* p, int force, int wg_cap, DgConvPlan* plan) {
  return plan ? conv_dispatch(p, force, wg_cap, nullptr, plan) : DG_EINVAL;
}

int dg_wgrad(const DgWgrad* p, int accumulate, int force, void* stream) {
  return wgrad_dispatch(p, accumulate, force, (hipStream_t)stream, nullptr);
}
int dg_wgrad_plan(const DgWgrad* p, int accumulate, int force, DgWgradPlan* plan) {
  return plan ? wgrad_dispatch(p, accumulate, force, nullptr, plan) : DG_EINVAL;
}
int dg_wgrad_group(const DgWgrad* items, int n, int force, int rounds, void* stream) {
  return wgrad_group_dispatch(items, n, force, rounds, (hipStream_t)stream, nullptr);
}
int dg_wgrad_group_plan(const DgWgrad* items, int n, int force, int rounds, DgWgradPlan* plans) {
  return plans ? wgrad_group_dispatch(items, n, force, rounds, nullptr, plans) : DG_EINVAL;
}
int dg_wgrad_kernel_variant(const DgWgrad* p, int force) {
  WgradKernel k;
  return select_wgrad(p, 1, force, &k) ? 0 : k.variant;
}
int dg_wgrad_has_sample_map(const DgWgrad* p, int force) {
  WgradKernel k;
  return select_wgrad(p, 1, force, &k) ? 0 : k.takes_gmod;
}

int dg_zero(float* p, long n, void* stream) { return p ? dg_zero_f32(p, n, (hipStream_t)stream) : DG_EINVAL; }

}  // extern "C"
