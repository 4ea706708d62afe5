/* dusty_gan_hip.h -- C ABI of libdustygan_hip.so (MI355X / gfx950 only).
 *
 * The drop-in boundary of the dusty-gan training hot path.  The reference (kazuto1011/dusty-gan) has no native
 * code on this path: every entry point below replaces a PyTorch module call (or its autograd backward) that the
 * reference's `Trainer.step` (trainers/dcgan_amp.py:162-325) makes.  The file:line next to each declaration is the
 * reference interface it replaces.  A maintainer binds these with ctypes; PyTorch is only the
 * owner of device memory and streams.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; nothing is allocated inside the library,
 *     workspaces are caller-owned; `stream` is a hipStream_t passed as void*;
 *   - return value: DG_OK (0) or a DG_E* code; kernels are launched asynchronously on `stream`;
 *   - images are fp32 [B,1,H,W]; feature maps are pixel-major/channel-minor ("NHWC") in `dtype` (DG_F32|DG_BF16);
 *   - conv weights: engine master fp32 [ky][kx][ci][co] ("cico"); the reference's (Cout,Cin,4,4) / (Cin,Cout,4,4)
 *     parameter tensors are strided VIEWS of that storage (no copy), so state_dict()/checkpoints keep the
 *     reference's shapes.
 */
#ifndef DUSTY_GAN_HIP_H
#define DUSTY_GAN_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DG_OK 0
#define DG_EINVAL 1
#define DG_EUNSUPPORTED 2
#define DG_EHIP 3

#define DG_F32 0
#define DG_BF16 1
/* DG_BF16X2 (round 5, the storage form of the "fp32x3" precision mode on the bf16 kernels): every element x is the PAIR
 * hi = bf16(x), lo = bf16(x - hi) (16 mantissa bits kept), 4 bytes per element like DG_F32 and addressed with the same element
 * strides, laid out per 64 channels as 128 bytes of hi followed by 128 bytes of lo: element i (flat element offset from a
 * 256-byte aligned base, channel-minor, channel count a multiple of 64) has hi at bf16 index 2 i - i % 64 and lo 64 further.
 * A matrix-core kernel then contracts x . w as x_hi w_hi + x_lo w_hi + x_hi w_lo with the bf16 kernels' own 128-byte channel
 * chunks (three K steps per real one) - no splitting in registers, no fp32 staging.  Taken by: the ping-pong conv (in, w, out,
 * aux all DG_BF16X2), the LDS-DMA weight-gradient kernel (a and g), the direct and the thin VALU kernels (any operand),
 * dg_cast / dg_uncast.  Everything else answers DG_EUNSUPPORTED. */
#define DG_BF16X2 2

/* conv-like op geometry: a COARSE grid Hc x Wc and a FINE grid 2Hc x 2Wc */
#define DG_MODE_S2 0   /* out on coarse, in on fine : Down forward, Up backward-data          */
#define DG_MODE_UP 1   /* out on fine, in on coarse : Up/Head forward, Down backward-data     */
#define DG_MODE_GEMM 2 /* plain rows (Proj)                                                   */

#define DG_EPI_LINEAR 0 /* out = scale*acc + bias                                             */
#define DG_EPI_LRELU 1  /* FusedLeakyReLU: leaky_relu(scale*acc + bias, 0.2) * sqrt(2)        */
#define DG_EPI_MASK 2   /* out = scale*acc * lrelu'(aux) * sqrt(2)  (backward / R1 tangent)   */

/* Parameter block of dg_conv.  Strides are in ELEMENTS. */
typedef struct DgConv {
  int mode, adj, ring;       /* adj: 0 = the reference's Pad (reflect rows, circular|reflect cols), 1 = its adjoint */
  int B, Hc, Wc;
  int K, N;                  /* contraction channels, output channels */
  const void* in;
  long in_sb, in_sp, in_sk;  /* batch, pixel (row*W+col), channel */
  void* out;
  long out_sb, out_sp, out_sn;
  const void* w;
  long w_st, w_sk, w_sn;     /* tap (ky*4+kx), k, n */
  float scale;               /* EqualLR runtime scale, models/ops/common.py:124-125,133 */
  int epi;
  const float* bias;         /* fp32 [bias_mod] or NULL; index n % bias_mod */
  int bias_mod;
  const void* aux;           /* DG_EPI_MASK: saved activation with out's layout/dtype */
  float* dbias;              /* optional: dbias[n % bias_mod] += rowscale[b] * sum_pixels out */
  const float* rowscale;     /* optional per-sample weight of the dbias sum */
  int in_dtype, out_dtype, w_dtype;
  const float* nscale;       /* optional per-output-channel scale (Head: one EqualLR scale per head) */
  const void* up_frag;       /* optional, 16-byte aligned, DG_UP_FRAG_BYTES: the weight fragments of the thin matrix-core
                              * MODE_UP kernel (Head forward, Down1 backward-data) kept current by the caller with
                              * dg_transpose_shadow_multi_frags; NULL: built by a launch in front of the kernel */
  float* dbias_ws;           /* optional scratch of DG_DBIAS_SLOTS x DG_DBIAS_SLOT_FLOATS floats, zero on entry and left zero:
                              * per-slot staging of the bias-gradient rows of the thin matrix-core MODE_S2 kernel (hundreds of
                              * atomic rows on the same two lines serialise memory-side) and, since round 6, the
                              * cross-workgroup staging of the direct and one-tile MFMA kernels' bias-gradient sums - two 64-bit
                              * fixed-point words per channel + a ticket, bias_mod <= 8191 - which makes those sums independent
                              * of the arrival order (without it they are float atomics); other kernels ignore it.  One launch
                              * at a time per scratch: launches of one stream may share it */
  /* Saved leaky-relu masks, 1 bit per element (models/ops/common.py:99-106 under autograd saves the sign of the
   * pre-activation; the backward / R1 tangent passes only ever need that sign).  Bit e of a mask buffer belongs to the
   * element at offset e of the tensor it describes (bit e % 8 of byte e / 8): the mask of `out` is indexed like `out`, the
   * mask of `aux` like `aux`.  Needs out_sn == 1 and N, out_sp, out_sb multiples of 8 (16 for the matrix-core kernels). */
  float* dbias_part;         /* optional, with dbias (round 5, bit-reproducible bias gradients): kernels that take it
                              * (DgConvPlan.dbias_rows > 0: the ping-pong conv, the thin matrix-core MODE_S2 kernel, the lock-step
                              * persistent conv at fp32) store ONE
                              * partial row of N floats per workgroup at dbias_part + row * N - summed inside the workgroup in a
                              * fixed order - and add nothing to dbias; the caller sums the rows with
                              * dg_wgrad_reduce(ws = dbias_part, dw = dbias, numel = N, splits = dbias_rows).  Kernels that do
                              * not take it ignore it and add onto dbias with atomics as before.  The rows are NOT folded:
                              * row element n is the sum for output channel n, so the form needs bias_mod == N - the kernels that take
                              * rows refuse (DG_EUNSUPPORTED) a dbias launch with bias_mod < N, with or without dbias_part. */
  void* mask_out;            /* optional, DG_EPI_LRELU: also store bit = (out element > 0) for every element written.  The
                              * ping-pong conv and the thin matrix-core MODE_S2 kernel write it from their epilogues, behind any
                              * other kernel the library adds one packing launch: the bits are there when dg_conv returns OK */
  const void* mask_in;       /* optional, DG_EPI_MASK: the bits of `aux` (written through mask_out by the launch that produced
                              * aux); kernels that take bits (DgConvPlan.mask_bits & 2) read 1/16 of the bytes, the others use aux,
                              * which stays mandatory */
  float* tanh_sum_parts;     /* optional (round 6), the thin matrix-core MODE_UP kernel only (DgConvPlan.sum_parts > 0: N == 1,
                              * DG_EPI_LINEAR, fp32 output - the depth head, models/gans/dcgan_eqlr.py:29-46): the launch writes
                              * tanh(out) instead of out (Generator.forward's torch.tanh, :71) and every workgroup STORES the sum
                              * of what it wrote at tanh_sum_parts[its index]; sample b's workgroups are the sum_parts indices
                              * from b * sum_parts: the per-sample sums DiffAugment's contrast needs (DgAugSet.xsum_parts), made
                              * where the image is made - no head post-processing launch for the baseline generator.  Kernels
                              * that do not take it (sum_parts == 0) ignore it: the caller then runs dg_head_post_fwd[_sum]. */
} DgConv;
#define DG_UP_FRAG_BYTES (3 * 18 * 1024)
#define DG_DBIAS_SLOTS 32
#define DG_DBIAS_SLOT_FLOATS 1024

/* Parameter block of dg_wgrad:  dw[tap][ci][co] += scale * sum_b rowscale[b] * sum_pixels a[..][ci] * g[..][co] */
typedef struct DgWgrad {
  int wmode, ring;           /* 0 = Down, 1 = Up/Head, 2 = plain rows (Proj: set B=1,Hc=1,Wc=batch) */
  int B, Hc, Wc;
  int Ci, Co;
  const void* a;             /* the layer's forward input */
  long a_sb, a_sp, a_sc;
  const void* g;             /* gradient w.r.t. the layer's pre-activation output */
  long g_sb, g_sp, g_sc;
  float* dw;                 /* fp32 [tap][Ci][Co] */
  float scale;
  const float* rowscale;     /* optional [B] */
  int a_dtype, g_dtype;
  /* Optional (zero = off).  ws: caller-owned workspace for the split-K partial tiles of the MFMA LDS-DMA kernel: split s
   * stores its [16][Ci][Co] partial at ws + s * 16 Ci Co with plain stores and NOTHING is added to dw - the caller sums
   * the partials with dg_wgrad_reduce (sizes from dg_wgrad_plan).  Without it the partial tiles meet in dw through fp32
   * atomics, which the memory side executes at ~1.3 TB/s against ~6 TB/s for stores (8x the bytes of dw per launch) - and in
   * arrival order.  Since round 6 every kernel that splits the reduction over workgroups has the form (the thin kernels, the
   * register-staged MFMA kernel of the fp32 modes, the direct kernel: numel = Ci Co for wmode 2); dg_wgrad_plan says which
   * launch takes it (splits > 1), a workspace handed to a launch that does not is DG_EUNSUPPORTED.
   * g_mod: the gradient's sample index is b % g_mod, so ONE launch over 3B input samples (real | fake | R1 tangent) can
   * pair the tangent rows with the real batch's gradient chain again (trainers/dcgan_amp.py:229-235). */
  float* ws;
  int g_mod;
} DgWgrad;

/* ---- conv-like passes ------------------------------------------------------------------------------------
 * dg_conv replaces, depending on (mode, adj, epi):
 *   Down.forward            models/gans/dcgan_eqlr.py:75-82  (Pad :77 + EqualLR(Conv2d 4,2,0) :80 + FusedLeakyReLU :81)
 *   Up.forward              models/gans/dcgan_eqlr.py:19-26  (Pad + EqualLR(ConvTranspose2d 4,2,3) + FusedLeakyReLU)
 *   Head.forward            models/gans/dcgan_eqlr.py:29-46
 *   Proj.forward            models/gans/dcgan_eqlr.py:6-16
 *   their autograd backward-data passes (loss.backward() at trainers/dcgan_amp.py:235,309 and
 *   torch.autograd.grad(create_graph=True) at :218-223), and the R1 tangent pass (double backward, :229-235).
 * `force` (dg_conv* and dg_wgrad*) is a request code: a forced kernel that does not take the shape answers DG_EUNSUPPORTED
 * (parity tests run each family on small problems); any other code runs the direct kernel (dg_wgrad_group refuses it). */
int dg_conv(const DgConv* p, int force, void* stream);
#define DG_FORCE_AUTO 0             /* both: pick (Proj stream -> MFMA family -> thin for <=4-channel sides -> direct)  */
#define DG_FORCE_DIRECT 1           /* both: the general direct kernel                                               */
#define DG_FORCE_MFMA 2             /* conv: the MFMA family's auto rule; wgrad: LDS-DMA where it fits, else REGSTAGED */
#define DG_FORCE_THIN 3             /* both: the thin LDS/VALU or matrix-core kernels of <=4-channel sides           */
#define DG_FORCE_LOCKSTEP 4         /* conv: the lock-step persistent large-tile MFMA kernel                         */
#define DG_FORCE_PINGPONG 5         /* conv: the ping-pong persistent MFMA kernel (bf16 / DG_BF16X2)                  */
#define DG_FORCE_WG_REGSTAGED 6     /* wgrad: the register-staged MFMA kernel                                        */
#define DG_FORCE_WG_DMA_PAIRS 7     /* wgrad: the LDS-DMA kernel with W-tap pairs                                    */
#define DG_FORCE_WG_DMA_NOPAIRS 8   /* wgrad: the LDS-DMA kernel without W-tap pairs                                 */
#define DG_FORCE_PINGPONG_SINGLE 9  /* conv: the ping-pong kernel without its both-parities tile (64-channel MODE_UP) */
#define DG_FORCE_PROJ_STREAM 10     /* conv: the weight-streaming Proj forward                                       */
/* "fp32x3" (precision contract: fp32 storage with fp32 or split-bf16 x 3 MFMA): a flag bit in the
 * `force` argument of dg_conv / dg_conv_ex / dg_conv_plan / dg_wgrad / dg_wgrad_plan, OR-ed onto the request code, for
 * DG_F32 operands on the matrix-core kernels.  Clear (default): exact fp32 products (v_mfma_f32_32x32x2_f32, 1/16 of the bf16
 * rate); set: every operand is split into bf16 hi + lo in registers and a product is a_hi b_hi + a_lo b_hi + a_hi b_lo on
 * the bf16 matrix instructions with fp32 accumulation (relative error ~2^-16 per product; the mode autocast-free fp32
 * training of trainers/dcgan_amp.py would want on this hardware).  Per call - nothing process-wide: two engines of
 * different precision in one process do not share a setting. */
#define DG_FORCE_FP32X3 0x100
/* What a dg_conv call launches (introspection for the parity tests and the benchmark: which kernel family / tile ran,
 * and how many tiles each persistent workgroup walks): DgConvPlan.family is one of */
#define DG_CONV_FAMILY_DIRECT 1       /* the direct kernel                                                   */
#define DG_CONV_FAMILY_MFMA 2         /* one-tile-per-workgroup MFMA                                         */
#define DG_CONV_FAMILY_THIN 3         /* thin (DgConvPlan.thin_mfma: which one)                              */
#define DG_CONV_FAMILY_LOCKSTEP 4     /* persistent large-tile MFMA, lock step (fp32, small layers)          */
#define DG_CONV_FAMILY_PINGPONG 5     /* persistent ping-pong MFMA (bf16 fat layers)                         */
#define DG_CONV_FAMILY_PROJ_STREAM 6  /* weight-streaming Proj forward (bf16 DG_MODE_GEMM, K = 512, B <= 32)  */
/* dg_conv_ex = dg_conv with a cap on the persistent kernel's workgroup count (wg_cap <= 0: one residency wave of the
 * device); dg_conv_plan fills `plan` for the same arguments and launches nothing. */
typedef struct DgConvPlan {
  int family;        /* DG_CONV_FAMILY_* */
  int bm, bn;        /* output tile (pixels x channels), 0 for the non-MFMA kernels */
  int tiles;         /* tiles of the launch */
  int workgroups;    /* grid size */
  int tiles_per_wg;  /* most tiles any workgroup walks */
  int thin_mfma;     /* DG_CONV_FAMILY_THIN: 1 = thin_s2_mfma, 2 = thin_up_mfma (matrix cores), 0 = the VALU kernels */
  int mask_bits;     /* 1: the kernel writes DgConv.mask_out itself (else a packing launch follows it), 2: it reads mask_in */
  int dbias_rows;    /* > 0: the kernel takes DgConv.dbias_part and writes this many partial rows of N floats; 0: it does not */
  int sum_parts;     /* > 0: the kernel takes DgConv.tanh_sum_parts and stores this many partial sums per sample; 0: it does not */
} DgConvPlan;
int dg_conv_ex(const DgConv* p, int force, int wg_cap, void* stream);
int dg_conv_plan(const DgConv* p, int force, int wg_cap, DgConvPlan* plan);
int dg_conv_mfma_supported(const DgConv* p);

/* dg_wgrad replaces the weight-gradient half of the same autograd calls.  accumulate: 1 = atomically add onto dw
 * (dw zeroed by the caller at step start: optim.zero_grad, trainers/dcgan_amp.py:177,246), 0 = overwrite. */
int dg_wgrad(const DgWgrad* p, int accumulate, int force, void* stream);
/* What dg_wgrad launches for these arguments, and the split-K workspace it can use: `splits` partial tiles of
 * 16 Ci Co floats (ws_floats = splits * 16 Ci Co; 0 when the kernel that runs has no workspace form).  The plan describes
 * the kernel: dg_wgrad alone refuses a `ws` or `g_mod` that kernel does not take.  DgWgradPlan.variant is one of */
#define DG_WGRAD_VARIANT_DIRECT 1     /* the direct kernel                                             */
#define DG_WGRAD_VARIANT_MFMA 2       /* register-staged MFMA (the fp32 modes' fat layers, Proj)        */
#define DG_WGRAD_VARIANT_THIN 3       /* thin (VALU)                                                    */
#define DG_WGRAD_VARIANT_DMA 5        /* MFMA on the LDS-DMA ring (bf16 / DG_BF16X2 Down and Up layers) */
#define DG_WGRAD_VARIANT_THIN_MFMA 7  /* thin on the matrix cores (bf16 Down1 / Head)                   */
typedef struct DgWgradPlan {
  int variant;      /* DG_WGRAD_VARIANT_*, 0 when `force` has no kernel for the shape */
  int splits;
  long ws_floats;
  int tap_pairs;    /* 1: one workgroup computes the W taps (kx, kx + 2) from one staged image */
} DgWgradPlan;
int dg_wgrad_plan(const DgWgrad* p, int accumulate, int force, DgWgradPlan* plan);
/* Up to 4 weight-gradient GEMMs as ONE launch (the layers of one network: independent of each other, all reading finished
 * activations and gradient chains - loss.backward() at trainers/dcgan_amp.py:235,309 produces them in one sweep too): every
 * item must run on the MFMA LDS-DMA kernel (dg_wgrad_plan: DG_WGRAD_VARIANT_DMA) and bring its split-K workspace `ws`, sized by
 * dg_wgrad_group_plan for the same (items, force, rounds).  One grid instead of n residency rounds: the ring fill and the
 * partial-tile stores of one layer's workgroups run under the matrix work of its neighbours'.  rounds > 0: the group as a
 * whole aims at rounds x 512 workgroups, shared among the items by their FLOPs - fewer, longer K ranges per item than a launch
 * of its own would use and proportionally fewer partial tiles; rounds <= 0: every item keeps the geometry (splits, ws_floats)
 * of its own dg_wgrad_plan.  The caller sums the partials with dg_wgrad_reduce as for single launches.  DG_EUNSUPPORTED
 * (nothing launched) if an item does not qualify. */
int dg_wgrad_group(const DgWgrad* items, int n, int force, int rounds, void* stream);
int dg_wgrad_group_plan(const DgWgrad* items, int n, int force, int rounds, DgWgradPlan* plans);
/* dw[i] (+)= sum_s ws[s * numel + i] for up to 16 layers in one launch (fixed summation order: deterministic gradients) */
typedef struct DgWgradReduce {
  const float* ws;
  float* dw;
  long numel;       /* 16 Ci Co, a multiple of 4 */
  int splits;
  int accumulate;   /* 1: add onto dw, 0: overwrite */
} DgWgradReduce;
int dg_wgrad_reduce(const DgWgradReduce* items, int n, void* stream);
int dg_wgrad_mfma_supported(const DgWgrad* p);
/* which kernel `force` launches: DgWgradPlan.variant of dg_wgrad_plan (0: a refusal) */
int dg_wgrad_kernel_variant(const DgWgrad* p, int force);
/* 1 when the kernel `force` launches honours DgWgrad.g_mod (the LDS-DMA kernel; Down1's thin matrix-core kernel) */
int dg_wgrad_has_sample_map(const DgWgrad* p, int force);

/* ---- BlurVH  models/ops/common.py:74-88 (forward) and its adjoint --------------------------------------- */
int dg_blur_fwd(const float* x, void* out, int dtype, int B, int H, int W, int ring, void* stream);
/* + mean_acc[0] += mean(mean_src[0..mean_n)) (dg_mean_acc) in the same launch: the R1 penalty's logged value
 * (trainers/dcgan_amp.py:229) rides on the tangent's BlurVH pass.  DG_EUNSUPPORTED unless W % 4 == 0 and 16-byte aligned */
int dg_blur_fwd_mean(const float* x, void* out, int dtype, int B, int H, int W, int ring, const float* mean_src, int mean_n,
                     float* mean_acc, void* stream);
int dg_blur_bwd(const void* d, int dtype, float* dx, int B, int H, int W, int ring, void* stream);
/* the same adjoint at the end of the R1 chain (trainers/dcgan_amp.py:218-235): dx = oscale * g and ssq[b] += sum of g_b^2
 * (ssq zeroed by the caller) in one pass instead of dg_blur_bwd + dg_sample_sum + dg_scale; DG_EUNSUPPORTED unless W % 4 == 0
 * and H W % 1024 == 0 */
int dg_blur_bwd_r1(const void* d, int dtype, float* dx, float oscale, float* ssq, int B, int H, int W, int ring, void* stream);
/* ... and with the R1 tangent's BlurVH in the SAME launch (round 6): out[b] = BlurVH(oscale * g_b) [B,H,W,2] in `dtype`,
 * g_b = BlurVH^T(d[b]) never written; ssq[b] += |g_b|^2 and (mean_acc non-NULL) mean_acc[0] += sum_b |g_b|^2 / mean_n - the
 * logged penalty, trainers/dcgan_amp.py:229 - both zeroed by the caller.  The two launches it replaces: dg_blur_bwd_r1 +
 * dg_blur_fwd_mean; same arithmetic in the same order, so out is bit-identical to theirs.  DG_EUNSUPPORTED (nothing launched)
 * unless W % 4 == 0, H % 4 == 0 and six image rows fit 60 KB of LDS. */
int dg_blur_r1_tangent(const void* d, int dtype, void* out, float oscale, float* ssq, float* mean_acc, int mean_n, int B, int H,
                       int W, int ring, void* stream);

/* ---- final EqualLR(Conv2d(C,1,(h0,w0)))  models/gans/dcgan_eqlr.py:95 ------------------------------------ */
int dg_final_fwd(const void* d4, int dtype, const float* wf, const float* bias, float scale, int B, long n, float* y,
                 void* stream);
/* `_acc` forms (dg_final_fwd_acc, dg_sample_sum_acc, dg_diffaug_fwd_acc, dg_diffaug_bwd_acc): the fp32 accumulator the
 * call adds into (y / out / xsum / gsum) was zeroed by the CALLER - a step that carves all of them from one buffer zero-fills
 * once per step instead of once per call */
int dg_final_fwd_acc(const void* d4, int dtype, const float* wf, const float* bias, float scale, int B, long n, float* y,
                 void* stream);
/* dd4[b] = up[b]*scale*wf*lrelu'(d4[b])*sqrt2 ; dbias4[i%C] += rowscale[b]*dd4[b][i] */
int dg_final_bwd_data(const void* d4, int dtype, const float* wf, const float* up, const float* rowscale, float scale,
                      int B, long n, int C, void* dd4, float* dbias, void* stream);
/* out[i] += scale * sum_b coef[b]*src[b][i] */
int dg_batch_wsum(const void* src, int dtype, const float* coef, float scale, int B, long n, float* out, void* stream);

/* ---- Generator tanh + DUSty maskout  models/gans/dcgan_eqlr.py:71; models/dusty.py:45-59,77-91,107-127 ---- */
/* gout [B,1+k,H,W] planar fp32 (ch0 raw depth -> tanh in place, ch1.. logits); arch 0 none, 1 dusty1, 2 dusty2 */
int dg_head_post_fwd(float* gout, const float* noise_pixel, const float* noise_image, int arch, int training,
                     float tau, float drop_const, int B, long HW, float* mask, float* depth, void* stream);
/* + dsum[b] += sum of depth[b] (dsum zeroed by the caller; HW % 256 == 0 or DG_EUNSUPPORTED): the per-sample sums DiffAugment's
 * contrast needs of its input, produced where the image is produced (dg_diffaug_fwd_pre then skips its own pass) */
int dg_head_post_fwd_sum(float* gout, const float* noise_pixel, const float* noise_image, int arch, int training,
                         float tau, float drop_const, int B, long HW, float* mask, float* depth, float* dsum, void* stream);
/* draw[n] = s_n * d(loss)/d(head output n) (s_depth for ch0, s_conf for the logits: the EqualLR scale of each head,
 * pre-multiplied so the head's backward-data / weight-gradient passes run with scale 1); dbias[n] += unscaled sums.
 * `draw` (planar fp32) may be NULL when the pixel-major bf16 copy is the only consumer (cp 2 / 4, HW % 4 == 0, 16-byte
 * aligned planes; DG_EUNSUPPORTED otherwise, DG_EINVAL when both are NULL).  `bias_ws` (optional, 1024 floats per sample,
 * zero on entry, left zero): per-sample staging of the bias sums - a thousand atomics on one address serialise at
 * ~10 ns each, B slots take them in parallel and the last block of each sample folds its slot into dbias */
int dg_head_post_bwd(const float* gout, const float* noise_pixel, const float* noise_image, const float* mask,
                     const float* ddepth, int arch, float tau, float drop_const, int B, long HW, float s_depth,
                     float s_conf, float* draw, float* dbias, void* draw_pm /* optional bf16 [B,H,W,cp] copy */, int cp,
                     float* bias_ws, void* stream);
/* The learnable Gumbel temperature (GumbelSigmoid(tau=None), models/dusty.py:25-26,38-43): the entry points above with `tau`
 * replaced by tau_w - a DEVICE pointer to the `arch` fp32 master weights, pixel then image (never a bf16 shadow: the kernel
 * forms the slope inv_k = softplus(w_k) + inv_tau_min itself, so a replayed step graph follows the training) - and
 * inv_tau_min = 1 / tau_max.  The backward also takes dtau_w, `arch` accumulators added to like dbias:
 * dtau_w[k] += sigmoid(w_k) * sum over pixels of pre_k s_k (1 - s_k) l_k (l the noisy logit, s its sigmoid, pre the factor in
 * front of the sigmoid's derivative in d1 / d2); the sums take the path the bias sums take (bias_ws: bit-reproducible).
 * arch 1 or 2; DG_EINVAL for a NULL tau_w or dtau_w or inv_tau_min <= 0.  dbias may be NULL. */
int dg_head_post_fwd_lt(float* gout, const float* noise_pixel, const float* noise_image, int arch, int training,
                        const float* tau_w, float inv_tau_min, float drop_const, int B, long HW, float* mask, float* depth,
                        void* stream);
int dg_head_post_fwd_sum_lt(float* gout, const float* noise_pixel, const float* noise_image, int arch, int training,
                            const float* tau_w, float inv_tau_min, float drop_const, int B, long HW, float* mask, float* depth,
                            float* dsum, void* stream);
int dg_head_post_bwd_lt(const float* gout, const float* noise_pixel, const float* noise_image, const float* mask,
                        const float* ddepth, int arch, const float* tau_w, float inv_tau_min, float* dtau_w, float drop_const,
                        int B, long HW, float s_depth, float s_conf, float* draw, float* dbias, void* draw_pm, int cp,
                        float* bias_ws, void* stream);
/* GumbelSigmoid.logistic_noise  models/dusty.py:30-36 */
int dg_logistic_noise(const float* u1, const float* u2, float eps, long n, float* out, void* stream);

/* ---- DiffAugment.forward  utils/diff_augment.py:114-132 and its backward ---------------------------------- */
/* policy bits: 1 brightness, 2 saturation, 4 contrast, 8 translation, 16 cutout; per-sample draws are arguments */
/* The per-sample gate of DiffAugment(policy, p < 1) (rand_translation / rand_cutout restore y[~mask] = x[~mask],
 * utils/diff_augment.py:53-102) travels in the parameter arrays every entry point below already takes: t_h[b] == DG_AUG_OFF
 * switches the translation off for sample b (t_w[b] is then ignored), o_x[b] == DG_AUG_OFF the cutout (o_y[b] ignored) - the
 * stage is then the exact identity for that sample, as if it were not in the policy.  INT32_MIN: no draw produces it.  The
 * colour stages have no gate (the reference overwrites their Bernoulli draw). */
#define DG_AUG_OFF (-2147483647 - 1)
int dg_diffaug_fwd(const float* x, const float* u_b, const float* u_c, const int* t_h, const int* t_w, const int* o_x,
                   const int* o_y, int policy, int B, int H, int W, float* xsum_ws, float* y, void* stream);
int dg_diffaug_fwd_acc(const float* x, const float* u_b, const float* u_c, const int* t_h, const int* t_w, const int* o_x,
                   const int* o_y, int policy, int B, int H, int W, float* xsum_ws, float* y, void* stream);
/* xsum already holds the per-sample sums of x */
int dg_diffaug_fwd_pre(const float* x, const float* u_b, const float* u_c, const int* t_h, const int* t_w, const int* o_x,
                       const int* o_y, int policy, int B, int H, int W, const float* xsum, float* y, void* stream);
int dg_diffaug_bwd(const float* gy, const float* u_b, const float* u_c, const int* t_h, const int* t_w, const int* o_x,
                   const int* o_y, int policy, int B, int H, int W, float* gsum_ws, float* gx, void* stream);
int dg_diffaug_bwd_acc(const float* gy, const float* u_b, const float* u_c, const int* t_h, const int* t_w, const int* o_x,
                   const int* o_y, int policy, int B, int H, int W, float* gsum_ws, float* gx, void* stream);
/* DiffAugment.forward + BlurVH.forward in one pass (utils/diff_augment.py:114-132 -> models/ops/common.py:74-88, the first
 * two modules every D(A(x)) call runs, trainers/dcgan_amp.py:199-204,255-260): the augmented image is only ever D's input,
 * so it is not written - out = BlurVH(A(x)) [nsets B, H, W, 2] in `dtype`.  One or two source sets per launch (the D
 * phase's real | fake halves); xsum = the per-sample sums of x (dg_fetch_reals_sum / dg_head_post_fwd_sum), read by the
 * contrast stage.  DG_EUNSUPPORTED unless W % 4 == 0, H % 4 == 0 (a workgroup owns a band of four output rows) and six image
 * rows fit 60 KB of LDS. */
#define DG_XSUM_PARTS 8       /* partial sums per sample where a producer leaves them un-summed (dg_step_prologue_fetch) */
typedef struct DgAugSet {
  const float* x;            /* [B,1,H,W] fp32 */
  const float* xsum;         /* [B], or with xsum_parts = DG_XSUM_PARTS: [B][DG_XSUM_PARTS] partial sums, added in index order */
  int xsum_parts;            /* 0 / 1: one float per sample */
  const float *u_b, *u_c;    /* [B] the uniform(-1,1) draws of brightness / contrast */
  const int *t_h, *t_w, *o_x, *o_y;
} DgAugSet;
int dg_diffaug_blur_fwd(const DgAugSet* sets, int nsets, int policy, int B, int H, int W, int ring, void* out, int dtype,
                        void* stream);
/* The adjoint pair BlurVH^T -> DiffAugment^T of the G phase (loss_G.backward() through :256-260) in two launches instead
 * of three: dg_blur_bwd_augsum is dg_blur_bwd that also accumulates gsum[b] += the sum of dx[b] over the rows / columns
 * whose gradient reaches the source image (gsum zeroed by the caller; DG_EUNSUPPORTED unless W % 4 == 0), and
 * dg_diffaug_bwd_pre is dg_diffaug_bwd with that sum given. */
int dg_blur_bwd_augsum(const void* d, int dtype, float* dx, const int* t_h, const int* o_x, const int* o_y, int policy,
                       float* gsum, int B, int H, int W, int ring, void* stream);
int dg_diffaug_bwd_pre(const float* gy, const float* u_b, const float* u_c, const int* t_h, const int* t_w, const int* o_x,
                       const int* o_y, int policy, int B, int H, int W, const float* gsum, float* gx, void* stream);
/* dg_diffaug_bwd_pre + dg_head_post_bwd as one launch: the generator's upstream gradient (DiffAugment's adjoint gather of
 * gy) is evaluated per pixel quad inside the head post-processing's backward and never written
 * (loss_G.backward() through utils/diff_augment.py:114-132 into models/dusty.py:77-91,107-127).  DG_EUNSUPPORTED - nothing
 * launched - unless W % 4 == 0, the planes are 16-byte aligned and cp is 2 / 4 (or draw_pm is NULL). */
int dg_head_post_bwd_aug(const float* gout, const float* noise_pixel, const float* noise_image, const float* mask,
                         const float* gy, const float* u_b, const float* u_c, const int* t_h, const int* t_w,
                         const int* o_x, const int* o_y, int policy, const float* gsum, int arch, float tau,
                         float drop_const, int B, int H, int W, float s_depth, float s_conf, float* draw, float* dbias,
                         void* draw_pm, int cp, float* bias_ws, void* stream);
/* ... with the learnable temperature (dg_head_post_bwd_lt's arguments in place of tau) */
int dg_head_post_bwd_aug_lt(const float* gout, const float* noise_pixel, const float* noise_image, const float* mask,
                            const float* gy, const float* u_b, const float* u_c, const int* t_h, const int* t_w,
                            const int* o_x, const int* o_y, int policy, const float* gsum, int arch, const float* tau_w,
                            float inv_tau_min, float* dtau_w, float drop_const, int B, int H, int W, float s_depth, float s_conf,
                            float* draw, float* dbias, void* draw_pm, int cp, float* bias_ws, void* stream);

/* ---- GANLoss, all metrics  models/loss.py:39-61 (loss_D), :66-85 (loss_G) ------------------------------------
 * metric: DG_GAN_* below (the reference's `solver.gan_mode` strings in models/loss.py order).  The loss with the step's
 * bookkeeping folded in (trainers/dcgan_amp.py:203-238,305-309).  D step: dy [2B] = [d/dy_real | d/dy_fake] of
 * w_gan * loss_D; up [2B] = [1..1 | dy_fake] and rs [2B] = [dy_real | 1..1] (the R1 schedule's per-sample vectors, either
 * may be NULL); acc[0..2] += (mean y_real, mean y_fake, loss_D); *dfinal_b += sum dy (the final conv's bias gradient,
 * nullable).  G step writes dy = d(w_gan * loss_G)/dy_fake and acc[0] += loss_G; y_real = D(real) logits, required by the relativistic
 * metrics (ragan / rahinge / ralsgan, average_diff models/loss.py:11-18) and ignored (may be NULL) otherwise.
 * `smoothing` = GANLoss.smoothing (lsgan's real label, models/loss.py:46).  DG_EUNSUPPORTED for an unknown metric. */
enum { DG_GAN_NSGAN = 0, DG_GAN_WGAN = 1, DG_GAN_LSGAN = 2, DG_GAN_HINGE = 3, DG_GAN_RAGAN = 4, DG_GAN_RAHINGE = 5,
       DG_GAN_RALSGAN = 6 };
int dg_gan_d_step(int metric, float smoothing, const float* y_real, const float* y_fake, int B, float w_gan, float* dy,
                  float* up, float* rs, float* acc, float* dfinal_b, void* stream);
int dg_gan_g_step(int metric, const float* y_real, const float* y_fake, int B, float w_gan, float* dy, float* acc,
                  void* stream);
/* The loss step and the final conv's backward as ONE launch: dg_gan_d_step (mode_g = 0; r1 = 1: the R1 schedule's up / rs
 * vectors drive the chain, r1 = 0: upstream dy, unit weights) or dg_gan_g_step (mode_g = 1), then dg_final_bwd_data over
 * the 2B (B) samples with those vectors, and - when dwf is given - the final conv's weight gradient
 * dwf[i] += scale * sum_b dy[b] d4[b][i] (dg_batch_wsum) from the same read of d4: `loss.backward()`'s first links,
 * trainers/dcgan_amp.py:203-235 and :259-309.  DG_EUNSUPPORTED (nothing launched) when the vector forms do not apply or
 * more than 256 samples are in the pass.  dbias_part (optional, n floats, with dbias): instead of atomics onto dbias the launch
 * stores one partial per element of the map (summed over the samples in a fixed order) and the caller sums the n / C rows
 * per channel: dg_wgrad_reduce(ws = dbias_part, dw = dbias, numel = C, splits = n / C) - bit-reproducible bias gradients. */
int dg_final_gan_bwd(int metric, int mode_g, float smoothing, const float* y_real, const float* y_fake, int B, float w_gan,
                     int r1, float* dy, float* up, float* rs, float* acc, float* dfinal_b, const void* d4, int dtype,
                     const float* wf, float scale, long n, int C, void* dd4, float* dbias, float* dwf, float* dbias_part,
                     void* stream);
int dg_mean_acc(const float* x, int n, float* acc, void* stream);
/* Bit-reproducible cross-block sums (round 5).  Registers, for the current device, the arena of small fp32 accumulators the
 * step zero-fills once (per-sample image sums, logits, the augment adjoint's window sums: dg_*_acc / dg_*_sum entry points
 * accumulate into slices of it) together with a shadow of 128 bytes per arena float (a cache line each: adds to one line
 * serialise memory-side), zero at rest: kernels whose blocks add
 * partial sums into an arena slot then add them as 32.32 fixed point to the slot's shadow word (integer addition commutes)
 * and the last block to arrive converts the total - instead of float atomics, whose result depends on the arrival order.
 * arena = shadow = NULL unregisters (float atomics again).  Nothing in the reference to replace: torch's reductions are
 * deterministic on the CPU and the reference never asks for determinism on the GPU. */
int dg_det_arena(float* arena, long n, void* shadow);

/* ---- path-length regularisation  trainers/dcgan_amp.py:268-306 (the parts that are not convolutions) ------------
 * The penalty needs d/dtheta of |d(sum x y)/dz|: a forward-over-reverse pass built from dg_conv / dg_wgrad (the
 * reverse pass ends with dz^T = W^T dp0^T, a dg_wgrad of wmode 2) plus these two.  dg_pl_penalty: lengths |dz_b|, the running baseline pl_ema (device scalar,
 * updated: lerp(.., 0.01) :297), the penalty (:300) and v [B][K] = w * d penalty / d dz; acc[0] += baseline,
 * acc[1] += penalty.  dg_head_post_bwd2: tangent of dg_head_post_bwd along the head tangent `thead` [B,1+k,H,W] (the
 * Hessian of tanh / Gumbel straight-through maskout, models/dusty.py:77-91,107-127), same outputs as dg_head_post_bwd; with draw_pm, cp must be 1..4 (else DG_EINVAL,
 * nothing launched). */
int dg_pl_penalty(const float* dz, int B, int K, float w, float* pl_ema, float* v, float* acc, void* stream);
int dg_head_post_bwd2(const float* gout, const float* noise_pixel, const float* noise_image, const float* mask,
                      const float* ddepth, const float* thead, int arch, float tau, float drop_const, int B, long HW,
                      float s_depth, float s_conf, float* draw, float* dbias, void* draw_pm, int cp, void* stream);

/* ---- Trainer.fetch_reals  trainers/dcgan_amp.py:154-160 (utils/lidar.py:31-36, utils/__init__.py:70-73) -- */
int dg_fetch_reals(const float* pol, const float* mask, float min_depth, float max_depth, float drop_const, long n,
                   float* out, void* stream);
int dg_fetch_reals_sum(const float* pol, const float* mask, float min_depth, float max_depth, float drop_const, int B,
                       long HW, float* out, float* xsum, void* stream); /* + xsum[b] += sum of out[b] (as dg_head_post_fwd_sum) */
/* the same from a device-resident pool of `npool` batches (the synthetic loader): the batch index is
 * *pool_ctr % npool, read ON THE DEVICE, so a training step captured in a hipGraph replays on the next batch without a
 * host-side copy into a static buffer (next(loader) at trainers/dcgan_amp.py:186) */
int dg_fetch_reals_pool_sum(const float* pol_pool, const float* mask_pool, const unsigned long long* pool_ctr, int npool,
                            float min_depth, float max_depth, float drop_const, int B, long HW, float* out, float* xsum,
                            void* stream);

/* ---- data formats either side of the step ---------------------------------------------
 * dg_scan_to_polar: KITTIOdometry.preprocess + .transform  datasets/kitti.py:54-77, optionally fused with
 * Trainer.fetch_reals (trainers/dcgan_amp.py:154-160).  scan [B,Hs,Ws,C] fp32 = the projected scans written by
 * process_kitti.py:76-118 (x, y, z[, reflectance] per cell, C >= 3; C == 4 is read with 16-byte loads); flip [B]
 * bytes (NULL = no horizontal flip; TF.hflip precedes the resize); H x W = cfg.dataset.shape, NEAREST resize =
 * torch's legacy nearest (src = min(floor(dst * in / out), in - 1)).  Outputs (NCHW fp32): pol [B,1,H,W] =
 * (|xyz| - min) / (max - min), mask [B,1,H,W] in {0,1} = |xyz| > 0 & > min & < max, invalid cells zeroed;
 * xyz [B,3,H,W] = xyz / max_depth (nullable); x_real [B,1,H,W] = the network input fetch_reals would make of
 * (pol, mask) with drop_const (nullable).
 * dg_inv_to_xyz: utils.postprocess's depth branch + Coordinate.inv_to_xyz  utils/__init__.py:163-178,
 * utils/lidar.py:38-68.  in [B,1,H,W]: generator depth in [-1,1] (from_tanh = 1: tanh_to_sigmoid + clamp first) or
 * inverse depth in [0,1]; angle [2,H,W] = (elevation, azimuth) grid of LiDAR.init_coordmap (:127-130);
 * drop_const / tol as Coordinate (0 / 1e-8 by default).  depth01 [B,1,H,W] (nullable) receives the [0,1] inverse
 * depth, points [B,3,H,W] the unit-space point map. */
int dg_scan_to_polar(const float* scan, int B, int Hs, int Ws, int C, int H, int W, const unsigned char* flip,
                     double min_depth, double max_depth, float drop_const, float* pol, float* mask, float* xyz,
                     float* x_real, void* stream);
int dg_inv_to_xyz(const float* in, const float* angle, int B, int H, int W, int from_tanh, float min_depth,
                  float max_depth, float drop_const, float tol, float* depth01, float* points, void* stream);
/* utils.postprocess's other branches (utils/__init__.py:169-172): mode 0 = tanh_to_sigmoid(x).clamp(0,1)
 * (depth_orig), mode 1 = sigmoid(x) (confidence) */
int dg_unit_map(const float* x, long n, int mode, float* y, void* stream);
/* xyz_to_normal(points, mode="closest")  utils/__init__.py:215-219 -> estimate_surface_normal utils/geometry.py:38-127
 * (d = 2): points [B,3,H,W] -> normal image [B,3,H,W] in [0,1] */
int dg_normals(const float* points, int B, int H, int W, int d, float* out, void* stream);

/* ---- raw Velodyne scans -> the dataset's files (process_kitti.py; csrc/scan_project.hip) ---------------------
 * dg_scan_project: process_point_clouds  process_kitti.py:76-118 for S raw scans.  points [N,4] fp32 = the scans' (x, y, z,
 * reflectance) records back to back, offsets [S+1] int64 (offsets[0] = 0, ascending, offsets[S] = N: scan s is points
 * [offsets[s], offsets[s+1])); out [S,H,W,4] fp32.  H must be 64 (DG_EUNSUPPORTED otherwise: the reference hard-codes the
 * last ring's row, 63).  Caller-owned workspaces, no initial contents required: keys [S*H*W] u64 (the z-buffer: depth bits
 * << 32 | point index, 64-bit atomicMin), status [S] int32.  Every cell holds the NEAREST point that fell into it (float32
 * depth; on a depth tie the LOWER point index), zeros where none did.  status[s] = 1: scan s has a ring row below -64, where
 * numpy's negative index raises - out[s] is all zeros and the caller reports the scan; rows in [-64,-1] wrap to row + 64 as
 * numpy's do.  cell [N] int32 (nullable): every point's row * W + column (-1: not scattered).  Bit-identical from run to
 * run and whatever S is.  ON RETURN every word of keys is (range bits << 32 | the winner's index within its scan) or the
 * empty word ~0 (csrc/scan_cell.h): the gather does not clear them, and dg_scan_labels reads them.
 * dg_angle_accum / dg_angle_finish: compute_avg_angles  process_kitti.py:143-183.  scans [S,H,W,C] fp32 projected scans
 * (C >= 3) at their own size; per pixel the 32.32 fixed-point sums of pitch = atan2(z, |xy|) and yaw = atan2(y, x) of
 * KITTIOdometry.preprocess's unit-space, range-masked xyz, and the count of pixels with depth > 1e-8, are ADDED to sums
 * [2,H,W] int64 and count [H,W] int32 (the caller zero-fills both before the first chunk): integer sums, so the result does
 * not depend on how the dataset is cut into chunks.  dg_angle_finish: angles [2,H,W] fp32 = sums / count, pitch first; a
 * never-valid pixel gets the mean pitch of its row's valid pixels and the mean yaw of its column's (NaN where the row /
 * column has none - the reference asserts there). */
int dg_scan_project(const float* points, const long* offsets, int S, int H, int W, unsigned long long* keys, int* status,
                    int* cell, float* out, void* stream);
int dg_angle_accum(const float* scans, int S, int H, int W, int C, double min_depth, double max_depth, long long* sums,
                   int* count, void* stream);
int dg_angle_finish(const long long* sums, const int* count, int H, int W, float* angles, void* stream);

/* ---- unordered clouds of any spinning LiDAR -> the dataset's files (dusty_gan_amd/datasets/beams.py;
 * csrc/beam_project.hip).  The reference holds no code for it.  points / offsets as dg_scan_project takes
 * them (both on the device).  Per point, in DOUBLE on the float32 coordinates (csrc/points_body.h): the elevation
 * u = atan2(z, sqrt(x^2 + y^2)) and the range d = |xyz| in metres.  A point with a non-finite coordinate takes no part in
 * either call, nor does the origin.  Neither call uses float atomics.
 * dg_elev_hist: for every point with min_depth < d < max_depth (both strict) and lo <= u < hi,
 *   hist[min(floor((u - lo) * (NB / (hi - lo))), NB - 1)] += 1.  hist [NB] u64 is zeroed by the CALLER and ADDED to, so a
 *   dataset goes through in chunks; integer counts, so the result depends neither on the chunking nor on scheduling.  One
 *   launch: a workgroup counts into NB u32 words of LDS and adds its non-zero bins with one global integer atomic each.
 *   DG_EINVAL: a NULL pointer, S < 1, lo >= hi (or either not finite), NB outside 64..16384.
 * dg_beam_project: out [S,H,W,4] fp32.  beams: H doubles ON THE HOST (read before the call returns), radians, strictly
 *   descending - row 0 is the highest beam, as in the KITTI files.
 *     row     the beam nearest to u in double; on an exact tie the LOWER row
 *     column  dg_scan_project's float32 expression floor(((-atan2f(y, x) / pi + 1) / 2 mod 1) * W) (csrc/scan_cell.h)
 *     cell    keeps its NEAREST point: 64-bit atomicMin of (bits of (float)d << 32 | point index within the scan), so of two
 *             points with the same float32 range the LOWER index wins - dg_scan_project's key and tie rule
 *   The winner's four floats are copied bit for bit; a cell without a point is zero.  cell [N] int32 (nullable): every
 *   point's row * W + column, -1 for a point that took no part - also a finite point whose float32 column coordinate
 *   rounds up to W itself (an azimuth a hair above -pi), which has no column here as in dg_scan_project.  keys [S*H*W]
 *   u64: caller-owned workspace, no initial contents required; ON RETURN every word is (range bits << 32 | the winner's
 *   index within its scan) or the empty word ~0, as dg_scan_project leaves them (the gather does not clear them;
 *   dg_scan_labels reads them).  Three launches (key fill, scatter, gather).  Bit-identical from run to run, whatever S is, and for
 *   any permutation of a scan's points up to the tie rule.  DG_EINVAL: a NULL pointer but cell, S < 1, H outside 1..256,
 *   W outside 1..8192, a table that is not strictly descending or holds an entry outside [-4, 4]. */
int dg_elev_hist(const float* points, const long* offsets, int S, double min_depth, double max_depth, double lo, double hi,
                 int NB, unsigned long long* hist, void* stream);
int dg_beam_project(const float* points, const long* offsets, int S, const double* beams, int H, int W,
                    unsigned long long* keys, int* cell, float* out, void* stream);

/* ---- the picture log of a training run (utils/render.py:18-127, train.py:28-34; csrc/render.hip) ---------------
 * acc: caller-owned u64 words [B,H,W,C] (24.40 fixed point, dg_fix40 of csrc/common.h), ZERO AT REST: all zeros before the
 * first accumulate, zeroed again by dg_splat_finish.  Integer atomics: the image is bit-identical whatever the order of the
 * points.  N <= 2^18 points per cloud (DG_EUNSUPPORTED above: the codec's range), |value| <= 8.
 * dg_splat_accum: bilinear_rasterizer  render.py:67-127 without the final layout.  coords [B,N,2] fp32 (coordinate 0 = row),
 * values [B,N,C] fp32, C <= 4: per point the four neighbouring cells at the clamped indices; a weight is zero where the clamp
 * moved the index, a corner weight below 1e-3 is zero.  A point with a non-finite coordinate is skipped (the reference's
 * .long() of NaN is undefined), and so is a non-finite term.
 * dg_render_points: render_point_clouds  render.py:26-62 up to the splat, per point, inputs untouched.  xyz, normals [B,N,3]
 * fp32; z flipped; @ R ([3,3], or [B,3,3] with R_batched; nullable); + t ([3], or [B,3] with t_batched; nullable); uv = (x/z,
 * y/z) focal + 0.5, times L; the in-image mask 0 < uv < L-1 on the normals only; uv = L - uv; weight = exp(-3 |xyz|) (|xyz| >
 * 1e-8); (weight normals, weight) splatted as C = 4 into acc [B,L,L,4].  Per-point arithmetic in double.
 * dg_splat_finish: out [B,C,H,W] fp32 = the words' values; normalize = 1: channels 0..C-2 divided by (channel C-1 + 1e-8)
 * (render.py:62-63, utils/lidar.py:101-102), channel C-1 as is.  Zeroes acc.
 * dg_image_grid: x [B,C,H,W] fp32 (C = 1 or 3; sample_stride floats between samples, >= C H W: a channel slice of a larger
 * tensor is read in place) times scale -> out uint8 [Hg,Wg,3] laid out as torchvision's make_grid(nrow=4, padding=2,
 * pad_value=0): xmaps = min(4,B), ymaps = ceil(B/xmaps), Hg = ymaps (H+2) + 2, Wg = xmaps (W+2) + 2, tile k at row (k / xmaps)
 * (H+2) + 2, column (k % xmaps) (W+2) + 2.  color = 1: channel 0 through matplotlib's Normalize(0,1) and the 256-entry turbo
 * table (index floor(v 256) clipped to 0..255, NaN -> (0,0,0)), the padding too (turbo(0)); color = 0: the channel
 * replicated (C = 1) or the three channels.  Float -> byte = clip(v 255, 0, 255) truncated (TensorBoard's), NaN -> 0.
 * dg_turbo_lut: the table csrc/turbo_lut.h, 768 floats, into HOST memory (no device needed). */
int dg_splat_accum(const float* coords, const float* values, int B, long N, int C, int H, int W, unsigned long long* acc,
                   void* stream);
int dg_render_points(const float* xyz, const float* normals, int B, long N, int L, const float* R, int R_batched, const float* t,
                     int t_batched, double focal, unsigned long long* acc, void* stream);
int dg_splat_finish(unsigned long long* acc, int B, int C, int H, int W, int normalize, float* out, void* stream);
int dg_image_grid(const float* x, long sample_stride, int B, int C, int H, int W, float scale, int color, unsigned char* out,
                  void* stream);
int dg_turbo_lut(float* host_out);

/* ---- validation metrics (the reference's CUDA extensions and their torch drivers) -------
 * dg_fps: furthest point sampling  utils/sampling/fps/furthest_point_sampling.cu:97-207 (+ gather_points :38-60 when
 * `out` is given).  xyz [B,n,3] fp32, m <= n samples per cloud, temp [B,n] fp32 workspace, idx [B,m] int32, out
 * [B,m,3] (nullable) = the sampled points (downsample_point_clouds, furthest_point_sampling.py:84-93).  Starts at
 * index 0, skips points with |p|^2 <= 1e-3, ties resolved in the reference launcher's thread order.
 * dg_chamfer_dir: all-pairs directed Chamfer means L[i][j] = mean_{p in A_i} min_{q in B_j} |p - q|^2 for A [Na,n,3],
 * B [Nb,m,3] -> L [Na,Nb]; compute_cd(A_i, B_j) of utils/metrics/cov_mmd_1nna.py:20-22 = L_AB[i][j] + L_BA[j][i]
 * (chamfer_distance.cu / nnsearch chamfer_distance.cpp:41-66).  One launch per matrix instead of the reference's
 * Python loop over i (:34-50).
 * dg_grid_vote: JSD occupancy histogram  utils/metrics/jsd.py:24-79: counters[argmin_k |p - grid_k|^2] += 1 for
 * every point (first index on ties); pts [P,3], grid [Ng,3] (unit_cube_grid_point_cloud :11-21), counters [Ng]
 * accumulate.  dg_jsd: _jensen_shannon_divergence :96-107 of two counter vectors -> out[0]. */
int dg_fps(const float* xyz, int B, int n, int m, float* temp, int* idx, float* out, void* stream);
/* dg_fps_map: dg_fps on clouds with strides, addressed as in dg_chamfer_nn: coordinate c of point p of cloud b is
 * X[b x_sb + p x_sp + c x_sc], so a planar point map [B,3,HW] (3 HW, 1, HW) is sampled where it lies, without the
 * packed [B,HW,3] copy.  idx [B,m] int32 and out [B,m,3] (nullable) equal dg_fps's on the packed copy of the same points,
 * bit for bit: one selection rule, one device body.  Planar input (x_sp == 1) of n <= 65 536 points keeps the running
 * minima in registers and LDS and never touches `temp`, which may then be NULL; every other input keeps them in
 * temp [B,n] (NULL there: DG_EINVAL). */
int dg_fps_map(const float* X, long x_sb, long x_sp, long x_sc, int B, int n, int m, float* temp, int* idx, float* out,
               void* stream);
int dg_chamfer_dir(const float* A, int Na, int n, const float* Bc, int Nb, int m, float* L, void* stream);
/* dg_chamfer_paired: the same directed means for B PAIRS of clouds, L[i] = mean_{p in A_i} min_{q in B_i} |p - q|^2 for
 * A [B,n,3], B [B,m,3] -> L [B] (the diagonal of dg_chamfer_dir's matrix: the same per-wave sums; above 1024 points the
 * 512-point slices of a cloud are added with float atomics in arrival order, as in dg_chamfer_dir, so the result is not
 * bit-reproducible run to run there); compute_cd of
 * utils/metrics/cov_mmd_1nna.py:19-21 on paired sets = L_AB + L_BA (evaluate_reconstruction.py:126). */
int dg_chamfer_paired(const float* A, int n, const float* Bc, int m, int B, float* L, void* stream);
/* dg_chamfer_nn: the paired nearest-neighbour search WITH indices (chamfer_distance.cu:9-127, nnsearch
 * chamfer_distance.cpp:39-62), the differentiable form: for B pairs A_i (n points), B_i (m points)
 * dist[i][p] = min_q |A_i[p] - B_i[q]|^2 and idx[i][p] = the LOWEST q that attains it (the reference's strict `<`,
 * chamfer_distance.cu:33,123 / .cpp:53).  Coordinate c of point p of cloud i is X[i x_sb + p x_sp + c x_sc]: a planar
 * point map [B,3,HW] is (3 HW, 1, HW), a cloud [B,n,3] is (3 n, 3, 1).  dist [B,n] fp32, idx [B,n] int32, one writer per
 * element, no atomics; a distance is the one dg_chamfer_paired sums, bit for bit.  n or m above 2^18: DG_EUNSUPPORTED. */
int dg_chamfer_nn(const float* A, long a_sb, long a_sp, long a_sc, int n, const float* Bc, long b_sb, long b_sp, long b_sc,
                  int m, int B, float* dist, int* idx, void* stream);
/* dg_emd: approximate earth mover's distance  utils/metrics/distance/emd/earth_mover_distance.cu (approxmatch :28-190
 * + matchcost :218-262 fused; the [m,n] match matrix is never stored).  paired = 1: out[i] = emd(A_i, B_i) (Na == Nb,
 * the extension's semantics); paired = 0: out [Na,Nb] for all pairs.  The value is the raw cost (compute_emd of
 * utils/metrics/cov_mmd_1nna.py:12-17 divides by the point count). */
int dg_emd(const float* A, int Na, int n, const float* Bc, int Nb, int m, int paired, float* out, void* stream);
/* dg_emd_grad: the gradient of dg_emd's paired cost, EarthMoverDistanceFunction.backward (matchcostgrad1 / matchcostgrad2,
 * earth_mover_distance.cu:305-437), in ONE launch and without a stored match matrix.  The reference's semantics: `match` is a
 * constant (nothing is differentiated through approxmatch),
 *   gradA[i][k] = grad_cost[i] sum_l 2 match[l][k] (A_k - B_l)      gradB[i][l] = grad_cost[i] sum_k 2 match[l][k] (B_l - A_k)
 * with match = the sum over the ten annealing levels of exp(level d^2) ratioL[k] ratioR[l].  Both are accumulated while the
 * mass is produced (dg_emd's three sweeps, plus a fourth per level in which a thread owns l), in the output rows themselves:
 * one writer per row, no atomics, no [B,m,n] buffer, deterministic.  Paired clouds only: A [B,n,3], Bc [B,m,3], grad_cost [B]
 * (NULL = ones; the scale is applied after the sum, as the reference does), gradA [B,n,3], gradB [B,m,3]; cost [B] (nullable)
 * = dg_emd(..., paired = 1), bit for bit.  One workgroup per pair with dg_emd's LDS footprint, so the same cap:
 * n + m <= 6400, DG_EUNSUPPORTED above. */
int dg_emd_grad(const float* A, int n, const float* Bc, int m, int B, const float* grad_cost, float* cost, float* gradA,
                float* gradB, void* stream);
/* dg_chamfer_backward: the Chamfer extension's backward (chamfer_distance.cpp:82-140 and the .cu backward) for packed clouds
 * A [B,n,3], Bc [B,m,3], from the gradients g1 [B,n], g2 [B,m] of the two distance vectors and the neighbour indices
 * idx1 [B,n], idx2 [B,m] that dg_chamfer_nn returned:
 *   gradA[i][p] += 2 g1[i][p] (A_p - B_idx1[p]),  gradB[i][idx1[p]] -= the same;     mirrored with g2 / idx2.
 * gradA [B,n,3] and gradB [B,m,3] are OVERWRITTEN.  The term a point gives itself has one writer; the terms it receives as a
 * neighbour are summed in 24.40 fixed point with integer atomics (order-independent: two runs agree bit for bit) and a
 * finishing pass adds the two and rounds once.  acc: B (n + m) * 4 u64 words, ZERO AT REST (the finishing pass zeroes what it
 * reads).  The fixed point holds |term| < 2^22 per coordinate and |total| < 2^22 at a resolution of 2^-40: unit-space
 * points (|A_p - B_k| <= 2) and |g| up to 1 - a sum over the distances; a mean over n points gives 1 / n - stay at |term| <= 4
 * and, with at most 2^18 points per cloud, |total| <= 2^20.  A term outside the window, or not finite, turns the entries that
 * should have received it into NaN.  An index outside its cloud contributes nothing.  n or m above 2^18: DG_EUNSUPPORTED. */
int dg_chamfer_backward(const float* A, int n, const float* Bc, int m, int B, const float* g1, const float* g2, const int* idx1,
                        const int* idx2, float* gradA, float* gradB, unsigned long long* acc, void* stream);
int dg_grid_vote(const float* pts, long P, const float* grid, int Ng, float* counters, void* stream);
int dg_jsd(const float* P, const float* Q, int n, float* out, void* stream);
/* SWD descriptors  utils/metrics/swd.py:16-62.  dg_pyr_down: pyramid_down (:24-30) on `planes` = B*C images
 * [H,W] -> [H/2,W/2] (H, W even).  dg_pyr_up_sub: fine -= pyramid_up(coarse) (:33-50), in place.
 * dg_extract_patches: extract_patches (:53-62) for given positions: out [B,NP,C,ph,pw], inds [NP] int64 =
 * y * (W - pw + 1) + x of each patch's top-left corner (the reference draws them with randperm). */
int dg_pyr_down(const float* in, long planes, int H, int W, float* out, void* stream);
int dg_pyr_up_sub(float* fine, const float* coarse, long planes, int H, int W, void* stream);
int dg_extract_patches(const float* img, int B, int C, int H, int W, int ph, int pw, const long* inds, int NP,
                       float* out, void* stream);

/* ---- small reductions / helpers --------------------------------------------------------------------------- */
int dg_sample_sum(const float* x, int B, long n, int sq, float* out, void* stream); /* out[b] = sum x or x^2 */
int dg_sample_sum_acc(const float* x, int B, long n, int sq, float* out, void* stream); /* out[b] = sum x or x^2 */
int dg_scale(const float* x, float a, long n, float* y, void* stream);
/* p[0..n) = 0 as a kernel launch (optim.zero_grad, trainers/dcgan_amp.py:177,246, and the step's accumulators).  The
 * library never uses hipMemsetAsync: its small fills replayed wrong from a hipGraph after a host-side synchronize. */
int dg_zero(float* p, long n, void* stream);
/* k <= 4 fp32 buffers (16-byte aligned, counts multiples of 4) zero-filled by ONE launch: the step's accumulator arena and
 * the two networks' gradient buffers (optim.zero_grad, trainers/dcgan_amp.py:177,246) as one graph node */
int dg_zero_multi(float* const* ptrs, const long* counts, int k, void* stream);

/* ---- optim.Adam.step + ema_inplace  trainers/dcgan_amp.py:116-125,238,312,316 and :30-35 ------------------ */
int dg_adam_ema_step(float* p, const float* grad, float* m, float* v, float* ema, void* shadow, int shadow_dtype,
                     long n, float gscale, float lr, float beta1, float beta2, float eps, int step, float ema_decay,
                     void* stream);
int dg_cast(const float* src, void* dst, int dtype, long n, void* stream);
/* the way back: dst[i] = (float)src[i] for DG_BF16 / DG_BF16X2 sources (hi + lo), a copy for DG_F32 */
int dg_uncast(const void* src, int dtype, float* dst, long n, void* stream);
/* up to 16 fp32 buffers (n[i] elements, multiples of 64) -> DG_BF16X2 copies in ONE launch: the split-bf16 twins of the fat
 * layers' weight shadows, rebuilt behind every optimizer step in the fp32x3 mode */
int dg_cast_x2_multi(const float* const* src, void* const* dst, const long* n, int count, void* stream);
int dg_transpose_shadow(const float* master, void* dst, int dtype, int Ci, int Co, void* stream);
/* every conv segment of a network in one launch: desc_dev[5 i + (0..4)] = (source element offset in master, destination
 * pointer, Ci, Co, first tile index), tiles = 16 taps x ceil(Ci/32) x ceil(Co/32) per segment (device memory) */
int dg_transpose_shadow_multi(const float* master, const long long* desc_dev, int nseg, int total_tiles, int dtype,
                              void* stream);
/* the same launch also rebuilds up to 4 DgConv.up_frag buffers from the fp32 master (bf16 only): weight element
 * (tap, n, k) of fragment set i is master[off + tap * m_st + n * m_sn + k * m_sk], rounded to bf16 like the shadow; K = 64.
 * One launch per optimizer step keeps every low-precision copy of a network current (Head / Down1 weights change with
 * optim.step, trainers/dcgan_amp.py:238,314) */
typedef struct DgUpFrag {
  long long off;             /* element offset of the layer's weights in `master` */
  void* frag;                /* DG_UP_FRAG_BYTES */
  long long m_st, m_sn, m_sk;
  int N, Hc, adj;            /* output channels (<= 4), coarse rows, DgConv.adj of the launches that use it */
} DgUpFrag;
int dg_transpose_shadow_multi_frags(const float* master, const long long* desc_dev, int nseg, int total_tiles, int dtype,
                                    const DgUpFrag* frags, int nfrag, void* stream);
/* the same launch with one more block doing what dg_counter_add_multi / dg_counter_add_multi_snap do (snap_idx < 0: no
 * snapshot): the last launch of a training step - the shadow refresh behind the generator's optimizer - also advances the
 * step's counters and files its scalars */
int dg_transpose_shadow_multi_tail(const float* master, const long long* desc_dev, int nseg, int total_tiles, int dtype,
                                   const DgUpFrag* frags, int nfrag, unsigned long long* const* counters,
                                   const unsigned long long* deltas, int k, int snap_idx, const float* src, int n,
                                   float* dst_ring, int ring, void* stream);

/* ---- Philox4x32-10 draws (the reference uses torch's device RNG: trainers/dcgan_amp.py:151-152, models/dusty.py:33-34,
 *      utils/diff_augment.py:27-28,59-60,86-87) --------------------------------------------------------------- */
int dg_philox_bits(uint64_t seed, uint64_t stream_id, uint64_t offset, long n4, uint32_t* out, void* stream);
/* kind 0 uniform[0,1), 1 normal, 2 uniform(lo,hi), 3 int32 in [ilo,ihi) */
int dg_philox_fill(uint64_t seed, uint64_t stream_id, uint64_t offset, int kind, float lo, float hi, int ilo, int ihi,
                   long n, void* out, void* stream);

/* one DiffAugment parameter set per sample: uf [3][B] = u_b,u_s,u_c in (-1,1); qi [4][B] = t_h,t_w,o_x,o_y
 * (ranges of utils/diff_augment.py:58-60,85-87); consumes 2*B Philox counters starting at `offset` */
int dg_aug_draw(uint64_t seed, uint64_t stream_id, uint64_t offset, int B, int H, int W, float* uf, int* qi,
                void* stream);
/* ... for DiffAugment(policy, p): the same seven numbers, then the two gates of sample b from ONE more Philox block at the
 * sample's first counter, offset + 2 b, under the stream DG_STREAM_AUG_GATE | stream_id << 32 (the caller's stream id in the high
 * word: augmenters of one seed on different streams draw different gates; the counter advance stays 2 per sample): word 0
 * gates the translation, word 1 the cutout, a stage is ON iff u < p with u = (word >> 8) 2^-24; a stage that is off gets
 * DG_AUG_OFF in t_h[b] / o_x[b].  p == 1 draws no gates: dg_aug_draw itself.  DG_EINVAL unless 0 <= p <= 1. */
#define DG_STREAM_AUG_GATE 16
int dg_aug_draw_p(uint64_t seed, uint64_t stream_id, uint64_t offset, int B, int H, int W, float p, float* uf, int* qi,
                  void* stream);

/* ---- device-resident counters (hipGraph-friendly variants): Philox offset / Adam step count read from device memory;
 *      dg_counter_add advances a counter after its consumers.  A step captured once replays with fresh draws. */
int dg_counter_add(unsigned long long* counter, unsigned long long delta, void* stream);
/* k <= 8 distinct counters advanced by one launch (DG_EINVAL on duplicates) */
int dg_counter_add_multi(unsigned long long* const* counters, const unsigned long long* deltas, int k, void* stream);
/* the same, and src[0..n) (n <= 64) is filed in slot (OLD value of counters[snap_idx]) % ring of dst_ring (n floats per slot;
 * device memory or mapped pinned host memory): the logged scalars of Trainer.step (trainers/dcgan_amp.py:319-323, five
 * blocking all_reduce + .item() there) leave the device with the step's last launch and are read by the host behind an
 * event, without a copy node or a blocking read on the launch stream */
int dg_counter_add_multi_snap(unsigned long long* const* counters, const unsigned long long* deltas, int k, int snap_idx,
                              const float* src, int n, float* dst_ring, int ring, void* stream);
int dg_philox_fill_dev(uint64_t seed, uint64_t stream_id, const unsigned long long* offset_dev, int kind, float lo,
                       float hi, int ilo, int ihi, long n, void* out, void* stream);
/* GumbelSigmoid.logistic_noise (models/dusty.py:30-36) in one launch: the same numbers as two dg_philox_fill_dev uniform
 * fills of n elements (U1, then U2) followed by dg_logistic_noise; the caller advances the counter by 2 ((n + 3) / 4) */
int dg_philox_logistic_dev(uint64_t seed, uint64_t stream_id, const unsigned long long* offset_dev, float eps, long n,
                           float* out, void* stream);
/* One launch in front of a training step: the zero-fill of k <= 4 fp32 buffers (dg_zero_multi: the accumulator arena and
 * the gradient buffers, optim.zero_grad at trainers/dcgan_amp.py:177,246) plus up to 6 draws - the numbers
 * dg_philox_fill_dev / dg_philox_logistic_dev / dg_aug_draw_dev produce for the same (seed, stream_id, *offset_dev + base):
 * sample_latents (trainers/dcgan_amp.py:151-152), GumbelSigmoid.logistic_noise (models/dusty.py:30-36) and DiffAugment's
 * parameters (utils/diff_augment.py:27-28,59-60,86-87).  The caller advances the counters as for the single draws. */
typedef struct DgDraw {
  int kind;                  /* 0 dg_philox_fill_dev, 1 dg_philox_logistic_dev, 2 dg_aug_draw_dev */
  int fill_kind;             /* kind 0: 0 U[0,1), 1 N(0,1), 2 U[lo,hi), 3 integers in [ilo, ihi) */
  uint64_t seed, stream_id;
  const unsigned long long* offset_dev;
  unsigned long long base;   /* added to *offset_dev: what earlier draws of this launch take from the same generator */
  float lo, hi, eps;
  int ilo, ihi;
  long n;                    /* kind 0 / 1: elements */
  void* out;                 /* kind 0 / 1 */
  void* out_bf16;            /* kind 0, optional: a bfloat16 copy of a float fill (the generator's latent operand) */
  int B, H, W;               /* kind 2 */
  float* uf;                 /* kind 2: [3][B] */
  int* qi;                   /* kind 2: [4][B] */
  float p;                   /* kind 2: DiffAugment's probability (dg_aug_draw_p); 1 and no p_dev: no gates are drawn.  NOT neutral
                              * at zero: a zero-initialised DgDraw has p = 0, which gates every sample off - set 1 for today's draw */
  const float* p_dev;        /* kind 2, optional: p read from device memory when the draw runs (dg_aug_draw_p_dev) */
} DgDraw;
int dg_step_prologue(float* const* zero_ptrs, const long* zero_counts, int k, const DgDraw* draws, int ndraw, void* stream);
/* ... and fetch_reals of the step's batch as more workgroups of the SAME launch (round 6; trainers/dcgan_amp.py:154-160 with
 * Coordinate.invert_depth, utils/lidar.py:31-36, and sigmoid_to_tanh, utils/__init__.py:70-73; same arithmetic as
 * dg_fetch_reals_pool_sum): out[B,1,H,W] = the inverse-depth image in [-1, 1] of batch (*pool_ctr % npool) of the device-resident
 * pool (pool_ctr NULL: pol / mask ARE the batch), and parts[B][DG_XSUM_PARTS] = the partial sums of out per sample - block j owns
 * pixels [j HW / DG_XSUM_PARTS, (j + 1) HW / DG_XSUM_PARTS) of the batch and STORES its sum (no accumulator this launch would
 * have to zero first, no atomics: bit-reproducible); DgAugSet.xsum_parts tells the reader.  DG_EUNSUPPORTED (nothing launched)
 * unless HW % (1024 DG_XSUM_PARTS) == 0 and the images are 16-byte aligned. */
typedef struct DgFetch {
  const float *pol, *mask;              /* [npool][B][HW] (or [B][HW]) polar depth in [0, 1] and validity {0, 1} */
  const unsigned long long* pool_ctr;   /* device-resident loader position, or NULL */
  int npool;
  float min_depth, max_depth, drop_const;
  int B;
  long HW;
  float* out;                           /* [B][HW] */
  float* parts;                         /* [B][DG_XSUM_PARTS] */
  /* the resident form (nslab > 0; all zero = the pool form above): pol = a scan split's store [nvar][nslab B][HW] in sampler
   * order (variant 1 = the horizontally flipped sample), mask unused (derived as pol > 0, see datasets/resident.py), npool
   * unused.  Batch = slab (*pool_ctr % nslab); sample b of it reads variant flip_tab[((*pool_ctr / nslab) & 1) nslab B +
   * slab B + b] - two per-sample flip tables, chosen by epoch parity - or variant 0 when flip_tab is NULL. */
  long nslab;
  const unsigned char* flip_tab;        /* [2][nslab B] {0, 1}, or NULL */
} DgFetch;
int dg_step_prologue_fetch(float* const* zero_ptrs, const long* zero_counts, int k, const DgDraw* draws, int ndraw,
                           const DgFetch* fetch, void* stream);
/* the resident form of dg_fetch_reals_pool_sum (same arithmetic and per-block sums; the batch and its flips picked on the device
 * as in DgFetch's resident form): fetch_reals of a step's further micro-batch where the fetch does not ride on the prologue */
int dg_fetch_reals_resident_sum(const float* store, const unsigned long long* pool_ctr, long nslab,
                                const unsigned char* flip_tab, float min_depth, float max_depth, float drop_const, int B,
                                long HW, float* out, float* xsum, void* stream);
/* batch `slab` of a resident store as the file loader yields it: depth [B][HW] = the stored polar depth of sample b's variant
 * flip[b] (flip NULL: variant 0), mask [B][HW] = depth > 0 ? 1 : 0.  16-byte accesses where HW % 4 == 0. */
int dg_resident_gather(const float* store, long nslab, int B, long HW, long slab, const unsigned char* flip, float* depth,
                       float* mask, void* stream);
int dg_aug_draw_dev(uint64_t seed, uint64_t stream_id, const unsigned long long* offset_dev, int B, int H, int W,
                    float* uf, int* qi, void* stream);
/* dg_aug_draw_p from the device-resident counter, with p itself read from device memory WHEN THE DRAW RUNS (a captured step
 * follows the adaptive controller's p, dg_ada_update); a p outside [0, 1] or not finite acts as its clamp (NaN: 0) */
int dg_aug_draw_p_dev(uint64_t seed, uint64_t stream_id, const unsigned long long* offset_dev, int B, int H, int W,
                      const float* p_dev, float* uf, int* qi, void* stream);
/* ---- the adaptive controller of DiffAugment's p (StyleGAN2-ADA's rule; the reference's p is a constant,
 *      utils/diff_augment.py:114-122): one single-workgroup launch per D phase, only when the controller is on.
 * state (device memory, the layout below; `p` is what dg_aug_draw_p_dev / DgDraw.p_dev read) and pend (device, two integers:
 * the sign sum and count of the iteration under way).
 * y_real != NULL (the D phase's real logits [B], trainers/dcgan_amp.py:203): pend += {sum_b sign(y_real[b]), B} - sign as
 * torch.sign, a logit that is not finite counts 0 - and rt_slot[0] += rt_scale * (this call's sum / B) (optional).
 * advance != 0 (the iteration's last call; with several ranks the caller sums pend over the ranks first, then calls with
 * y_real == NULL): window += pend, pend = 0, steps += 1, and at steps % interval == 0:  r_t = sign_sum / count,
 * p = clamp(p + sign(r_t - target) * (batch_size * interval) / (kimg * 1000), 0, 1) in float32 in this order, window = 0.
 * p_slot[0] = p behind this call (optional).  Integer sums: two runs give the same bits. */
typedef struct DgAdaState {
  float p;
  long long sign_sum, count; /* the window since the last adjustment */
  int steps;                 /* iterations seen */
} DgAdaState;
int dg_ada_update(const float* y_real, int B, void* state, long long* pend, int advance, float target, int interval,
                  int batch_size, float kimg, float rt_scale, float* rt_slot, float* p_slot, void* stream);
/* Adam with the (0-based, already-completed) step count in device memory: this call is step *step_dev + 1 */
int dg_adam_ema_step_dev(float* p, const float* grad, float* m, float* v, float* ema, void* shadow, int shadow_dtype,
                         long n, float gscale, float lr, float beta1, float beta2, float eps,
                         const unsigned long long* step_dev, float ema_decay, void* stream);

/* The optimizer of a network as ONE launch that forms the gradients it consumes (round 6; trainers/dcgan_amp.py:238, :312-316
 * behind loss.backward()'s last reductions): per piece of the flat buffers, the sum of the piece's split-K partial rows
 * (`part`, [splits][numel], fixed order - what dg_wgrad_reduce would add to the gradient; `accumulate`: + the gradient buffer's
 * content), optionally + ws_scale * sum_b ws_coef[b] * ws_src[b][i] (dg_batch_wsum: the final conv's weight gradient from the
 * R1 tangent; ws_coef NULL = 1), then Adam with beta1 = 0 + the EMA (`ema` NULL: none) exactly as dg_adam_ema_step_dev, and
 * every store: master, exp_avg_sq, EMA, the summed gradient (kept), the compute-type shadow, and for kind 1 - a [16][ci][co]
 * conv segment, co == 64 or co % 128 == 0, ci % 16 == 0 - the [16][co][ci] shadow `shadow_t` (dg_transpose_shadow_multi's output).  Replaces
 * dg_batch_wsum + dg_wgrad_reduce + dg_adam_ema_step_dev + the fat layers' share of dg_transpose_shadow_multi; the results are
 * bit-identical to theirs (same order of additions) except where ws_src folds dg_batch_wsum in.  Pieces must not overlap;
 * anything of the buffers no piece covers is left untouched.  `first_block` is filled by the library. */
#define DG_OPT_MAX_SEG 20
typedef struct DgOptSeg {
  long long off, numel;          /* piece [off, off + numel) of p / grad / v / ema / shadow, multiples of 4 */
  const float* part;             /* partial rows or NULL */
  int splits, accumulate;
  int kind, ci, co;              /* kind 0: flat; 1: conv tile walk (needs shadow_t) */
  void* shadow_t;
  const void* ws_src; const float* ws_coef; long long ws_stride; int ws_n, ws_bf16; float ws_scale;
  int first_block;
} DgOptSeg;
int dg_adam_fused(float* p, float* grad, float* v, float* ema, void* shadow, int shadow_dtype, const DgOptSeg* segs, int nseg,
                  float gscale, float lr, float beta2, float eps, const unsigned long long* step_dev, float ema_decay,
                  void* stream);
/* Adam (beta1 = 0) + EMA of Proj.weight [Np][K] with its weight gradient wscale * dp0^T z (trainers/dcgan_amp.py:309,312:
 * loss_G.backward() + optim_G.step() for that one tensor) formed inside the kernel from the bf16 operands dp0 [nb][Np]
 * and zT [nb][K]: the 268 MB gradient is never written.  Two kernels behind it: an LDS-resident VALU kernel for the
 * per-GPU batch (nb even, <= 64, operands fit 64 KB of LDS) and, for larger nb (the all-gathered global batch of a
 * data-parallel run), the MFMA gradient GEMM with the optimizer as its epilogue (Np % 128 == 0, K % 128 == 0).
 * Round 6: op_dtype DG_F32 (fp32 operands on the fp32 matrix instructions: the exact-fp32 mode) and DG_F32 | DG_FORCE_FP32X3
 * (fp32 operands split into bf16 pairs in registers: the fp32x3 mode) take the matrix-core path too - those modes ran the
 * gradient GEMM, its reduce and the plain optimizer over the 268 MB gradient.  shadow may be NULL (fp32 modes: the master IS
 * what the forward pass reads).  DG_EUNSUPPORTED for anything else (other element types, other shapes) - the caller then uses
 * dg_wgrad + dg_adam_ema_step_dev. */
int dg_adam_proj_fused(float* p, float* v, float* ema, void* shadow, int shadow_dtype, const void* dp0, const void* zT,
                       int op_dtype, int nb, long Np, int K, float wscale, float gscale, float lr, float beta2,
                       float eps, const unsigned long long* step_dev, float ema_decay, void* stream);

/* ---- GAN inversion  evaluate_reconstruction.py:32-164 with utils/__init__.py:224-246 ------------------------------------
 * dg_inv_loss_grad: masked_loss (utils/__init__.py:237-246) of the reference inverse depth `ref` [B,HW] against the generated
 * one - gen [B,*] with sample stride gen_sb: tanh_to_sigmoid of it (from_tanh = 1: the head output's tanh'd depth channel,
 * gout [B,nheads,HW]) or the image itself - under `mask` [B,HW]: loss[b] = sum(|ref - gen| or (ref - gen)^2) mask / msum[b]
 * (distance 0 = l1, 1 = l2; msum[b] = sum of the sample's mask, 0 gives NaN as in the reference).  With draw / draw_pm the
 * same launch writes d loss_b / d (head depth pre-activation) * s_depth (the head's EqualLR scale) where dg_head_post_bwd
 * writes its head gradient - draw [B,nheads,HW] planar fp32 and / or draw_pm [B,HW,cp] pixel-major bf16 - confidence
 * channels zero; l1 takes sign(gen - ref) with sign(0) = 0.  Per-sample sums in a fixed order: nchunk > 1 workgroups per
 * sample store their partials in parts [B*nchunk] and draw tickets [B] (zero on entry, left zero); the last one adds the
 * partials in chunk order.
 * dg_sphere_adam: one step of SphericalOptimizer (utils/__init__.py:224-234: torch.optim.Adam, then every latent row / sqrt(
 * mean(row^2) + 1e-9)) on latent [B,nz] fp32 with moments m, v [B,nz] and gradient grad(b, j) = grad[b g_sb + j g_sk], at
 * step index k = *step_dev (device memory: a replayed hipGraph advances it), Adam step count k + 1.  sched [num_step + 1][3]
 * holds per step k (fp32, formed as torch's Adam forms them): the step size lr lambda(k) / (1 - beta1^(k+1)) with the LambdaLR schedule of
 * evaluate_reconstruction.py:72-77 (lambda(0) = 0), sqrt(1 - beta2^(k+1)), and the perturbation strength 0.05 noise_sigma
 * max(0, 1 - k/num_step/noise_ratio)^2 (:100-104); index k > num_step reads row num_step.  The same launch writes the
 * generator input of step k + 1, latent + strength(k + 1) randn (perturb = 0: the latent alone), into zT [B,nz] of
 * z_dtype (DG_F32 / DG_BF16) - randn from Philox (seed, counter (k' ceil(nz/4) + j/4, stream_id | b << 32)), Box-Muller on
 * word pairs as dg_philox_fill kind 1 - or noise_in [B,nz] when given (the perturbation itself, injected).  The last
 * row's workgroup increments *step_dev (ticket [1]: zero on entry, left zero).
 * prime = 1: no optimiser step, only zT for step *step_dev (the first forward).  nz <= 1024.
 * dg_sphere_adam_rows: the same with the perturbation of row b keyed as row row0 + b (stream word stream_id | (row0 + b) <<
 * 32; row0 >= 0): a scan keyed by its dataset index draws the same perturbations in any batch.  row0 = 0 is dg_sphere_adam.
 * dg_depth_metrics: compute_depth_error + compute_depth_accuracy (utils/metrics/depth.py) of revert_depth(inv, norm=False)
 * (utils/lidar.py:38-47) of inv_ref / inv_gen [B,HW] under mask [B,HW], and the drop ratios of the evaluation CSV
 * (evaluate_reconstruction.py:138-152): out [B,9] = abs_rel, sq_rel, rmse, rmse_log, accuracy_1..3, drop_gen, drop_ref.
 * drop_gen = sum(1 - keep) / HW over keep [B,kc,HW] (the dusty masks), or with keep_is_depth over |keep| > tol of the
 * depth image keep [B,1,HW].  max_depth <= 0: inv_ref / inv_gen are depths already (no revert_depth).  One workgroup per
 * sample; a zero mask sum gives NaN as in the reference. */
int dg_inv_loss_grad(const float* gen, long gen_sb, int from_tanh, const float* ref, const float* mask, const float* msum,
                     int distance, int B, long HW, float s_depth, float* draw, int nheads, void* draw_pm, int cp,
                     float* parts, unsigned* tickets, int nchunk, float* loss, void* stream);
/* dg_inv_loss_grad_add: the same, as a FURTHER term of the loss (demo.py:516-519 adds l1 and l2): loss[b] += the term, the
 * depth channel of draw (required) += its gradient, and draw_pm, when given, = the planar sums rounded to bf16. */
int dg_inv_loss_grad_add(const float* gen, long gen_sb, int from_tanh, const float* ref, const float* mask, const float* msum,
                         int distance, int B, long HW, float s_depth, float* draw, int nheads, void* draw_pm, int cp,
                         float* parts, unsigned* tickets, int nchunk, float* loss, void* stream);
/* The Chamfer term of the inversion loss  demo.py:508-515 with chamfer_distance.cpp:82-140: loss_b = mean_j d1 + mean_k d2
 * between the target's points R and P = postprocess(out)["points"] (utils/__init__.py:163-178), both planar [B,3,HW] as
 * dg_inv_to_xyz writes them (HW <= 2^18), with (d1, idx1) = dg_chamfer_nn(R, P) and (d2, idx2) = dg_chamfer_nn(P, R).
 * dg_inv_chamfer_scatter: for every target point j adds R_j and a count of 1 to generated pixel idx1[j] in acc [B,HW,4]
 * u64 words (24.40 fixed point, dg_fix40 of csrc/common.h, word 3 the count; integer atomics: order-independent), ZERO AT
 * REST: dg_inv_chamfer_grad zeroes what it reads.
 * dg_inv_chamfer_grad: loss[b] = (or += with add) the term, per-sample sums in the fixed order of dg_inv_loss_grad (parts
 * [B*nchunk], tickets [B]), and per generated pixel k  gP = (2/HW)(P_k - R_idx2[k]) + (2/HW)(c_k P_k - S_k), chained through
 * Coordinate.inv_to_xyz (utils/lidar.py:61-68; angle [2,HW], the LiDAR's drop_const 0, `tol`), the closed-interval clamp
 * and tanh_to_sigmoid to g = d loss_b / d depth (depth [B,HW]: the generator's MASKED depth), then the head gradient of
 * the EVAL-mode graph (models/dusty.py:45-59,77-91,107-127) where dg_head_post_bwd writes its: depth channel g mask
 * (1 - t^2) s_depth, pixel confidence g (t - drop_const) mask_image sp (1 - sp) / tau s_conf (the straight-through Gumbel
 * sigmoid under the fixed noise_pixel [B,HW]), dusty2's image channel 0 (eval: a plain threshold, :120).  gout [B,nheads,HW]
 * (tanh'd depth, logits) and mask [B,arch,HW] as dg_head_post_fwd left them; nheads = arch + 1.  draw planar fp32 and / or
 * draw_pm [B,HW,cp] bf16 (the planar value rounded); add = 1: the gradient is added to what draw (required) holds. */
int dg_inv_chamfer_scatter(const float* R, const int* idx1, int B, long HW, unsigned long long* acc, void* stream);
int dg_inv_chamfer_grad(const float* P, const float* R, const float* d1, const float* d2, const int* idx2,
                        unsigned long long* acc, const float* depth, const float* angle, const float* gout,
                        const float* noise_pixel, const float* mask, int arch, float tau, float drop_const, float min_depth,
                        float max_depth, float tol, int B, long HW, float s_depth, float s_conf, int add, float* draw,
                        int nheads, void* draw_pm, int cp, float* parts, unsigned* tickets, int nchunk, float* loss,
                        void* stream);
/* The earth mover's term of the inversion loss, on K rays of the target (beyond the reference's demo, which has no EMD loss;
 * the distance is the one its evaluation reports: compute_emd, utils/metrics/cov_mmd_1nna.py:12-17, on a furthest-point
 * sample).  T_b = the K pixels dg_fps_map selects on the target's point map R_b, drawn once; each step the generated point
 * map P_b is read on the SAME pixels, loss_b = dg_emd(P_b[T_b], R_b[T_b]) / K, and dg_emd_grad's gradA (grad_cost = 1 / K,
 * the match a constant as in the reference's backward) is the point gradient at the sampled pixels, zero elsewhere.
 * dg_points_gather: out [B,K,3] packed, out[b][s][c] = X[b x_sb + idx[b][s] x_sp + c x_sc] for idx [B,K] int32 - strides as
 * dg_chamfer_nn's: a planar point map [B,3,n] is (3 n, 1, n), a packed cloud [B,n,3] is (3 n, 3, 1).  An index outside
 * [0, n) writes zeros.  One writer per element.
 * dg_inv_points_grad: the dense pixel pass.  gP [B,K,3] the point gradient of the K samples; slot [B,HW] int32 the inverse of
 * T_b (slot[b][T_b[s]] = s, -1 for a pixel that is no sample: its point gradient is 0; a value >= K counts as -1);
 * term [B] and scale: loss[b] = (add ? loss[b] : 0) + term[b] scale, the product rounded on its own, written by one thread per
 * sample (no parts, no tickets: the cost is a per-sample scalar already).  Per pixel the point gradient is chained exactly as
 * dg_inv_chamfer_grad chains its own - one device body, csrc/inv_chain.h - with that entry's depth, angle, gout, noise_pixel,
 * mask, arch, tau, drop_const, min_depth, max_depth, tol, s_depth, s_conf and outputs draw / draw_pm / add / nheads / cp.  EVERY
 * pixel is written, by one writer, without atomics: bit-reproducible.  nchunk workgroups per sample (1..65535). */
int dg_points_gather(const float* X, long x_sb, long x_sp, long x_sc, int n, const int* idx, int B, int K, float* out,
                     void* stream);
int dg_inv_points_grad(const float* gP, const int* slot, const float* term, float scale, int K, const float* depth,
                       const float* angle, const float* gout, const float* noise_pixel, const float* mask, int arch, float tau,
                       float drop_const, float min_depth, float max_depth, float tol, int B, long HW, float s_depth, float s_conf,
                       int add, float* draw, int nheads, void* draw_pm, int cp, int nchunk, float* loss, void* stream);
int dg_sphere_adam(const float* grad, long g_sb, long g_sk, float* latent, float* m, float* v, unsigned long long* step_dev,
                   unsigned* ticket, const float* noise_in, void* zT, int z_dtype, int B, int nz, const float* sched,
                   int num_step, float beta1, float beta2, float eps, int perturb, uint64_t seed, uint64_t stream_id, int prime,
                   void* stream);
int dg_sphere_adam_rows(const float* grad, long g_sb, long g_sk, float* latent, float* m, float* v, unsigned long long* step_dev,
                        unsigned* ticket, const float* noise_in, void* zT, int z_dtype, int B, int nz, const float* sched,
                        int num_step, float beta1, float beta2, float eps, int perturb, uint64_t seed, uint64_t stream_id,
                        int prime, int row0, void* stream);
int dg_depth_metrics(const float* inv_ref, const float* inv_gen, const float* mask, const float* keep, int kc,
                     int keep_is_depth, float tol, int B, long HW, float min_depth, float max_depth, float* out, void* stream);

/* ---- Multi-code GAN inversion (mGANprior)  demo.py:353-366, 466-488, 523-530 ------------------------------------------------
 * N latents per scan run through the generator's lower layers; their feature maps at one layer - pixel-major
 * [sample][P pixels][C channels] in `dtype` (DG_F32 / DG_BF16), code n of scan s = lower-batch row s N + n - are blended per
 * channel with alpha [B,N,C] fp32 and the blend runs on as one sample.
 * dg_feat_compose: out[s,p,c] = sum_n alpha[s,n,c] a[s N + n,p,c], accumulated in fp32 in code order, rounded once on the store.
 * dg_feat_compose_bwd: from g [B,P,C] = d loss / d out (NO leaky-relu factor in it):
 *   dpre[s N + n,p,c] = g[s,p,c] alpha[s,n,c] f(a[s N + n,p,c]),  f(x) = sqrt(2) for x > 0, else 0.2 sqrt(2): the factor the conv
 *   kernels' DG_EPI_MASK epilogue takes from `aux` - the gradient w.r.t. the pre-activations of the lower rows;
 *   dalpha[s,n,c] = sum_p g[s,p,c] a[s N + n,p,c], fp32, in a fixed order: nchunk (1..P) workgroups per (s, n) leave partial sums in
 *   parts [B N][nchunk][C] and draw tickets [B N] (both zero on entry, left zero; not read when nchunk = 1); the last one adds the
 *   partials in chunk order.  Two launches on the same data give the same bits.
 * Any C, P; vector accesses where C % 4 == 0 (bf16: C % 8 == 0 for the widest) and the pointers are aligned.  P C < 2^31.
 * dg_alpha_adam: torch.optim.Adam (defaults) on alpha [n] with moments m, v at step index k = *step_dev, which it only READS:
 * launch it before the dg_sphere_adam of the same step, whose last workgroup advances the index.  sched [num_step + 1][3] as
 * dg_sphere_adam's (columns 0, 1: lr(k) / (1 - beta1^(k+1)), sqrt(1 - beta2^(k+1)); column 2 unused), row num_step beyond it. */
int dg_feat_compose(const void* a, const float* alpha, void* out, int dtype, int B, int N, int P, int C, void* stream);
int dg_feat_compose_bwd(const void* g, const void* a, const float* alpha, void* dpre, float* dalpha, float* parts,
                        unsigned* tickets, int nchunk, int dtype, int B, int N, int P, int C, void* stream);
int dg_alpha_adam(const float* grad, float* alpha, float* m, float* v, const unsigned long long* step_dev, const float* sched,
                  int num_step, float beta1, float beta2, float eps, long n, void* stream);

/* ---- Target corruptions of the restoration experiment  demo.py:71-137, 385-397 ------------------------------------------------
 * The demo corrupts the scan it inverts against and compares the inversion with the full scan.  Images are fp32 [B,1,H,W],
 * contiguous.
 * dg_corrupt_mask: out = mask row_keep[h] col_keep[w] (u < rate); row_keep [H], col_keep [W], u [B,H,W] are each optional
 *   (NULL: factor 1; `rate` is read only with u).  out == mask is allowed.  One body for dropout_noise (demo.py:71-74: a pixel
 *   is KEPT where u < rate), sparse_hlines / sparse_vlines (:77-88: rows / columns ::int(1 / rate)), random_lines (:91-95),
 *   corrupt_half (:98-101) and corrupt_quarter (:104-108); the caller builds the keep vectors.
 * dg_additive_noise: out = x + (noise strength), the product rounded to fp32 before the sum, never one FMA (:111-113:
 *   `randn_like(depth) * strength`, then `depth + noise`).  out == x is allowed.
 * dg_median3x3: kornia.filters.median_blur(x, (3, 3)) as closing calls it (:117): the 5th smallest of the nine taps, taps
 *   outside the image read as ZERO (not circular, not replicated).  out != x.
 * dg_hole_fill: the `while` loop of closing (:118-123) on x in place, per sample.  A sweep sets every pixel with x <= thresh
 *   (the reference's 1e-8) to the maximum of its 3x3 neighbourhood - centre included, taps outside the image ignored
 *   (F.max_pool2d pads with -inf) - and every pixel of sweep k reads the state after sweep k - 1 (Jacobi).  A sample stops when
 *   no hole is left, when a sweep filled nothing (no pixel of the sample exceeds thresh: the reference's loop never ends
 *   there; that sweep is discarded) and in any case after max(H, W) - 1 sweeps (at least one), within which a valid pixel
 *   reaches every other.  sweeps [B]: the sweeps that filled something; left [B]: the holes remaining (0, or H W for an
 *   all-hole sample, which comes back unchanged).  tmp: B H W floats of scratch (the second buffer of the sweeps), != x.  One
 *   workgroup per sample, no host read-back between sweeps.  H W <= 2^18, else DG_EUNSUPPORTED. */
int dg_corrupt_mask(const float* mask, const float* row_keep, const float* col_keep, const float* u, float rate, int B, int H,
                    int W, float* out, void* stream);
int dg_additive_noise(const float* x, const float* noise, float strength, long n, float* out, void* stream);
int dg_median3x3(const float* x, int B, int H, int W, float* out, void* stream);
int dg_hole_fill(float* x, float* tmp, int B, int H, int W, float thresh, int* sweeps, int* left, void* stream);

/* ---- the synthesis command (dusty_gan_amd/synthesis.py; csrc/synthesis.hip) -----------------------
 * dg_latent_walk: out[i] = walk(w_i, z0, z1) for i < n with w = torch.linspace(0, 1, n) in float32 (n = 1: w = 0);
 * z0, z1 [nz], out [n, nz].  mode 0 = lerp, 1 = slerp  utils/interp.py:4-16: slerp's angle comes from the normalised
 * endpoints, the un-normalised ones are blended.  Norms and dot product are reduced once per launch; arithmetic in
 * float64, rounded once per output (lerp's rows 0 and n - 1 are z0 and z1 exactly).  Endpoints on one line (|cos| = 1 in
 * float32) give non-finite rows under slerp.  n < 1, nz < 1 or an unknown mode: DG_EINVAL.
 * dg_export_points: generated inverse depth inv [B,1,H,W] (as dg_inv_to_xyz's `in`, with its from_tanh / drop_const /
 * tol) on the angle grid [2,H,W] -> out [B, H W, 4] float32 (16-byte aligned): for every scan b, out[b, 0:counts[b]]
 * holds one KITTI record (x, y, z, 0) in METRES per valid pixel, in row-major pixel order (ring 0 first, columns
 * ascending).  A pixel is valid by dg_inv_to_xyz's predicate and its coordinates are that function's `points` times
 * max_depth (one pixel body, csrc/inv_point.h).  Records at and beyond counts[b] are not written.  chunk_counts: workspace
 * of B * ceil(H W / DG_EXPORT_CHUNK) int32 (need not be initialised).  Two launches, no atomics: two calls give the same
 * bytes.  H W > 2^31 - 1: DG_EINVAL. */
#define DG_EXPORT_CHUNK 1024
int dg_latent_walk(const float* z0, const float* z1, int n, int nz, int mode, float* out, void* stream);
int dg_export_points(const float* inv, const float* angle, int B, int H, int W, int from_tanh, float min_depth,
                     float max_depth, float drop_const, float tol, int* chunk_counts, float* out, int* counts, void* stream);

/* ---- an arbitrary point cloud onto the range image (utils/lidar.py:70-107; csrc/points_depth.hip) -----
 * dg_points_to_depth: Coordinate.points_to_depth.  rec: B clouds of N records of `stride` (3 or 4) floats, rec_sb floats
 * between clouds (>= N stride), record = (x, y, z[, anything]) in UNIT space (metres / max_depth): KITTI (x, y, z, r)
 * records go in where they lie.  counts [B] int32 (nullable = N everywhere; clamped to [0, N]): records at and beyond
 * counts[b] are not read.  angle [2,H,W] fp32 (elevation, azimuth).  Per point d_u = |xyz|, d_m = d_u max_depth, w =
 * exp(-tau d_u) [min_depth < d_m < max_depth] (both strict), u = atan2(z, hypot(x, y)), v = atan2(y, x), id = the pixel
 * minimising (u - U)^2 + (v - V)^2 over all H W pixels, the LOWEST index on a tie (strict `<` over ascending indices);
 * the distance is formed from differences in fp32, the per-point quantities in double.  NO AZIMUTH WRAP-AROUND, as in the
 * reference: a pixel row ends half a pixel from +-pi, so a point across the seam is still nearest to the row's end pixel on
 * its own side.  Per pixel depth_2d = sum w d_m / (sum w + 1e-8), valid = depth_2d != 0, depth [B,H,W] fp32 = (depth_2d -
 * min_depth) / (max_depth - min_depth) where valid and drop_value elsewhere; valid [B,H,W] bytes 0 / 1.  (The reference's
 * line 104 calls a `minmax_norm` that does not exist; `normalize_minmax` is what is built.)  A point with a non-finite
 * coordinate takes no part, nor does the origin.  idx [B,N] int32 (nullable): the pixel of every point, -1 for one that
 * took no part (out of range, non-finite, at or beyond counts[b]).
 * acc: caller-owned u64 words [B,H W,2] = (sum w d_u, sum w) in 24.40 fixed point (dg_fix40), ZERO AT REST: all zeros
 * before the call, zeroed again by its second launch.  Integer atomics: depth, valid and idx are bit-identical for any
 * permutation of the points (idx permuted with them), eager or replayed from a graph.  Two launches (search + sums; finish).
 * Limits: H W <= 2^18 and N <= 2^18 (DG_EUNSUPPORTED above: the codec's range, as dg_chamfer_nn); 0 <= tau <= 16 (w >=
 * e^-16 = 2^-23, 17 bits above the 2^-40 quantum), 0 <= min_depth < max_depth finite, stride 3 or 4, B <= 65535, no NULL
 * but counts and idx: DG_EINVAL, nothing launched. */
int dg_points_to_depth(const float* rec, long rec_sb, int stride, const int* counts, int B, int N, const float* angle, int H,
                       int W, double min_depth, double max_depth, double tau, float drop_value, unsigned long long* acc,
                       float* depth, unsigned char* valid, int* idx, void* stream);

/* ---- ray-drop transfer: G's inferred drops applied to the cloud that was inverted (dusty_gan_amd/raydrop.py;
 * csrc/raydrop.hip).  The paper's use of the measurability head on simulated scans; the reference holds no
 * code for it.
 * dg_pixel_winner: win [B,H W] int32 = for every pixel the NEAREST of the points dg_points_to_depth binned into it (idx
 *   [B,N] as that call returned it; rec / rec_sb / stride / counts as given to it), -1 for a pixel without a point.  Nearest
 *   by d_u = |xyz| in double on the float32 coordinates (the per-point body of dg_points_to_depth, csrc/points_body.h)
 *   rounded once to float32; equal rounded ranges: the LOWEST point index.  An idx outside [0, H W) takes no part.  ws:
 *   caller-owned u64 words [B,H W], ZERO AT REST (all zeros before the call, zeroed again by its second launch); one
 *   integer atomic max per point on the complemented key (range bits << 32 | index): the same bits for any launch order,
 *   eager or replayed.  Two launches.  stride 3 or 4, B <= 65535, H W <= 2^31 - 1, no NULL but counts: DG_EINVAL.
 * dg_raydrop_keep: keep [B,K,H,W] uint8 = win >= 0 && mp && mi for K realisations of the drop.  conf [B,arch,H,W]: G's raw
 *   confidence logits (arch 1 dusty1: h1; 2 dusty2: h1, h2); mp / mi are head_px_fwd's (csrc/head_post.h) in eval mode:
 *   mp = sigmoid((h1 + noise) / tau) > 0.5, mi = h2 > 0 (dusty2; 1 otherwise).  noise_in [B,K,H W] when given; NULL:
 *   GumbelSigmoid.logistic_noise drawn from Philox - for scan first_index + b, realisation k, pixel p the element p of the
 *   dg_philox_logistic_dev draw of H W elements at counter offset (first_index + b) 2 ceil(H W / 4) with the stream word
 *   (stream_id | k << 32): the number does not depend on B, on K or on the batch a scan travels in.  stream_id < 2^32.
 *   noise_out (nullable) [B,K,H W]: the noise used.  With H W % 4 == 0 keep must be 4-byte and noise_out 16-byte aligned.
 *   One launch.  arch 1 or 2, tau > 0, B and K in 1..65535: else DG_EINVAL.
 * dg_raydrop_gather: for every (b, k), over the pixels p in row-major order with keep[b,k,p] != 0 and 0 <= win[b,p] < N:
 *   out_records[b,k,j] = the `stride` 32-bit words of record win[b,p] of rec (ANY buffer of the layout given: the caller's
 *   records in metres come back unchanged, bit for bit) with column 3 = 0 for stride 3; out_labels[b,k,j] =
 *   labels[b, win[b,p]] (labels [B,N] uint32 and out_labels both, or neither); out_index[b,k,j] = win[b,p]; j ascending
 *   from 0; out_counts[b,k] = the number of such pixels.  Outputs are [B,K,H W(,4)]; rows at and beyond the count are not
 *   written.  chunk_counts: workspace of B K ceil(H W / DG_EXPORT_CHUNK) int32 (need not be initialised).  Two launches, no
 *   atomics (dg_export_points' ordered compaction): two calls give the same bytes.  out_records 16-byte aligned. */
int dg_pixel_winner(const float* rec, long rec_sb, int stride, const int* counts, const int* idx, int B, int N, int H, int W,
                    unsigned long long* ws, int* win, void* stream);
int dg_raydrop_keep(const float* conf, int arch, const int* win, const float* noise_in, uint64_t seed, uint64_t stream_id,
                    uint64_t first_index, float eps, float tau, int B, int K, int H, int W, unsigned char* keep,
                    float* noise_out, void* stream);
int dg_raydrop_gather(const float* rec, long rec_sb, int stride, int N, const int* win, const unsigned char* keep,
                      const unsigned* labels, int B, int K, int H, int W, int* chunk_counts, float* out_records,
                      unsigned* out_labels, int* out_index, int* out_counts, void* stream);

/* ---- semantic labels on the range image, and label-driven object removal (dusty_gan_amd/datasets/labels.py,
 * dusty_gan_amd/removal.py; csrc/label_image.hip, csrc/object_removal.hip).  Integer work and bit-for-bit
 * copies only; no float atomics anywhere.
 * dg_scan_labels: the SemanticKITTI branch of process_point_clouds  process_kitti.py:120-131.  keys [S*H*W] u64 as
 *   dg_scan_project or dg_beam_project (same S, H, W, offsets) LEFT them; labels [N] uint32 = the raw `.label` words in the
 *   points' order; lut: 65536 bytes on the device, entry i = the class of raw id i, 255 = no such id.  sem [S,H,W] uint8 =
 *   lut[labels[offsets[s] + winner] & 0xFFFF], 0 for an empty cell; inst [S,H,W] uint16 (nullable) = labels >> 16 of the
 *   winner, 0 for an empty cell: the label of the very record the projection's `out` holds, under its tie rule.  status [S]
 *   int32, zeroed by the CALLER: status[s] |= 1 (integer atomic OR) when a winner of scan s has an id whose lut entry is 255
 *   (sem is 255 there).  One launch.  DG_EINVAL: a NULL pointer other than inst, S < 1, H or W < 1.
 * dg_label_resize: sem [B,Hs,Ws] uint8 -> out [B,H,W] uint8 with dg_scan_to_polar's NEAREST rule (csrc/nearest.h: src =
 *   min(floor(dst * float(in) / out), in - 1)), no flip.
 * dg_remove_mask: sem [B,H,W] uint8, valid [B,H,W] fp32 (non-zero = a measured pixel: the target's mask), table: 256 bytes on
 *   the device (non-zero = remove this class), r in 0..8.  remove [B,H,W] uint8 = 1 where any pixel q with |dh| <= r and
 *   |dw| <= r has valid[q] && table[sem[q]], else 0; columns wrap around (the azimuth is a ring), rows outside the image take
 *   no part.  class_pixels [B,256] uint32, zeroed by the CALLER and ADDED to: the valid pixels of every class before
 *   dilation (counted in LDS, one integer global atomic per non-zero bin per workgroup).  One launch.  B, H <= 65535.
 * dg_compose_removed: per pixel of [B,H,W]: tgt_inv / valid = the target's inverse depth and mask, gen_inv = the generated
 *   inverse depth, keep = the generated keep map (keep_is_depth 0: kept where keep != 0; 1: kept where keep > tol -
 *   evaluate_batch's two rules).  inv_out = tgt_inv's bits where !remove && valid, gen_inv's bits where remove && kept, +0
 *   elsewhere; source uint8 = 1 (measured), 2 (generated), 0 (empty) respectively; sem_out uint8 = sem, fill_label, 0.
 *   counts [B,3] int32, zeroed by the CALLER: removed = pixels with remove && valid, filled = pixels with source 2, in_front =
 *   filled pixels that were valid and whose gen_inv > tgt_inv (a background nearer than the object measured there).  One
 *   launch; integer atomics only.  fill_label 0..255, B <= 65535.
 * dg_cloud_remove: for every cloud b, over the records n < counts[b] (nullable = N; clamped to [0, N]) in input order, the
 *   records with idx[b,n] < 0, idx[b,n] >= H W (took no part in the image) or remove[b, idx[b,n]] == 0: out_records[b,j] =
 *   the `stride` 32-bit words of record n of rec, bit for bit, column 3 = 0 for stride 3; out_labels[b,j] = labels[b,n]
 *   (labels [B,N] uint32 and out_labels both, or neither); out_index[b,j] = n; j ascending from 0; out_counts[b] = their
 *   number.  idx [B,N] as dg_points_to_depth returned it, remove [B,H W].  Outputs are [B,N(,4)]; rows at and beyond the count
 *   are not written.  chunk_counts: workspace of B ceil(N / DG_EXPORT_CHUNK) int32 (need not be initialised).  Two launches,
 *   no atomics (csrc/compact.h over records): two calls give the same bytes.  out_records 16-byte aligned. */
int dg_scan_labels(const unsigned long long* keys, const long* offsets, const unsigned* labels, const unsigned char* lut, int S,
                   int H, int W, unsigned char* sem, unsigned short* inst, int* status, void* stream);
int dg_label_resize(const unsigned char* sem, int B, int Hs, int Ws, int H, int W, unsigned char* out, void* stream);
int dg_remove_mask(const unsigned char* sem, const float* valid, const unsigned char* table, int B, int H, int W, int r,
                   unsigned char* remove, unsigned* class_pixels, void* stream);
int dg_compose_removed(const float* tgt_inv, const float* valid, const float* gen_inv, const float* keep, int keep_is_depth,
                       float tol, const unsigned char* remove, const unsigned char* sem, int fill_label, int B, int H, int W,
                       float* inv_out, unsigned char* source, unsigned char* sem_out, int* counts, void* stream);
int dg_cloud_remove(const float* rec, long rec_sb, int stride, const int* counts, const int* idx, const unsigned char* remove,
                    const unsigned* labels, int B, int N, int H, int W, int* chunk_counts, float* out_records,
                    unsigned* out_labels, int* out_index, int* out_counts, void* stream);

const char* dg_version(void);

#ifdef __cplusplus
}
#endif
#endif
