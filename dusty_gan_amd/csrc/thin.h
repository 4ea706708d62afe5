// The thin family (conv_thin.hip): one pick per pass - the kernel that runs, its template arguments and launch geometry,
// and what the engine sizes buffers from - made once per descriptor and consumed by plan and launch alike (api.hip), and
// the launchers of the kernel files (thin_valu.hip, thin_wgrad_mfma.hip, thin_up_mfma.hip, thin_s2_mfma.hip), which turn a
// pick into <<<>>> and compute no geometry of their own.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 tw_bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 tw_bf16x4;
typedef __attribute__((ext_vector_type(16))) float tw_f32x16;
typedef __attribute__((ext_vector_type(4))) float tw_f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned tw_u32x4;

// tile sizes the picks share with the kernels
#define SK_PX 64         // thin_smallk: pixels of a column tile
#define SN_PX 64         // thin_smalln
#define TU_PX 64         // thin_up_mfma: pixels of a column tile, image rows of a block's segment
#define TU_RS 8
#define WG_ROWS_PB 2     // thin_wgrad_down_mfma: coarse rows per block (4 on large grids: ThinWgradPick.rows_pb)
#define WGU_ROWS_PB 2    // thin_wgrad_up_mfma
extern const int thin_s2_mfma_cap;   // thin_s2_mfma's grid cap (S2_CAP of thin_s2_mfma.hip, a compile-time switch of that file)

enum ThinConvKernel { THIN_CONV_NONE, THIN_SMALLK, THIN_SMALLN, THIN_UP_MFMA, THIN_S2_MFMA };
struct ThinConvPick {
  ThinConvKernel kernel;
  int ta, tb;        // template arguments: SMALLK <KMAX>, SMALLN <in_dtype, N>, UP_MFMA <X2>, S2_MFMA <CP, MB>
  long grid;         // workgroups per launch (SMALLK: one launch per 64 output channels)
  size_t lds;        // dynamic LDS bytes (SMALLN)
  int tiles_x;       // SMALLK, UP_MFMA, S2_MFMA: column tiles of a row
  int nseg;          // UP_MFMA: row segments of a sample
  long ntiles;       // S2_MFMA
  int thin_mfma, mask_bits, dbias_rows, sum_parts;   // DgConvPlan's fields of the same names
};
int thin_conv_pick(const ConvP* p, ThinConvPick* k);   // DG_OK, or DG_EUNSUPPORTED (kernel = THIN_CONV_NONE)
int thin_conv_launch(const ConvP* p, const ThinConvPick& k, hipStream_t s);

enum ThinWgradKernel { THIN_WGRAD_NONE, THIN_WGRAD_DOWN_VALU, THIN_WGRAD_UP_VALU, THIN_WGRAD_DOWN_MFMA, THIN_WGRAD_UP_MFMA };
struct ThinWgradPick {
  ThinWgradKernel kernel;
  int ta;            // template argument: DOWN_VALU <CMAX>, DOWN_MFMA <NPT>, UP_MFMA <NP>
  int rows_pb;       // DOWN_MFMA: coarse rows per block
  int passes;        // launches: 64-channel slices (VALU), pairs of gradient channels (UP_MFMA <1>)
  unsigned grid;     // workgroups per launch
  size_t lds;        // dynamic LDS bytes
  int splits;        // partial tiles of the workspace form (DgWgrad.ws: one per block), 0: this call's launch has none
  bool takes_gmod;   // the kernel honours DgWgrad.g_mod
};
int thin_wgrad_pick(const WgradP* p, ThinWgradPick* k);   // DG_OK, or DG_EUNSUPPORTED (kernel = THIN_WGRAD_NONE)
int thin_wgrad_launch(const WgradP* p, const ThinWgradPick& k, hipStream_t s);

// the kernel files' launchers
int thin_conv_valu_launch(const ConvP* p, const ThinConvPick& k, hipStream_t s);     // SMALLK, SMALLN
int thin_up_mfma_launch(const ConvP* p, const ThinConvPick& k, hipStream_t s);
int thin_s2_mfma_launch(const ConvP* p, const ThinConvPick& k, hipStream_t s);
int thin_wgrad_valu_launch(const WgradP* p, const ThinWgradPick& k, hipStream_t s);  // DOWN_VALU, UP_VALU
int thin_wgrad_mfma_launch(const WgradP* p, const ThinWgradPick& k, hipStream_t s);  // DOWN_MFMA, UP_MFMA

// One kernel instantiation: the opt-in to more than the default 64 KiB of dynamic LDS and the launch come from the same
// function pointer, so a launcher chooses the template arguments once.
template <typename T> struct thin_arg { typedef T type; };
template <typename... A>
inline int thin_launch(void (*fn)(A...), long grid, size_t lds, hipStream_t s, typename thin_arg<A>::type... a) {
  if (lds > 64 * 1024) HIP_CHECK_RET(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  fn<<<(unsigned)grid, 256, lds, s>>>(a...);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}
