// What feeds a training step: the Philox4x32-10 draws (latents, Gumbel logistic noise, DiffAugment parameters), the
// device-resident counters behind them, the resident scan store's gather, and the step prologue - one launch that zero-fills,
// draws and fetches the real batch.  Every draw has ONE body; its stand-alone entry points and the prologue's blocks run it.
#include "step_inputs.h"
#include "pointwise.h"   // (nblk, sum_chunk)

// (philox4x32_10: common.h)
// raw bits: out[4*i + j] = philox(seed, counter = (offset + i, stream))[j]
__global__ void philox_bits_kernel(uint64_t seed, uint64_t stream, uint64_t offset, long n4, uint32_t* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  uint32_t r[4];
  philox4x32_10(seed, offset + (uint64_t)i, stream, r);
  out[4 * i + 0] = r[0]; out[4 * i + 1] = r[1]; out[4 * i + 2] = r[2]; out[4 * i + 3] = r[3];
}

// ---- the draws.  Their Philox offset is (offp ? *offp : 0) + base: a device-resident counter, so that a whole training step can
//      be captured once in a hipGraph and replayed (a host-side offset would be frozen in the captured kernel arguments), plus
//      what the host knows - the whole offset for the host-offset entry points, the share of earlier draws of a prologue.
__device__ __forceinline__ uint64_t draw_offset(const unsigned long long* offp, uint64_t base) { return (offp ? *offp : 0ull) + base; }

// group i of 4 outputs, from Philox counter offset + i:
// kind 0: uniform in [0,1) with 24 bits (bits >> 8) * 2^-24
// kind 1: standard normal by Box-Muller on pairs (u in (0,1]: 1 - uniform)
// kind 2: uniform(lo,hi)
// kind 3: integer in [ilo, ihi) as int32 (modulo of the 32-bit draw; range << 2^32 so the bias is < 2^-20)
__device__ __forceinline__ void philox_fill_body(uint64_t seed, uint64_t stream, uint64_t offset, int kind, float lo, float hi,
                                                 int ilo, int ihi, long n, void* __restrict__ out, bf16* __restrict__ out_bf16,
                                                 long i) {
  if (4 * i >= n) return;
  uint32_t r[4];
  philox4x32_10(seed, offset + (uint64_t)i, stream, r);
  const float s24 = 1.f / 16777216.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long o = 4 * i + j;
    if (o >= n) break;
    if (kind == 3) {
      ((int*)out)[o] = ilo + (int)(r[j] % (uint32_t)(ihi - ilo));
    } else if (kind == 1) {
      const int a = j & ~1;
      const float u1 = 1.f - (float)(r[a] >> 8) * s24, u2 = (float)(r[a + 1] >> 8) * s24;
      const float rad = sqrtf(-2.f * logf(u1));
      const float v = (j & 1) ? rad * sinf(6.283185307179586f * u2) : rad * cosf(6.283185307179586f * u2);
      ((float*)out)[o] = v;
      if (out_bf16) out_bf16[o] = (bf16)v;
    } else {
      const float u = (float)(r[j] >> 8) * s24;
      const float v = kind == 2 ? lo + (hi - lo) * u : u;
      ((float*)out)[o] = v;
      if (out_bf16) out_bf16[o] = (bf16)v;
    }
  }
}
__global__ void philox_fill_dev_kernel(uint64_t seed, uint64_t stream, const unsigned long long* __restrict__ offp, uint64_t base,
                                       int kind, float lo, float hi, int ilo, int ihi, long n, void* __restrict__ out) {
  philox_fill_body(seed, stream, draw_offset(offp, base), kind, lo, hi, ilo, ihi, n, out, nullptr,
                   (long)blockIdx.x * blockDim.x + threadIdx.x);
}
// (philox_logistic_body, GumbelSigmoid.logistic_noise straight from the generator: step_inputs.h - raydrop.hip draws with it too)
__global__ void philox_logistic_dev_kernel(uint64_t seed, uint64_t stream, const unsigned long long* __restrict__ offp,
                                           float eps, long n, float* __restrict__ out) {
  philox_logistic_body(seed, stream, *offp, eps, n, out, (long)blockIdx.x * blockDim.x + threadIdx.x);
}
// logistic noise of GumbelSigmoid from two uniform fields
__global__ void logistic_noise_kernel(const float* __restrict__ u1, const float* __restrict__ u2, float eps, long n,
                                      float* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = -logf(logf(u1[i] + eps) / logf(u2[i] + eps) + eps);
}

// One DiffAugment parameter set per sample (utils/diff_augment.py:27-28,36-38,46-48,59-60,86-87): three
// uniform(-1,1) draws and four integer draws, from two Philox counters per sample.
struct AugGeom { int sh, sw, nx, ny; };   // translation half-ranges, cutout offset ranges
__host__ __device__ __forceinline__ AugGeom aug_geom(int H, int W) {
  const int sh = (int)(H * (1.0 / 8.0) / 2 + 0.5), sw = (int)(W * (1.0 / 8.0) / 2 + 0.5);  // diff_augment.py:58
  const int ch = (int)(H * 0.5 + 0.5), cw = (int)(W * 0.5 + 0.5);                          // diff_augment.py:85
  return {sh, sw, H + (1 - ch % 2), W + (1 - cw % 2)};
}
__device__ __forceinline__ void aug_draw_body(uint64_t seed, uint64_t stream, uint64_t offset, int B, int sh, int sw, int nx,
                                              int ny, float* __restrict__ uf, int* __restrict__ qi, int b) {
  if (b >= B) return;
  uint32_t r0[4], r1[4];
  philox4x32_10(seed, offset + 2 * (uint64_t)b, stream, r0);
  philox4x32_10(seed, offset + 2 * (uint64_t)b + 1, stream, r1);
  const float s24 = 1.f / 16777216.f;
  for (int j = 0; j < 3; ++j) uf[j * B + b] = -1.f + 2.f * (float)(r0[j] >> 8) * s24;
  qi[0 * B + b] = -sh + (int)(r1[0] % (uint32_t)(2 * sh + 1));
  qi[1 * B + b] = -sw + (int)(r1[1] % (uint32_t)(2 * sw + 1));
  qi[2 * B + b] = (int)(r1[2] % (uint32_t)nx);
  qi[3 * B + b] = (int)(r1[3] % (uint32_t)ny);
}
// The gates of DiffAugment(policy, p < 1) (rand_translation / rand_cutout, utils/diff_augment.py:59,86: mask = bernoulli_(p)), AFTER
// the sample's seven numbers, which stay what they are: one more Philox block at the sample's FIRST counter under a stream of
// its own, DG_STREAM_AUG_GATE | the caller's stream id << 32 (two augmenters of one seed on different streams gate apart) - word 0 gates the translation, word 1 the cutout, ON iff u < p with u a 24-bit uniform in [0, 1), so p = 1 never
// gates a stage off and p = 0 always does.  A sample's gates depend on (seed, stream, its counter) alone.  Off: DG_AUG_OFF in t_h / o_x.
struct AugGate { int on; float p; const float* p_dev; };   // p_dev: p read when the draw runs (a captured step follows the memory)
__device__ __forceinline__ void aug_gate_body(uint64_t seed, uint64_t stream, uint64_t offset, int B, const AugGate& gt, int* __restrict__ qi, int b) {
  if (!gt.on || b >= B) return;
  const float p = gt.p_dev ? *gt.p_dev : gt.p;
  uint32_t r[4];
  philox4x32_10(seed, offset + 2 * (uint64_t)b, (uint64_t)DG_STREAM_AUG_GATE | (stream << 32), r);
  const float s24 = 1.f / 16777216.f;
  if (!((float)(r[0] >> 8) * s24 < p)) qi[0 * B + b] = DG_AUG_OFF;
  if (!((float)(r[1] >> 8) * s24 < p)) qi[2 * B + b] = DG_AUG_OFF;
}
__host__ __device__ __forceinline__ AugGate aug_gate(float p, const float* p_dev) { return {p_dev != nullptr || p != 1.f, p, p_dev}; }
__global__ void aug_draw_dev_kernel(uint64_t seed, uint64_t stream, const unsigned long long* __restrict__ offp, uint64_t base,
                                    int B, AugGeom g, AugGate gt, float* __restrict__ uf, int* __restrict__ qi) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t offset = draw_offset(offp, base);
  aug_draw_body(seed, stream, offset, B, g.sh, g.sw, g.nx, g.ny, uf, qi, b);
  aug_gate_body(seed, stream, offset, B, gt, qi, b);
}

// (dg_counter_add* advance a counter after its consumers, in stream order)
__global__ void counter_add_multi_kernel(CounterAdds a) {
  if (blockIdx.x == 0) counter_adds_body(a);
}

// batch `slab` of a resident store as {depth, mask}: V consecutive pixels of one sample per lane (V = 4: 16-byte accesses)
template <int V>
__global__ __launch_bounds__(256) void resident_gather_kernel(const float* __restrict__ store, long nslab, int B, long HW,
                                                              long slab, const unsigned char* __restrict__ flip,
                                                              float* __restrict__ depth, float* __restrict__ mask) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * HW / V) return;
  const long e = i * V, b = e / HW;
  const long var = flip ? (long)flip[b] : 0;
  const float* src = store + (var * nslab + slab) * (long)B * HW + e;   // sample (var, slab B + b), pixel e - b HW
  if constexpr (V == 4) {
    const float4 p = *(const float4*)src;
    *(float4*)(depth + e) = p;
    *(float4*)(mask + e) = make_float4(p.x > 0.f ? 1.f : 0.f, p.y > 0.f ? 1.f : 0.f, p.z > 0.f ? 1.f : 0.f, p.w > 0.f ? 1.f : 0.f);
  } else {
    const float p = *src;
    depth[e] = p;
    mask[e] = p > 0.f ? 1.f : 0.f;
  }
}

// fetch_reals, stand-alone (step_inputs.h: the pixel and the three forms of the source; the step prologue below runs the same
// fetch as blocks of its launch): block i owns `chunk` pixels of the batch, all of one sample.  kResident: a resident scan
// store, whose mask is pol > 0.  xsum != nullptr: per-sample sums of the result, one accumulator add per block (see
// head_post_fwd_kernel) - single floats strided by 256 per lane, then the block sum: the same order on every form of the
// source, so the sums of a resident fetch are dg_fetch_reals_sum's bits.  xsum == nullptr: chunk = 256, any pixel count.
template <bool kResident>
__device__ __forceinline__ float fetch_px_at(const float* __restrict__ pol, const float* __restrict__ mask, int k, const DgFetch& f) {
  const float p = pol[k];
  return fetch_real_px(p, kResident ? (p > 0.f ? 1.f : 0.f) : mask[k], f.min_depth, f.max_depth, f.drop_const);
}
template <bool kResident>
__device__ __forceinline__ float fetch_sum_sweep(const float* __restrict__ pol, const float* __restrict__ mask,
                                                 float* __restrict__ out, int chunk, const DgFetch& f) {
  float acc = 0.f;
#pragma unroll 4
  for (int k = threadIdx.x; k < chunk; k += 256) {               // (independent pixels: their loads in flight together)
    const float v = fetch_px_at<kResident>(pol, mask, k, f);
    out[k] = v;
    acc += v;
  }
  return acc;
}
template <bool kResident>
__global__ __launch_bounds__(256) void fetch_reals_kernel(DgFetch f, float* __restrict__ xsum, int chunk, const DgDet det) {
  __shared__ float red[16];
  const long i0 = (long)blockIdx.x * chunk, b = i0 / f.HW;
  const FetchSrc src = fetch_src<kResident>(f, b, i0 - b * f.HW);
  if (!xsum) {
    if (i0 + threadIdx.x < (long)f.B * f.HW) f.out[i0 + threadIdx.x] = fetch_px_at<kResident>(src.pol, src.mask, threadIdx.x, f);
    return;
  }
  const float sblk = dg_block_sum(fetch_sum_sweep<kResident>(src.pol, src.mask, f.out + i0, chunk, f), red);
  if (threadIdx.x == 0) dg_acc_add(&xsum[b], sblk, (unsigned)(f.HW / chunk), det);
}

// One launch for what a training step needs before its first real kernel: the zero-fill of the accumulator arena and the
// gradient buffers (dg_zero_multi) and every parameter draw of the step - latents (with their bfloat16 copy), Gumbel
// logistic noise, DiffAugment parameters - as extra blocks.  Four dependent launches of 4-8 us each otherwise.
struct PrologueZero { float* p[4]; long first[5]; int k; int blocks; };
struct PrologueDraws { DgDraw d[6]; int first_block[7]; int n; };
// fetch_reals as more blocks of the same launch (round 6): block j of the job owns pixels [j chunk, (j + 1) chunk) of the
// batch - chunk = HW / DG_XSUM_PARTS, so a sample is DG_XSUM_PARTS blocks - and STORES its partial sum to parts[j]: the
// per-sample sums DiffAugment's contrast needs leave as DG_XSUM_PARTS partials per sample, summed by the reader in a fixed
// order.  No accumulator that this very launch would have to zero first, no atomics.
struct PrologueFetch { DgFetch f; int first_block; int blocks; long chunk; };
// one fetch block's sweep of `chunk` pixels; kDerived: `mask` is not read, the validity is pol > 0.  (Not the stand-alone
// kernel's sweep above - single floats into an accumulator - on purpose: this one was tuned for the launch it rides on.)
template <bool kDerived>
__device__ __forceinline__ float prologue_fetch_sweep(const float* pol, const float* mask, float* out, long chunk,
                                                      const DgFetch& f) {
  float acc = 0.f;
  constexpr int U = 4;                                   // four trips' loads in flight per lane (8 x 16 bytes)
  for (long k0 = (long)threadIdx.x * 4; k0 < chunk; k0 += U * 1024) {
    float4 p4[U], m4[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long k = k0 + u * 1024;
      if (k < chunk) {
        p4[u] = *(const float4*)(pol + k);
        if (kDerived) {
          m4[u] = make_float4(p4[u].x > 0.f ? 1.f : 0.f, p4[u].y > 0.f ? 1.f : 0.f, p4[u].z > 0.f ? 1.f : 0.f,
                              p4[u].w > 0.f ? 1.f : 0.f);
        } else {
          m4[u] = *(const float4*)(mask + k);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long k = k0 + u * 1024;
      if (k >= chunk) break;
      float4 o;
      o.x = fetch_real_px(p4[u].x, m4[u].x, f.min_depth, f.max_depth, f.drop_const);
      o.y = fetch_real_px(p4[u].y, m4[u].y, f.min_depth, f.max_depth, f.drop_const);
      o.z = fetch_real_px(p4[u].z, m4[u].z, f.min_depth, f.max_depth, f.drop_const);
      o.w = fetch_real_px(p4[u].w, m4[u].w, f.min_depth, f.max_depth, f.drop_const);
      *(float4*)(out + k) = o;
      acc += (o.x + o.y) + (o.z + o.w);
    }
  }
  return acc;
}
// block j of the fetch: its DG_XSUM_PARTS-th of one sample, a contiguous run of that sample's image in every form of the source
template <bool kResident>
__device__ __forceinline__ float prologue_fetch_block(const DgFetch& f, int j, long chunk) {
  const FetchSrc src = fetch_src<kResident>(f, j / DG_XSUM_PARTS, (long)(j % DG_XSUM_PARTS) * chunk);
  return prologue_fetch_sweep<kResident>(src.pol, src.mask, f.out + (long)j * chunk, chunk, f);
}
__global__ __launch_bounds__(256) void step_prologue_kernel(PrologueZero z, PrologueDraws dr, PrologueFetch fe) {
  if (fe.blocks > 0 && (int)blockIdx.x >= fe.first_block) {
    __shared__ float red[16];
    const DgFetch& f = fe.f;
    const int j = (int)blockIdx.x - fe.first_block;
    const float acc = f.nslab > 0 ? prologue_fetch_block<true>(f, j, fe.chunk) : prologue_fetch_block<false>(f, j, fe.chunk);
    const float sblk = dg_block_sum(acc, red);
    if (threadIdx.x == 0) f.parts[j] = sblk;
    return;
  }
  if ((int)blockIdx.x < z.blocks) {
    const long stride = (long)z.blocks * 256, total = z.first[z.k];
    for (long i4 = (long)blockIdx.x * 256 + threadIdx.x; 4 * i4 < total; i4 += stride) {
      const long i = 4 * i4;
      int j = 0;
#pragma unroll
      for (int q = 1; q < 4; ++q)
        if (q < z.k && i >= z.first[q]) j = q;
      *(float4*)(z.p[j] + (i - z.first[j])) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return;
  }
  const int blk = (int)blockIdx.x - z.blocks;
  int j = 0;
  for (int q = 1; q < dr.n; ++q)
    if (blk >= dr.first_block[q]) j = q;
  const DgDraw& d = dr.d[j];
  const long i = (long)(blk - dr.first_block[j]) * 256 + threadIdx.x;
  const uint64_t offset = draw_offset(d.offset_dev, d.base);
  if (d.kind == 0) {
    philox_fill_body(d.seed, d.stream_id, offset, d.fill_kind, d.lo, d.hi, d.ilo, d.ihi, d.n, d.out, (bf16*)d.out_bf16, i);
  } else if (d.kind == 1) {
    philox_logistic_body(d.seed, d.stream_id, offset, d.eps, d.n, (float*)d.out, i);
  } else {
    const AugGeom g = aug_geom(d.H, d.W);
    aug_draw_body(d.seed, d.stream_id, offset, d.B, g.sh, g.sw, g.nx, g.ny, d.uf, d.qi, (int)i);
    aug_gate_body(d.seed, d.stream_id, offset, d.B, aug_gate(d.p, d.p_dev), d.qi, (int)i);
  }
}

extern "C" {

int dg_philox_bits(uint64_t seed, uint64_t stream, uint64_t offset, long n4, uint32_t* out, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  philox_bits_kernel<<<nblk(n4), 256, 0, s>>>(seed, stream, offset, n4, out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

static int fill_check(int kind, int ilo, int ihi) {
  return (kind < 0 || kind > 3 || (kind == 3 && ihi <= ilo)) ? DG_EINVAL : DG_OK;
}
static int philox_fill(uint64_t seed, uint64_t stream, const unsigned long long* offset_dev, uint64_t base, int kind, float lo,
                       float hi, int ilo, int ihi, long n, void* out, void* s_) {
  if (fill_check(kind, ilo, ihi) != DG_OK) return DG_EINVAL;
  philox_fill_dev_kernel<<<nblk((n + 3) / 4), 256, 0, (hipStream_t)s_>>>(seed, stream, offset_dev, base, kind, lo, hi, ilo, ihi, n,
                                                                         out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}
int dg_philox_fill(uint64_t seed, uint64_t stream, uint64_t offset, int kind, float lo, float hi, int ilo, int ihi,
                   long n, void* out, void* s_) {
  return philox_fill(seed, stream, nullptr, offset, kind, lo, hi, ilo, ihi, n, out, s_);
}
int dg_philox_fill_dev(uint64_t seed, uint64_t stream, const unsigned long long* offset_dev, int kind, float lo,
                       float hi, int ilo, int ihi, long n, void* out, void* s_) {
  return philox_fill(seed, stream, offset_dev, 0, kind, lo, hi, ilo, ihi, n, out, s_);
}

// logistic noise of n elements from the device-resident Philox offset; the caller advances the counter by 2 ((n + 3) / 4)
int dg_philox_logistic_dev(uint64_t seed, uint64_t stream, const unsigned long long* offset_dev, float eps, long n,
                           float* out, void* s_) {
  if (!offset_dev || !out || n <= 0) return DG_EINVAL;
  philox_logistic_dev_kernel<<<nblk((n + 3) / 4), 256, 0, (hipStream_t)s_>>>(seed, stream, offset_dev, eps, n, out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

int dg_logistic_noise(const float* u1, const float* u2, float eps, long n, float* out, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  logistic_noise_kernel<<<nblk(n), 256, 0, s>>>(u1, u2, eps, n, out);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

static bool aug_p_ok(float p) { return p >= 0.f && p <= 1.f; }   // (false for a NaN)
static int aug_draw(uint64_t seed, uint64_t stream, const unsigned long long* offset_dev, uint64_t base, int B, int H, int W,
                    float p, const float* p_dev, float* uf, int* qi, void* s_) {
  if (!uf || !qi || B <= 0 || H <= 0 || W <= 0 || !aug_p_ok(p)) return DG_EINVAL;
  aug_draw_dev_kernel<<<nblk(B), 256, 0, (hipStream_t)s_>>>(seed, stream, offset_dev, base, B, aug_geom(H, W), aug_gate(p, p_dev),
                                                            uf, qi);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}
int dg_aug_draw(uint64_t seed, uint64_t stream, uint64_t offset, int B, int H, int W, float* uf, int* qi, void* s_) {
  return aug_draw(seed, stream, nullptr, offset, B, H, W, 1.f, nullptr, uf, qi, s_);
}
int dg_aug_draw_dev(uint64_t seed, uint64_t stream, const unsigned long long* offset_dev, int B, int H, int W,
                    float* uf, int* qi, void* s_) {
  return aug_draw(seed, stream, offset_dev, 0, B, H, W, 1.f, nullptr, uf, qi, s_);
}
int dg_aug_draw_p(uint64_t seed, uint64_t stream, uint64_t offset, int B, int H, int W, float p, float* uf, int* qi, void* s_) {
  return aug_draw(seed, stream, nullptr, offset, B, H, W, p, nullptr, uf, qi, s_);
}
int dg_aug_draw_p_dev(uint64_t seed, uint64_t stream, const unsigned long long* offset_dev, int B, int H, int W,
                      const float* p_dev, float* uf, int* qi, void* s_) {
  if (!offset_dev || !p_dev) return DG_EINVAL;
  return aug_draw(seed, stream, offset_dev, 0, B, H, W, 1.f, p_dev, uf, qi, s_);
}

// k <= 8 DISTINCT counters advanced by one launch (one graph node instead of one per counter)
static int counter_add_multi(unsigned long long* const* counters, const unsigned long long* deltas, int k, int snap_idx,
                             const float* src, int n, float* dst_ring, int ring, void* s_) {
  CounterAdds a{};
  const int rc = fill_counter_adds(a, counters, deltas, k, snap_idx, src, n, dst_ring, ring);
  if (rc != DG_OK) return rc;
  counter_add_multi_kernel<<<1, 64, 0, (hipStream_t)s_>>>(a);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}
int dg_counter_add(unsigned long long* counter, unsigned long long delta, void* s_) {
  return counter_add_multi(&counter, &delta, 1, -1, nullptr, 0, nullptr, 1, s_);
}
int dg_counter_add_multi(unsigned long long* const* counters, const unsigned long long* deltas, int k, void* s_) {
  return counter_add_multi(counters, deltas, k, -1, nullptr, 0, nullptr, 1, s_);
}
// ... and slot (old value of counters[snap_idx]) % ring of `dst_ring` (n floats per slot; device memory or mapped pinned host
// memory) receives src[0..n): the step's logged scalars leave the device from the step's last launch - no copy node behind
// the graph, and the host reads slot i once an event recorded behind step i has completed, never blocking the launch stream
int dg_counter_add_multi_snap(unsigned long long* const* counters, const unsigned long long* deltas, int k, int snap_idx,
                              const float* src, int n, float* dst_ring, int ring, void* s_) {
  if (snap_idx < 0) return DG_EINVAL;
  return counter_add_multi(counters, deltas, k, snap_idx, src, n, dst_ring, ring, s_);
}

int dg_resident_gather(const float* store, long nslab, int B, long HW, long slab, const unsigned char* flip, float* depth,
                       float* mask, void* s_) {
  if (!store || !depth || !mask || nslab < 1 || B <= 0 || HW <= 0 || slab < 0 || slab >= nslab) return DG_EINVAL;
  hipStream_t s = (hipStream_t)s_;
  if (HW % 4 == 0 && (((size_t)store | (size_t)depth | (size_t)mask) & 15) == 0)
    resident_gather_kernel<4><<<nblk((long)B * HW / 4), 256, 0, s>>>(store, nslab, B, HW, slab, flip, depth, mask);
  else
    resident_gather_kernel<1><<<nblk((long)B * HW), 256, 0, s>>>(store, nslab, B, HW, slab, flip, depth, mask);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}

// the four stand-alone forms of fetch_reals: each names its source in a DgFetch (include/dusty_gan_hip.h) for one launcher.
// xsum != nullptr: xsum[b] += sum of out[b] over its HW pixels (xsum zeroed by the caller; HW % 256 == 0 or DG_EUNSUPPORTED)
static int fetch_reals_launch(DgFetch f, float min_depth, float max_depth, float drop_const, float* out, float* xsum, void* s_) {
  f.min_depth = min_depth; f.max_depth = max_depth; f.drop_const = drop_const; f.out = out;
  const int rc = fetch_check(f);
  if (rc != DG_OK) return rc;
  if (xsum && f.HW % 256 != 0) return DG_EUNSUPPORTED;
  const int chunk = xsum ? sum_chunk(f.HW) : 256;
  const unsigned grid = nblk((long)f.B * f.HW, chunk);
  const DgDet det = dg_det_current();
  if (f.nslab > 0) fetch_reals_kernel<true><<<grid, 256, 0, (hipStream_t)s_>>>(f, xsum, chunk, det);
  else fetch_reals_kernel<false><<<grid, 256, 0, (hipStream_t)s_>>>(f, xsum, chunk, det);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}
int dg_fetch_reals(const float* pol, const float* mask, float min_depth, float max_depth, float drop_const, long n,
                   float* out, void* s_) {
  DgFetch f{};
  f.pol = pol; f.mask = mask; f.B = 1; f.HW = n;
  return fetch_reals_launch(f, min_depth, max_depth, drop_const, out, nullptr, s_);
}
int dg_fetch_reals_sum(const float* pol, const float* mask, float min_depth, float max_depth, float drop_const, int B,
                       long HW, float* out, float* xsum, void* s_) {
  if (!xsum) return DG_EINVAL;
  DgFetch f{};
  f.pol = pol; f.mask = mask; f.B = B; f.HW = HW;
  return fetch_reals_launch(f, min_depth, max_depth, drop_const, out, xsum, s_);
}
// ... from a device-resident pool of `npool` batches: batch index = *pool_ctr % npool, read on the device
int dg_fetch_reals_pool_sum(const float* pol_pool, const float* mask_pool, const unsigned long long* pool_ctr, int npool,
                            float min_depth, float max_depth, float drop_const, int B, long HW, float* out, float* xsum,
                            void* s_) {
  if (!xsum || !pool_ctr) return DG_EINVAL;
  DgFetch f{};
  f.pol = pol_pool; f.mask = mask_pool; f.pool_ctr = pool_ctr; f.npool = npool; f.B = B; f.HW = HW;
  return fetch_reals_launch(f, min_depth, max_depth, drop_const, out, xsum, s_);
}
// ... from a resident scan store: the batch and each sample's stored variant picked on the device
int dg_fetch_reals_resident_sum(const float* store, const unsigned long long* pool_ctr, long nslab,
                                const unsigned char* flip_tab, float min_depth, float max_depth, float drop_const, int B,
                                long HW, float* out, float* xsum, void* s_) {
  if (!xsum || nslab < 1) return DG_EINVAL;
  DgFetch f{};
  f.pol = store; f.pool_ctr = pool_ctr; f.nslab = nslab; f.flip_tab = flip_tab; f.B = B; f.HW = HW;
  return fetch_reals_launch(f, min_depth, max_depth, drop_const, out, xsum, s_);
}

// zero-fill of k <= 4 fp32 buffers (as dg_zero_multi; k may be 0) + ndraw <= 6 draws (DgDraw) + optionally fetch_reals of one
// batch (DgFetch) in one launch
static int step_prologue_impl(float* const* ptrs, const long* counts, int k, const DgDraw* draws, int ndraw, const DgFetch* fetch,
                              void* s_) {
  if (k < 0 || k > 4 || ndraw < 0 || ndraw > 6 || (k && (!ptrs || !counts)) || (ndraw && !draws)) return DG_EINVAL;
  PrologueZero z{};
  long tot = 0;
  for (int i = 0; i < k; ++i) {
    if (!ptrs[i] || counts[i] < 0 || counts[i] % 4 != 0 || ((size_t)ptrs[i] & 15) != 0) return DG_EINVAL;
    z.p[i] = ptrs[i]; z.first[i] = tot;
    tot += counts[i];
  }
  z.first[k] = tot;
  z.k = k;
  unsigned zb = nblk(tot / 4);
  if (zb > 2048) zb = 2048;
  z.blocks = (int)zb;
  PrologueDraws dr{};
  long blocks = 0;
  for (int i = 0; i < ndraw; ++i) {
    const DgDraw& d = draws[i];
    if (!d.offset_dev) return DG_EINVAL;
    long threads;
    if (d.kind == 0) {
      if (!d.out || d.n <= 0 || fill_check(d.fill_kind, d.ilo, d.ihi) != DG_OK || (d.fill_kind == 3 && d.out_bf16)) return DG_EINVAL;
      threads = (d.n + 3) / 4;
    } else if (d.kind == 1) {
      if (!d.out || d.n <= 0) return DG_EINVAL;
      threads = (d.n + 3) / 4;
    } else if (d.kind == 2) {
      if (!d.uf || !d.qi || d.B <= 0 || d.H <= 0 || d.W <= 0 || !aug_p_ok(d.p)) return DG_EINVAL;
      threads = d.B;
    } else {
      return DG_EINVAL;
    }
    dr.d[i] = d;
    dr.first_block[i] = (int)blocks;
    blocks += (threads + 255) / 256;
    if (blocks > (1L << 30)) return DG_EUNSUPPORTED;
  }
  dr.first_block[ndraw] = (int)blocks;
  dr.n = ndraw;
  PrologueFetch fe{};
  if (fetch) {
    const DgFetch& f = *fetch;
    if (fetch_check(f) != DG_OK || !f.parts) return DG_EINVAL;
    // 16-byte accesses, whole 1024-pixel sweeps per block, DG_XSUM_PARTS blocks per sample
    if (f.HW % (1024L * DG_XSUM_PARTS) != 0 || (((size_t)f.pol | (size_t)(f.nslab > 0 ? nullptr : f.mask) | (size_t)f.out) & 15) != 0)
      return DG_EUNSUPPORTED;
    fe.f = f;
    fe.chunk = f.HW / DG_XSUM_PARTS;
    fe.blocks = f.B * DG_XSUM_PARTS;
    fe.first_block = (int)(zb + blocks);
  }
  if (zb + blocks + fe.blocks == 0) return DG_OK;
  step_prologue_kernel<<<(unsigned)(zb + blocks + fe.blocks), 256, 0, (hipStream_t)s_>>>(z, dr, fe);
  HIP_CHECK_RET(hipGetLastError());
  return DG_OK;
}
int dg_step_prologue(float* const* ptrs, const long* counts, int k, const DgDraw* draws, int ndraw, void* s_) {
  return step_prologue_impl(ptrs, counts, k, draws, ndraw, nullptr, s_);
}
int dg_step_prologue_fetch(float* const* ptrs, const long* counts, int k, const DgDraw* draws, int ndraw, const DgFetch* fetch,
                           void* s_) {
  if (!fetch) return DG_EINVAL;
  return step_prologue_impl(ptrs, counts, k, draws, ndraw, fetch, s_);
}

}  // extern "C"
