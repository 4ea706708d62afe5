// The streamed first-minimum search of the point-set kernels (gfx950), written once: chamfer_dir_kernel and chamfer_nn_kernel
// (point_chamfer.hip, 3-D points) and points_search_kernel (points_depth.hip, 2-D angles) are built from these bodies.
//   * A lane keeps PT query points in registers as PT / 2 packed pairs per coordinate, p[c][h], and their running minima rmin[h].
//   * The workgroup streams the m targets through two LDS buffers of MC entries (float4 for 3-D, float2 for 2-D); every lane reads
//     the SAME entry (broadcast).  The next chunk's global loads are issued before the math and stored to LDS after it.  The tail
//     of the last chunk repeats target 0: no effect on a minimum, and chunk 0 holds it first, so none on the first minimum either.
//   * A distance is formed from DIFFERENCES: d = d0 d0, then one fma per further coordinate in coordinate order - packed in the
//     stream (nn_chunk_min), scalar in nn_dist, the same operations in the same order: the same bits.
//   * The stream tracks the minimum only.  Per point and chunk ONE strict compare notes the chunk in which the running minimum
//     last fell, i.e. the FIRST chunk that attains the final minimum (nn_stream_first); the lane then rescans that chunk from
//     global memory with strict `<` over ascending indices (nn_first_in_chunk).  The LOWEST index attaining the minimum wins: the
//     project's tie rule (the reference's nnsearch, chamfer_distance.cu, and torch.argmin).
// `load(k, v)` is the caller's read of target k (0 <= k < m) from global memory into v[DIM], with the caller's strides.
#pragma once

typedef float f2 __attribute__((ext_vector_type(2)));

template <int DIM> struct nn_entry;
template <> struct nn_entry<3> { typedef float4 type; };
template <> struct nn_entry<2> { typedef float2 type; };
__device__ __forceinline__ float4 nn_pack(const float (&v)[3]) { return make_float4(v[0], v[1], v[2], 0.f); }
__device__ __forceinline__ float2 nn_pack(const float (&v)[2]) { return make_float2(v[0], v[1]); }
__device__ __forceinline__ void nn_unpack(const float4& q, float (&v)[3]) { v[0] = q.x; v[1] = q.y; v[2] = q.z; }
__device__ __forceinline__ void nn_unpack(const float2& q, float (&v)[2]) { v[0] = q.x; v[1] = q.y; }

// the chunk filler: chunk c of the targets into this thread's registers, and from there into one LDS buffer
template <int DIM, int MC, int THREADS, class Load>
__device__ __forceinline__ void nn_fetch(Load load, int c, int m, float (&r)[MC / THREADS][DIM]) {
#pragma unroll
  for (int u = 0; u < MC / THREADS; ++u) {
    const int k = c * MC + u * THREADS + threadIdx.x;
    load(k < m ? k : 0, r[u]);   // the tail of the last chunk repeats target 0
  }
}
template <int DIM, int MC, int THREADS>
__device__ __forceinline__ void nn_commit(const float (&r)[MC / THREADS][DIM], typename nn_entry<DIM>::type* chunk) {
#pragma unroll
  for (int u = 0; u < MC / THREADS; ++u) chunk[u * THREADS + threadIdx.x] = nn_pack(r[u]);
}

// the inner loop over one LDS chunk: rmin[h] = min(rmin[h], |chunk[t] - p[.][h]|^2) for every t
template <int DIM, int PT, int MC, int UNROLL>
__device__ __forceinline__ void nn_chunk_min(const typename nn_entry<DIM>::type* chunk, const f2 (&p)[DIM][PT / 2],
                                             f2 (&rmin)[PT / 2]) {
#pragma unroll UNROLL
  for (int t = 0; t < MC; ++t) {
    float v[DIM];
    nn_unpack(chunk[t], v);
#pragma unroll
    for (int h = 0; h < PT / 2; ++h) {
      // (the differences of the further coordinates are stated first: the results are the same bits in any order, and under this
      // one the compiler's schedule of the 2-D and the 3-D loop is no slower than either hand-written loop was - DESIGN.md 7j)
      f2 dc[DIM];
#pragma unroll
      for (int c = 1; c < DIM; ++c) dc[c] = (f2){v[c], v[c]} - p[c][h];
      dc[0] = (f2){v[0], v[0]} - p[0][h];
      f2 d = dc[0] * dc[0];
#pragma unroll
      for (int c = 1; c < DIM; ++c) d = __builtin_elementwise_fma(dc[c], dc[c], d);
      rmin[h][0] = __builtin_fminf(rmin[h][0], d[0]);
      rmin[h][1] = __builtin_fminf(rmin[h][1], d[1]);
    }
  }
}

// the scalar form of the stream's distance
template <int DIM>
__device__ __forceinline__ float nn_dist(const float (&q)[DIM], const float (&x)[DIM]) {
  const float d0 = q[0] - x[0];
  float d = d0 * d0;
#pragma unroll
  for (int c = 1; c < DIM; ++c) {
    const float dc = q[c] - x[c];
    d = __builtin_fmaf(dc, dc, d);
  }
  return d;
}

// The whole walk over ceil(m / MC) chunks, by all THREADS threads of the workgroup (two barriers' worth of LDS discipline: a
// buffer is written only after the barrier that ends its last reading).  Leaves in rmin the minima over all m targets and in
// wch[2 h + e] the first chunk that attains rmin[h][e].
template <int DIM, int PT, int MC, int THREADS, int UNROLL, class Load>
__device__ __forceinline__ void nn_stream_first(Load load, int m, typename nn_entry<DIM>::type (&qbuf)[2][MC],
                                                const f2 (&p)[DIM][PT / 2], f2 (&rmin)[PT / 2], int (&wch)[PT]) {
  const int nchunk = (m + MC - 1) / MC;
  float r[MC / THREADS][DIM];
#pragma unroll
  for (int h = 0; h < PT / 2; ++h) {
    rmin[h] = (f2){3.0e38f, 3.0e38f};
    wch[2 * h] = 0; wch[2 * h + 1] = 0;
  }
  nn_fetch<DIM, MC, THREADS>(load, 0, m, r);
  nn_commit<DIM, MC, THREADS>(r, qbuf[0]);
  __syncthreads();
  for (int c = 0; c < nchunk; ++c) {
    const int buf = c & 1;
    if (c + 1 < nchunk) nn_fetch<DIM, MC, THREADS>(load, c + 1, m, r);
    f2 was[PT / 2];
#pragma unroll
    for (int h = 0; h < PT / 2; ++h) was[h] = rmin[h];
    nn_chunk_min<DIM, PT, MC, UNROLL>(qbuf[buf], p, rmin);
#pragma unroll
    for (int h = 0; h < PT / 2; ++h) {
      if (rmin[h][0] < was[h][0]) wch[2 * h] = c;
      if (rmin[h][1] < was[h][1]) wch[2 * h + 1] = c;
    }
    if (c + 1 < nchunk) nn_commit<DIM, MC, THREADS>(r, qbuf[buf ^ 1]);
    __syncthreads();
  }
}

// the lowest index of chunk `chunk` whose nn_dist to x is strictly smallest
template <int DIM, int MC, class Load>
__device__ __forceinline__ int nn_first_in_chunk(Load load, int m, int chunk, const float (&x)[DIM]) {
  const int k0 = chunk * MC, k1 = min(m, k0 + MC);
  float best = 3.0e38f;
  int bi = k0;
  for (int k = k0; k < k1; ++k) {
    float q[DIM];
    load(k, q);
    const float d = nn_dist<DIM>(q, x);
    if (d < best) { best = d; bi = k; }
  }
  return bi;
}
