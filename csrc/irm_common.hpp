// What the fused held-out score passes on the arm-split fold panel share: csrc/irm.hip (the
// AIPW score of DML-IRM and its sensitivity, target and multi-split forms) and csrc/iivm.hip
// (the two AIPW scores of the LATE). What decides a row's score and the order of every sum
// lives here, once, so that the moments two passes have in common carry the same bits: the
// column read, the segment record, the ordered support compaction, the score itself, the
// per-workgroup partials and their fixed-order sum.
#pragma once
#include "common.hpp"

namespace ate {

template <typename T>
__device__ __forceinline__ double ld_col(const T* X, int64_t ld, int c, int64_t i) {
  return (double)X[(int64_t)c * ld + i];
}

struct Seg { int64_t r0, r1; };

// Ordered compaction (ascending j: the dot products keep the summation order of the dense
// loop, bit for bit) of the feature columns with a nonzero coefficient in any of NV
// interleaved vectors: cv[(1 + j) * NV + v], xc[j], compacted in place (q < return value);
// column j stays when any of its NV coefficients is nonzero. The whole block must call it.
template <int NV, typename C>
__device__ int compact_support_n(C* cv, int* xc, int p, int* wcnt /* [>= 16] */) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int base = 0;
  for (int j0 = 0; j0 < p; j0 += blockDim.x) {
    const int j = j0 + threadIdx.x;
    C val[NV];
    bool keep = false;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      val[v] = j < p ? cv[(int64_t)(1 + j) * NV + v] : C(0);
      keep = keep || val[v] != C(0);
    }
    const int c = j < p ? xc[j] : 0;
    const uint64_t m = __ballot(keep);
    if (lane == 0) wcnt[wid] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wid; ++w) off += wcnt[w];
    int tot = base;
    for (int w = 0; w < nw; ++w) tot += wcnt[w];
    const int pos = off + __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();                                      // all reads of the dense slots done
    ATE_DASSERT(pos <= j);                                // compaction only moves entries down
    if (keep) {
#pragma unroll
      for (int v = 0; v < NV; ++v) cv[(int64_t)(1 + pos) * NV + v] = val[v];
      xc[pos] = c;
    }
    __syncthreads();
    base = tot;
  }
  return base;
}

// the AIPW score of one valid row (everything after the three dot products, fp64)
__device__ __forceinline__ double irm_psi(double y, double w, double g0, double g1, double m,
                                          double clip) {
  const double lo = clip, hi = 1.0 - clip;
  const double e = m < lo ? lo : (m > hi ? hi : m);
  const double r1 = y - g1, r0 = y - g0;
  return g1 - g0 + w * r1 / e - (1.0 - w) * r0 / (1.0 - e);
}

template <int N>
__device__ __forceinline__ void write_partial(double (&v)[N], double* red, double* partial) {
  block_sum<N>(v, red);
  if (threadIdx.x == 0) {
    double* out = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * N;
#pragma unroll
    for (int q = 0; q < N; ++q) out[q] = v[q];
  }
}

// one block of 256 threads: thread i sums partials i, i+256, ... (fixed order), then a
// fixed-shape block reduction -> deterministic for a given launch geometry (the N-moment
// sibling of csrc/dml.hip sum7_kernel)
template <int N>
__global__ __launch_bounds__(256) void irm_sum_kernel(const double* __restrict__ partial, int nb,
                                                      double* __restrict__ out) {
  __shared__ double red[16 * N];
  double v[N] = {};
  for (int b = threadIdx.x; b < nb; b += 256)
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] += partial[(int64_t)b * N + q];
  block_sum<N>(v, red);
  if (threadIdx.x == 0)
#pragma unroll
    for (int q = 0; q < N; ++q) out[q] = v[q];
}

}  // namespace ate
