// Projection of per-row scores on a B-spline basis of one covariate, with the Rademacher
// multiplier bootstrap of the projected curve (CATE curves of DML-IRM with a uniform
// confidence band; estimators/cate.py).
//
// Basis: d functions of degree q <= 3 on a clamped knot vector t[0 .. d+q] (the boundary
// knots repeated q + 1 times, d - q - 1 strictly increasing interior knots). Span
// sp in [0, d - q) covers [t[q+sp], t[q+sp+1]), the last one closed on the right; a row in
// span sp has exactly the q + 1 non-zero basis values b_{sp} .. b_{sp+q}, evaluated in
// registers by the span-local Cox-de Boor recurrence (every denominator is a knot
// difference that contains the span, so nothing divides by zero).
//
// Pass 1 (ate_cate_moments): n | S psi | S psi^2 | rows per span | v = S b psi | M = S b b'.
// Pass 2 (ate_cate_boot), with e_i = psi_i - b_i' beta:
//   Meat = S e^2 b b',   T[r][j] = S xi_i^r e_i b_{i,j}
// with the Rademacher multipliers xi_i^r of csrc/boot_common.hpp (the draws, the bit ->
// replicate mapping, the launch geometry, the bucketing and the slab sum are shared with
// csrc/gate.hip there). Rows with rid < 0 are skipped (padding rows and rows the caller
// leaves out): they contribute exactly nothing.
//
// Shape (that of gate_boot_kernel): a workgroup of CH threads walks chunks of CH rows
// (blockIdx.x, grid stride). Per chunk one row per thread is loaded and evaluated, the rows
// are bucketed by span with a stable counting sort (bucket_rows) and
// a record (b_0..b_3 or e b_0..e b_3, zero above q) per row is written to LDS in bucket order.
//  - Band sums (count, v, M; Meat): thread t owns function t % 16 of span t / 16 (+ CH / 16 per
//    pass) -- 1, b_c psi (4), b_a b_c for a <= c (10) -- and walks that span's run with one
//    accumulator in a register. Only the band |j - k| <= q of M exists; the sum kernel adds the
//    spans' local blocks into the full symmetric matrix.
//  - Replicate sums: thread t owns bit t % 32 of the four words of Philox stream t / 32 (four
//    replicates) and walks each span's run with (q + 1) x 4 fp64 accumulators; the span loop is
//    wave-uniform, so for d <= 8 the d x 4 sums of the basis slots stay in registers for the
//    whole kernel (the loop is unrolled), above that they live in the thread's own slots of
//    the workgroup's partial slab.
// No atomics: per-workgroup partials, combined in a fixed order by the sum kernels, so one
// launch geometry gives one set of bits.
#include "boot_common.hpp"

using namespace ate;

namespace {

constexpr int DREG = 8;      // up to this many basis functions: replicate sums in registers
constexpr int DMAX = 32;     // basis functions (and so spans) at most
constexpr int QMAX = 3;
constexpr int NF = 16;       // band functions per span (15 in use)
constexpr int REC = 6;       // doubles per bucketed row: r_0..r_3 | psi | 1
constexpr int NPASS = 8;     // band passes at most: DMAX spans / (64 / NF)

// span of x (the number of interior knots at or below it: exact fp64 compares) and its
// q + 1 non-zero basis values N[0..Q] = b_sp .. b_{sp+Q}; N above Q is 0
template <int Q>
__device__ __forceinline__ int basis_eval(const double* sk, int d, double x, double (&N)[QMAX + 1]) {
  int sp = 0;
  for (int j = Q + 1; j < d; ++j) sp += sk[j] <= x ? 1 : 0;
  ATE_DASSERT(sp >= 0 && sp < d - Q);
  const int s = Q + sp;
  N[0] = 1.0;
#pragma unroll
  for (int j = 1; j <= QMAX; ++j) N[j] = 0.0;
#pragma unroll
  for (int j = 1; j <= Q; ++j) {
    double saved = 0.0;
#pragma unroll
    for (int r = 0; r < j; ++r) {
      const double hi = sk[s + r + 1], lo = sk[s + r + 1 - j];
      const double temp = N[r] / (hi - lo);
      N[r] = saved + (hi - x) * temp;
      saved = (x - lo) * temp;
    }
    N[j] = saved;
  }
  return sp;
}

__device__ __forceinline__ int basis_eval_q(int q, const double* sk, int d, double x,
                                            double (&N)[QMAX + 1]) {
  switch (q) {
    case 0: return basis_eval<0>(sk, d, x, N);
    case 1: return basis_eval<1>(sk, d, x, N);
    case 2: return basis_eval<2>(sk, d, x, N);
    default: return basis_eval<3>(sk, d, x, N);
  }
}

// the two record entries whose product is band function k: 0 -> 1, 1..4 -> r_c psi,
// 5..14 -> r_a r_c (a <= c, row-major), 15 -> unused
__device__ __forceinline__ void band_fn(int k, int& ia, int& ic) {
  ia = 5; ic = 5;
  if (k >= 1 && k <= 4) { ia = k - 1; ic = 4; }
  if (k >= 5 && k < 15) {
    int kk = k - 5, a = 0;
    while (kk >= 4 - a) { kk -= 4 - a; ++a; }
    ia = a; ic = a + kk;
  }
}
__host__ __device__ inline int band_slot(int a, int c) {      // a <= c
  return 5 + a * 4 - a * (a - 1) / 2 + (c - a);
}

// this thread's band function over the runs of its spans, one register per pass
__device__ __forceinline__ void band_accumulate(const double* rec, const int* start, int nsp,
                                                int ia, int ic, double (&acc)[NPASS]) {
  const int spp = blockDim.x >> 4, g = threadIdx.x >> 4;
#pragma unroll
  for (int p = 0; p < NPASS; ++p) {
    const int sp = p * spp + g;
    if (sp < nsp) {
      const int r0 = start[sp], r1 = start[sp + 1];
      double a = acc[p];
      for (int r = r0; r < r1; ++r) a = fma(rec[r * REC + ia], rec[r * REC + ic], a);
      acc[p] = a;
    }
  }
}

// PB [bx][DMAX][NF]
__device__ __forceinline__ void band_store(double* __restrict__ PB, int nsp,
                                           const double (&acc)[NPASS]) {
  const int spp = blockDim.x >> 4, g = threadIdx.x >> 4, k = threadIdx.x & 15;
#pragma unroll
  for (int p = 0; p < NPASS; ++p) {
    const int sp = p * spp + g;
    if (sp < nsp) {
      ATE_DASSERT(sp < DMAX);
      PB[((int64_t)blockIdx.x * DMAX + sp) * NF + k] = acc[p];
    }
  }
}

// ---------------------------------------------------------------- pass 1
// PB [nbx][DMAX][NF], PS [nbx][2] = (S psi, S psi^2)
__global__ __launch_bounds__(CHMAX) void cate_moments_kernel(
    const double* __restrict__ psi, const double* __restrict__ x, const int64_t* __restrict__ rid,
    int64_t ld, const double* __restrict__ knots, int d, int q, double* __restrict__ PB,
    double* __restrict__ PS) {
  __shared__ __attribute__((aligned(16))) double rec[CHMAX * REC];
  __shared__ double sk[DMAX + QMAX + 1];
  __shared__ double red[16 * 2];
  __shared__ int wcnt[CHMAX / 64][DMAX];
  __shared__ int start[DMAX + 1];
  const int CH = blockDim.x, t = threadIdx.x, nsp = d - q;
  ATE_DASSERT(d >= q + 1 && d <= DMAX && q >= 0 && q <= QMAX && CH <= CHMAX && (CH & 63) == 0);
  if (t < d + q + 1) sk[t] = knots[t];
  int ia, ic;
  band_fn(t & 15, ia, ic);
  double acc[NPASS];
#pragma unroll
  for (int p = 0; p < NPASS; ++p) acc[p] = 0.0;
  double m[2] = {0.0, 0.0};
  __syncthreads();
  const int64_t nchunk = (ld + CH - 1) / CH;
  for (int64_t ck = blockIdx.x; ck < nchunk; ck += gridDim.x) {
    const int64_t i = ck * CH + t;
    const bool valid = i < ld && rid[i] >= 0;
    const double p = valid ? psi[i] : 0.0;
    double N[QMAX + 1];
    const int g = basis_eval_q(q, sk, d, valid ? x[i] : sk[0], N);
    m[0] += p;
    m[1] += p * p;
    const int pos = bucket_rows<DMAX>(valid, g, wcnt, start);
    if (valid) {
#pragma unroll
      for (int c = 0; c <= QMAX; ++c) rec[pos * REC + c] = N[c];
      rec[pos * REC + 4] = p;
      rec[pos * REC + 5] = 1.0;
    }
    __syncthreads();
    band_accumulate(rec, start, nsp, ia, ic, acc);
  }
  band_store(PB, nsp, acc);
  block_sum<2>(m, red);
  if (t == 0) {
    PS[(int64_t)blockIdx.x * 2 + 0] = m[0];
    PS[(int64_t)blockIdx.x * 2 + 1] = m[1];
  }
}

// Band partials of all workgroups into TOT [DMAX][NF] | S psi | S psi^2: workgroup sp < nsp
// sums span sp (thread (k, sl) adds the workgroups sl, sl + 16, ... of function k in ascending
// order, the 16 slices are then added in slice order); with PS, workgroup nsp sums the two
// score moments the same way over 128 slices.
__global__ __launch_bounds__(256) void cate_band_reduce_kernel(
    const double* __restrict__ PB, const double* __restrict__ PS, int nbx, int nsp,
    double* __restrict__ TOT) {
  __shared__ double part[256];
  const int t = threadIdx.x, sp = blockIdx.x;
  const int w = sp < nsp ? NF : 2, k = t % w, sl = t / w, nsl = 256 / w;
  const double* src = sp < nsp ? PB + (int64_t)sp * NF + k : PS + k;
  const int64_t stride = sp < nsp ? DMAX * NF : 2;
  double a = 0.0;
#pragma unroll 8
  for (int bx = sl; bx < nbx; bx += nsl) a += src[(int64_t)bx * stride];
  part[t] = a;
  __syncthreads();
  if (sl != 0) return;
  for (int s2 = 1; s2 < nsl; ++s2) a += part[s2 * w + k];
  TOT[(sp < nsp ? sp * NF : DMAX * NF) + k] = a;
}

// The spans' local blocks into the outputs, in ascending span order.
//   moments: out = n | S psi | S psi^2 | count [nsp] | v [d] | M [d][d]
//   boot:    out = Meat [d][d]
__global__ __launch_bounds__(256) void cate_band_out_kernel(const double* __restrict__ TOT,
                                                            bool mom, int d, int q,
                                                            double* __restrict__ out) {
  __shared__ double tot[DMAX][NF];
  const int t = threadIdx.x, nsp = d - q;
  for (int o = t; o < nsp * NF; o += 256) (&tot[0][0])[o] = TOT[o];
  __syncthreads();
  double* M = out;
  if (mom) {
    double* cnt = out + 3;
    double* v = cnt + nsp;
    M = v + d;
    if (t == 0) {
      double n = 0.0;
      for (int sp = 0; sp < nsp; ++sp) n += tot[sp][0];
      out[0] = n;
    }
    if (t == 1 || t == 2) out[t] = TOT[DMAX * NF + t - 1];
    if (t < nsp) cnt[t] = tot[t][0];
    if (t >= 64 && t < 64 + d) {
      const int j = t - 64;
      double a = 0.0;
      for (int sp = (j - q > 0 ? j - q : 0); sp <= j && sp < nsp; ++sp) a += tot[sp][1 + (j - sp)];
      v[j] = a;
    }
  }
  for (int o = t; o < d * d; o += 256) {
    const int r = o / d, c = o % d;
    const int j = r < c ? r : c, h = r < c ? c : r;      // (j, h), j <= h: the mirror's bits
    double a = 0.0;
    if (h - j <= q)
      for (int sp = (h - q > 0 ? h - q : 0); sp <= j && sp < nsp; ++sp)
        a += tot[sp][band_slot(j - sp, h - sp)];
    M[o] = a;
  }
}

// ---------------------------------------------------------------- pass 2
// one span's run [r0, r1) of the bucketed chunk into this thread's four replicates of the
// span's Q + 1 basis slots. The words are stored inverted (as csrc/gate.hip): a set bit is
// the multiplier -1. xi is assembled from its bits (1.0 with the bit as the sign): a convert
// of the sign-extended bit field "| 1" is compiled to an unsigned convert here, -1 -> 2^32 - 1.
template <int Q>
__device__ __forceinline__ void walk_run(const double* rec, const uint4* sw, int nsw, int s,
                                         int bit, int r0, int r1, double (*a)[4]) {
#pragma unroll 2
  for (int r = r0; r < r1; ++r) {
    const uint4 w = sw[r * nsw + s];
    const uint32_t wk[4] = {w.x, w.y, w.z, w.w};
    double xi[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      xi[k] = __hiloint2double((int)(0x3FF00000u | (((wk[k] >> bit) & 1u) << 31)), 0);
#pragma unroll
    for (int c = 0; c <= Q; ++c) {
      const double eb = rec[r * REC + c];
#pragma unroll
      for (int k = 0; k < 4; ++k) a[c][k] = fma(eb, xi[k], a[c][k]);   // exact product: +/-eb
    }
  }
}

// partial slabs: PT [(by * nbx + bx)][j < d][k < 4][CH], PB [bx][DMAX][NF] (stream block 0)
template <int Q, bool REG>
__global__ __launch_bounds__(CHMAX) void cate_boot_kernel(
    const double* __restrict__ psi, const double* __restrict__ x, const int64_t* __restrict__ rid,
    int64_t ld, const double* __restrict__ knots, const double* __restrict__ beta, int d, int nst,
    uint64_t seed, double* __restrict__ PT, double* __restrict__ PB) {
  __shared__ __attribute__((aligned(16))) uint4 sw[CHMAX * SPWMAX];   // bucketed Philox words
  __shared__ __attribute__((aligned(16))) double rec[CHMAX * REC];    // bucketed e b_c
  __shared__ double sk[DMAX + QMAX + 1];
  __shared__ double sb[DMAX];
  __shared__ int wcnt[CHMAX / 64][DMAX];
  __shared__ int start[DMAX + 1];
  const int CH = blockDim.x, nsw = CH >> 5, nsp = d - Q;
  const int t = threadIdx.x;
  const int s = t >> 5, bit = t & 31;
  const int stream0 = blockIdx.y * nsw;
  const bool active = stream0 + s < nst;
  const bool doband = blockIdx.y == 0;    // the first stream block also sums the meat
  ATE_DASSERT(d >= Q + 1 && d <= DMAX && (!REG || d <= DREG) && CH <= CHMAX && (CH & 63) == 0);
  if (t < d + Q + 1) sk[t] = knots[t];
  if (t < d) sb[t] = beta[t];
  int ia, ic;
  band_fn(t & 15, ia, ic);
  double acc[NPASS];
#pragma unroll
  for (int p = 0; p < NPASS; ++p) acc[p] = 0.0;
  const int64_t slab = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * d * 4 * CH;
  double c[REG ? DREG : Q + 1][4];
  if (REG) {
#pragma unroll
    for (int j = 0; j < (REG ? DREG : 1); ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) c[j][k] = 0.0;
  } else {
    for (int j = 0; j < d; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) PT[slab + ((int64_t)j * 4 + k) * CH + t] = 0.0;
  }
  __syncthreads();
  const int64_t nchunk = (ld + CH - 1) / CH;
  for (int64_t ck = blockIdx.x; ck < nchunk; ck += gridDim.x) {
    const int64_t i = ck * CH + t;
    const int64_t id = i < ld ? rid[i] : -1;
    const bool valid = id >= 0;
    const double p = valid ? psi[i] : 0.0;
    double N[QMAX + 1];
    const int g = basis_eval<Q>(sk, d, valid ? x[i] : sk[0], N);
    double e = p;
#pragma unroll
    for (int cc = 0; cc <= Q; ++cc) e -= N[cc] * sb[g + cc];
    const int pos = bucket_rows<DMAX>(valid, g, wcnt, start);
    if (valid) {
#pragma unroll
      for (int cc = 0; cc <= QMAX; ++cc) rec[pos * REC + cc] = e * N[cc];
      rec[pos * REC + 4] = 0.0;
      rec[pos * REC + 5] = 1.0;
      store_words(sw, pos, nsw, stream0, nst, seed, id);
    }
    __syncthreads();
    if (doband) band_accumulate(rec, start, nsp, ia, ic, acc);
    if (active) {
      if (REG) {
#pragma unroll
        for (int sp = 0; sp < (REG ? DREG - Q : 1); ++sp)
          if (sp < nsp) walk_run<Q>(rec, sw, nsw, s, bit, start[sp], start[sp + 1], &c[REG ? sp : 0]);
      } else {
        for (int sp = 0; sp < nsp; ++sp) {
          const int r0 = start[sp], r1 = start[sp + 1];
          if (r0 == r1) continue;
          const int64_t o = slab + (int64_t)sp * 4 * CH + t;
          ATE_DASSERT(sp + Q < d);
#pragma unroll
          for (int cc = 0; cc <= Q; ++cc)
#pragma unroll
            for (int k = 0; k < 4; ++k) c[cc][k] = PT[o + ((int64_t)cc * 4 + k) * CH];
          walk_run<Q>(rec, sw, nsw, s, bit, r0, r1, &c[0]);
#pragma unroll
          for (int cc = 0; cc <= Q; ++cc)
#pragma unroll
            for (int k = 0; k < 4; ++k) PT[o + ((int64_t)cc * 4 + k) * CH] = c[cc][k];
        }
      }
    }
  }
  if (REG) {
#pragma unroll
    for (int j = 0; j < (REG ? DREG : 1); ++j)
      if (j < d)
#pragma unroll
        for (int k = 0; k < 4; ++k) PT[slab + ((int64_t)j * 4 + k) * CH + t] = c[j][k];
  }
  if (doband) band_store(PB, nsp, acc);
}

// T [B][d] from the slabs, by the fixed-order slab_sum.
__global__ __launch_bounds__(256) void cate_t_sum_kernel(const double* __restrict__ PT, int d,
                                                         int B, int CH, int nbx, int nby,
                                                         double* __restrict__ T) {
  double a;
  long long z;
  int b, f;
  if (slab_sum<false>(PT, nullptr, d, B, CH, nbx, nby, a, z, b, f)) T[(int64_t)b * d + f] = a;
}

inline int64_t pb_elems(int nbx) { return (int64_t)nbx * DMAX * NF; }
constexpr int64_t TOT_ELEMS = DMAX * NF + 2;
inline bool bad_basis(int d, int q) { return q < 0 || q > QMAX || d < q + 1 || d > DMAX; }

template <int Q>
int launch_boot(const Geo& g, int nbx, hipStream_t s, const double* psi, const double* x,
                const int64_t* rid, int64_t ld, const double* knots, const double* beta, int d,
                uint64_t seed, double* PT, double* PB) {
  const auto reg = cate_boot_kernel<Q, true>, slab = cate_boot_kernel<Q, false>;
  if (d <= DREG)
    ATE_LAUNCH(reg, dim3(nbx, g.nby), dim3(g.CH), 0, s, psi, x, rid, ld,
               knots, beta, d, g.nst, seed, PT, PB);
  else
    ATE_LAUNCH(slab, dim3(nbx, g.nby), dim3(g.CH), 0, s, psi, x, rid, ld,
               knots, beta, d, g.nst, seed, PT, PB);
  ATE_CHECK_LAUNCH();
  return 0;
}

}  // namespace

ATE_KERNEL_SHAPE("cate_moments_kernel", CHMAX, 0, cate_moments_kernel)
ATE_KERNEL_SHAPE("cate_boot_kernel<0, reg>", CHMAX, 0, cate_boot_kernel<0, true>)
ATE_KERNEL_SHAPE("cate_boot_kernel<1, reg>", CHMAX, 0, cate_boot_kernel<1, true>)
ATE_KERNEL_SHAPE("cate_boot_kernel<2, reg>", CHMAX, 0, cate_boot_kernel<2, true>)
ATE_KERNEL_SHAPE("cate_boot_kernel<3, reg>", CHMAX, 0, cate_boot_kernel<3, true>)
ATE_KERNEL_SHAPE("cate_boot_kernel<0, slab>", CHMAX, 0, cate_boot_kernel<0, false>)
ATE_KERNEL_SHAPE("cate_boot_kernel<1, slab>", CHMAX, 0, cate_boot_kernel<1, false>)
ATE_KERNEL_SHAPE("cate_boot_kernel<2, slab>", CHMAX, 0, cate_boot_kernel<2, false>)
ATE_KERNEL_SHAPE("cate_boot_kernel<3, slab>", CHMAX, 0, cate_boot_kernel<3, false>)

// bytes of the partial workspace of ate_cate_moments(d, q, nbx); -1: bad arguments
ATE_API int64_t ate_cate_moments_scratch(int d, int q, int nbx) {
  if (bad_basis(d, q) || bad_boot(1, nbx)) return -1;       // pass 1 has no replicates
  return (pb_elems(nbx) + (int64_t)nbx * 2 + TOT_ELEMS) * 8;
}

// psi, x [ld] fp64, rid [ld] int64 global row ids (negative: skip the row; psi and x are then
// not read). knots [d + q + 1] fp64 (device). out [3 + (d - q) + d + d*d] fp64:
// n | S psi | S psi^2 | rows per span | v | M. scratch: ate_cate_moments_scratch bytes.
// nbx: workgroups along the rows.
ATE_API int ate_cate_moments(const void* psi, const void* x, const void* rid, int64_t ld,
                             const void* knots, int d, int q, int nbx, void* scratch, void* out,
                             void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (bad_basis(d, q) || bad_boot(1, nbx, ld)) return -1;
  double* PB = (double*)scratch;
  double* PS = PB + pb_elems(nbx);
  ATE_LAUNCH(cate_moments_kernel, dim3(nbx), dim3(CHMAX), 0, s, (const double*)psi,
             (const double*)x, (const int64_t*)rid, ld, (const double*)knots, d, q, PB, PS);
  ATE_CHECK_LAUNCH();
  double* TOT = PS + (int64_t)nbx * 2;
  ATE_LAUNCH(cate_band_reduce_kernel, dim3(d - q + 1), dim3(256), 0, s, (const double*)PB,
             (const double*)PS, nbx, d - q, TOT);
  ATE_CHECK_LAUNCH();
  ATE_LAUNCH(cate_band_out_kernel, dim3(1), dim3(256), 0, s, (const double*)TOT, true, d, q,
             (double*)out);
  ATE_CHECK_LAUNCH();
  return 0;
}

// bytes of the partial workspace of ate_cate_boot(d, q, B, nbx); -1: bad arguments
ATE_API int64_t ate_cate_boot_scratch(int d, int q, int B, int nbx) {
  if (bad_basis(d, q) || bad_boot(B, nbx)) return -1;
  return (slab_elems(geometry(B), d, nbx) + pb_elems(nbx) + TOT_ELEMS) * 8;
}

// The rows of ate_cate_moments and beta [d] fp64 (device). out [d*d + B*d] fp64: Meat | T.
// scratch: ate_cate_boot_scratch bytes, 16-byte aligned. nbx: workgroups along the rows.
ATE_API int ate_cate_boot(const void* psi, const void* x, const void* rid, int64_t ld,
                          const void* knots, const void* beta, int d, int q, int B, uint64_t seed,
                          int nbx, void* scratch, void* out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (bad_basis(d, q) || bad_boot(B, nbx, ld)) return -1;
  const Geo g = geometry(B);
  double* PT = (double*)scratch;
  double* PB = PT + slab_elems(g, d, nbx);
  const double *p = (const double*)psi, *xx = (const double*)x, *kn = (const double*)knots,
               *be = (const double*)beta;
  const int64_t* r = (const int64_t*)rid;
  int rc;
  switch (q) {
    case 0: rc = launch_boot<0>(g, nbx, s, p, xx, r, ld, kn, be, d, seed, PT, PB); break;
    case 1: rc = launch_boot<1>(g, nbx, s, p, xx, r, ld, kn, be, d, seed, PT, PB); break;
    case 2: rc = launch_boot<2>(g, nbx, s, p, xx, r, ld, kn, be, d, seed, PT, PB); break;
    default: rc = launch_boot<3>(g, nbx, s, p, xx, r, ld, kn, be, d, seed, PT, PB); break;
  }
  if (rc != 0) return rc;
  double* TOT = PB + pb_elems(nbx);
  ATE_LAUNCH(cate_band_reduce_kernel, dim3(d - q), dim3(256), 0, s, (const double*)PB,
             (const double*)nullptr, nbx, d - q, TOT);
  ATE_CHECK_LAUNCH();
  ATE_LAUNCH(cate_band_out_kernel, dim3(1), dim3(256), 0, s, (const double*)TOT, false, d, q,
             (double*)out);
  ATE_CHECK_LAUNCH();
  const int64_t items = (int64_t)g.nby * d * 4 * g.CH;
  ATE_LAUNCH(cate_t_sum_kernel, dim3((unsigned)((items + 15) / 16)), dim3(256), 0, s,
             (const double*)PT, d, B, g.CH, nbx, g.nby, (double*)out + (int64_t)d * d);
  ATE_CHECK_LAUNCH();
  return 0;
}
