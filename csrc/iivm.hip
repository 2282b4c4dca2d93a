// Fused held-out score pass of the cross-fitted interactive IV model (DML-IIVM, Chernozhukov
// et al. 2018 §5.2; DoubleML DoubleMLIIVM): the local average treatment effect (LATE) with a
// binary instrument Z, a binary treatment taken D and linear nuisances.
//
// The panel is the arm-split fold panel of csrc/irm.hip with the INSTRUMENT in its W column
// (segment 2k + z = rows of fold k with Z = z at segs_per_fold = 2; 1: a plain K-fold panel)
// and D in a further target column. For every row i of segment s, with the five coefficient
// vectors (g0, g1, r0, r1, m) of block k = s / segs_per_fold:
//   g0 = E[Y|Z=0,X]  g1 = E[Y|Z=1,X]  r0 = E[D|Z=0,X]  r1 = E[D|Z=1,X]  m = E[Z|X]
//   e = min(max(m, clip), 1 - clip)
//   b = g1 - g0 + z (y - g1) / e - (1 - z)(y - g0) / (1 - e)     (the ITT score: irm_psi on y)
//   a = r1 - r0 + z (d - r1) / e - (1 - z)(d - r0) / (1 - e)     (the first stage: irm_psi on d)
// and the 15 moments (result.LATE_MOMENTS)
//   0 S b   1 S b^2   2 n   3 n_clipped   4 S a   5 S a^2   6 S a b   7 S z
//   8 S z d   9 S (1-z) d   10 S z (y-g1)^2   11 S (1-z)(y-g0)^2
//   12 S z (d-r1)^2   13 S (1-z)(d-r0)^2   14 S (z-m)^2
// are accumulated in fp64: theta = S b / S a, and no per-row value is written to HBM. Four
// fp64 divisions per row (two per score), the count of the sensitivity pass of csrc/irm.hip.
// The five vectors are staged in LDS interleaved per column (cv[j * 5 + r]: one column's five
// coefficients are one contiguous LDS read), the ordered union of their supports is
// compacted, every column of that union is read ONCE, and `one`, Y, D and Z once per row; z
// is read from the panel on every row, never inferred from the segment.
//
// Shared bits, at the same nbx: a thread owns the same rows as in irm_score_kernel, visits
// the columns in the same ascending-j order, and a column outside one vector's own support
// has the coefficient 0 there: fma(0, x, acc) = acc for every finite x, so the wider union
// leaves each dot product as it was (but for an accumulator that is exactly -0.0, which
// becomes +0.0: the score adds, subtracts and compares it, so no moment changes). The row
// then goes through the same irm_psi and the same expressions as irm_accumulate, the block
// through block_sum and the partials through the same fixed-order sum, moment by moment. So
//   moments [0,1,2,3,7,10,11,14] carry the bits of ate_irm_score_moments [0,1,2,3,7,4,5,6]
//     called with the rows (g0, g1, m), and
//   moments [4,5,12,13] those of ate_irm_score_moments [0,1,4,5] on a panel whose Y column
//     holds D, called with the rows (r0, r1, m).
#include "irm_common.hpp"

using namespace ate;

namespace {

constexpr int NL = 15;   // moments; not 16: the static red[16 NL] + 64 bytes stay within 2048
constexpr int NV = 5;    // coefficient vectors of a block: g0, g1, r0, r1, m

// one valid row's contribution to the 15 moments. The terms shared with irm_accumulate
// (csrc/irm.hip) are the same expressions on the same operands.
__device__ __forceinline__ void iivm_accumulate(double (&v)[NL], double y, double d, double z,
                                                double g0, double g1, double q0, double q1,
                                                double m, double clip) {
  const double lo = clip, hi = 1.0 - clip;
  const double r1 = y - g1, r0 = y - g0, rm = z - m;
  const double u1 = d - q1, u0 = d - q0;
  ATE_DASSERT(z == 0.0 || z == 1.0);
  const double b = irm_psi(y, z, g0, g1, m, clip);
  const double a = irm_psi(d, z, q0, q1, m, clip);
  v[0] += b;
  v[1] += b * b;
  v[2] += 1.0;
  v[3] += (m < lo || m > hi) ? 1.0 : 0.0;
  v[4] += a;
  v[5] += a * a;
  v[6] += a * b;
  v[7] += z;
  v[8] += z * d;
  v[9] += (1.0 - z) * d;
  v[10] += z * (r1 * r1);
  v[11] += (1.0 - z) * (r0 * r0);
  v[12] += z * (u1 * u1);
  v[13] += (1.0 - z) * (u0 * u0);
  v[14] += rm * rm;
}

// stage the five coefficient vectors of block k, interleaved per column, and the column
// list; returns the size of the compacted union
template <typename C>
__device__ __forceinline__ int stage_five(C* cv, int* xc, const int* __restrict__ xcols, int p,
                                          int P, const double* __restrict__ coef, int k,
                                          int* wcnt) {
  for (int j = threadIdx.x; j < p; j += blockDim.x) {
    xc[j] = xcols[j];
    ATE_DASSERT(xc[j] >= 0 && (P == 0 || xc[j] < P));
  }
  for (int j = threadIdx.x; j <= p; j += blockDim.x)
#pragma unroll
    for (int r = 0; r < NV; ++r)
      cv[(int64_t)j * NV + r] = (C)coef[((int64_t)k * NV + r) * (p + 1) + j];
  __syncthreads();
  return compact_support_n<NV>(cv, xc, p, wcnt);
}

// fp32 / fp64 column-major panels: fp64 dot products, RPT rows per thread 256 apart (the
// row ownership of irm_score_kernel). partial: [nseg * nbx][15].
template <typename T, int RPT>
__global__ __launch_bounds__(256) void iivm_score_kernel(
    const T* __restrict__ X, int64_t ld, const int* __restrict__ xcols, int p, int P,
    const Seg* __restrict__ segs, int nseg, int spf,
    const double* __restrict__ coef /*[nfold][5][p+1]*/, int y0, int y1, int d0, int d1, int w0,
    int w1, int vcol, double clip, double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double sh[];
  double* cv = sh;                                // [p+1][5]
  int* xc = (int*)(sh + (int64_t)NV * (p + 1));   // [p]
  __shared__ double red[16 * NL];                 // static LDS: 1920 + 64 bytes, inside the
  __shared__ int wcnt[16];                        // 2048 iivm_pass leaves free
  const int s = blockIdx.y, k = s / spf;
  ATE_DASSERT(s < nseg && spf >= 1 && y0 >= 0 && d0 >= 0 && w0 >= 0 && vcol >= 0);
  ATE_DASSERT(P == 0 || (y0 < P && d0 < P && w0 < P && vcol < P && y1 < P && d1 < P && w1 < P));
  p = stage_five(cv, xc, xcols, p, P, coef, k, wcnt);
  const Seg sg = segs[s];
  ATE_DASSERT(sg.r0 >= 0 && sg.r0 <= sg.r1 && sg.r1 <= ld);
  double v[NL] = {};
  for (int64_t base = sg.r0 + (int64_t)blockIdx.x * 256 * RPT; base < sg.r1;
       base += (int64_t)gridDim.x * 256 * RPT) {
    double a[NV][RPT];
    int64_t ii[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      ii[r] = base + r * 256 + threadIdx.x;
#pragma unroll
      for (int q = 0; q < NV; ++q) a[q][r] = cv[q];
    }
    for (int j = 0; j < p; ++j) {
      const double* cj = cv + (int64_t)(1 + j) * NV;
      const int c = xc[j];
      double x[RPT];
#pragma unroll
      for (int r = 0; r < RPT; ++r) x[r] = ii[r] < sg.r1 ? ld_col(X, ld, c, ii[r]) : 0.0;
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        const double bq = cj[q];
#pragma unroll
        for (int r = 0; r < RPT; ++r) a[q][r] += bq * x[r];
      }
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      if (ii[r] >= sg.r1) continue;
      if (ld_col(X, ld, vcol, ii[r]) == 0.0) continue;          // padding row
      const double y = ld_col(X, ld, y0, ii[r]) + (y1 >= 0 ? ld_col(X, ld, y1, ii[r]) : 0.0);
      const double d = ld_col(X, ld, d0, ii[r]) + (d1 >= 0 ? ld_col(X, ld, d1, ii[r]) : 0.0);
      const double z = ld_col(X, ld, w0, ii[r]) + (w1 >= 0 ? ld_col(X, ld, w1, ii[r]) : 0.0);
      ATE_DASSERT(spf != 2 || z == (double)(s & 1));
      iivm_accumulate(v, y, d, z, a[0][r], a[1][r], a[2][r], a[3][r], a[4][r], clip);
    }
  }
  write_partial<NL>(v, red, partial);
}

// bf16 panels (column-major and 64-row blocked): each thread owns 8 CONSECUTIVE rows, so
// every column read is one 16-byte load through (cs, bs); dot products in fp32 (bf16 values
// are exact in fp32; coefficients rounded to fp32), the scores in fp64 (the row ownership
// and arithmetic of irm_score_bf16_kernel).
__global__ __launch_bounds__(256) void iivm_score_bf16_kernel(
    const bf16_t* __restrict__ X, int64_t cs, int64_t bs, const int* __restrict__ xcols, int p,
    int P, int64_t ld, const Seg* __restrict__ segs, int nseg, int spf,
    const double* __restrict__ coef, int y0, int y1, int d0, int d1, int w0, int w1, int vcol,
    double clip, double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) float shf[];
  float* cv = shf;                                 // [p+1][5]
  int* xc = (int*)(shf + (int64_t)NV * (p + 1));   // [p]
  __shared__ double red[16 * NL];
  __shared__ int wcnt[16];
  const int s = blockIdx.y, k = s / spf;
  ATE_DASSERT(s < nseg && spf >= 1 && y0 >= 0 && d0 >= 0 && w0 >= 0 && vcol >= 0);
  ATE_DASSERT(P == 0 || (y0 < P && d0 < P && w0 < P && vcol < P && y1 < P && d1 < P && w1 < P));
  p = stage_five(cv, xc, xcols, p, P, coef, k, wcnt);
  const Seg sg = segs[s];
  ATE_DASSERT(sg.r0 >= 0 && sg.r0 <= sg.r1 && (ld == 0 || sg.r1 <= ld) && (sg.r0 & 7) == 0 &&
              (sg.r1 & 7) == 0);
  auto ld8 = [&](int c, int64_t i, float (&o)[8]) {
    ATE_DASSERT((i & 7) == 0 && c >= 0 && (P == 0 || c < P) && (ld == 0 || i + 8 <= ld));
    // (c, i) at c*cs + (i/64)*bs + i%64; the 8 rows never straddle a block (i % 8 == 0)
    const uint4 u = *reinterpret_cast<const uint4*>(X + (int64_t)c * cs + (i >> 6) * bs + (i & 63));
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      o[2 * q] = __uint_as_float(w[q] << 16);
      o[2 * q + 1] = __uint_as_float(w[q] & 0xFFFF0000u);
    }
  };
  auto ld8_pair = [&](int c0, int c1, int64_t i, float (&hi)[8], float (&lo)[8]) {
    ld8(c0, i, hi);
    if (c1 >= 0) ld8(c1, i, lo); else { for (int r = 0; r < 8; ++r) lo[r] = 0.f; }
  };
  double v[NL] = {};
  for (int64_t i = sg.r0 + ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8; i < sg.r1;
       i += (int64_t)gridDim.x * 256 * 8) {
    float a[NV][8];
#pragma unroll
    for (int q = 0; q < NV; ++q)
#pragma unroll
      for (int r = 0; r < 8; ++r) a[q][r] = cv[q];
#pragma unroll 2
    for (int j = 0; j < p; ++j) {
      float x[8];
      ld8(xc[j], i, x);
      const float* cj = cv + (int64_t)(1 + j) * NV;
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        const float bq = cj[q];
#pragma unroll
        for (int r = 0; r < 8; ++r) a[q][r] += bq * x[r];
      }
    }
    float vv[8], ya[8], yb[8], da[8], db[8], wa[8], wb[8];
    ld8(vcol, i, vv);
    ld8_pair(y0, y1, i, ya, yb);
    ld8_pair(d0, d1, i, da, db);
    ld8_pair(w0, w1, i, wa, wb);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      if (vv[r] == 0.f) continue;                                 // padding row
      const double y = (double)ya[r] + (double)yb[r];
      const double d = (double)da[r] + (double)db[r];
      const double z = (double)wa[r] + (double)wb[r];
      ATE_DASSERT(spf != 2 || z == (double)(s & 1));
      iivm_accumulate(v, y, d, z, (double)a[0][r], (double)a[1][r], (double)a[2][r],
                      (double)a[3][r], (double)a[4][r], clip);
    }
  }
  write_partial<NL>(v, red, partial);
}

constexpr int IIVM_LDS_MAX = 64 * 1024 - 2048;   // dynamic LDS: what the static part leaves

template <typename T>
int iivm_score_t(const void* X, int64_t ld, const void* xcols, int p, int P, const void* segs,
                 int nseg, int spf, const void* coef, int y0, int y1, int d0, int d1, int w0,
                 int w1, int vcol, double clip, int nbx, void* partial, size_t sh, hipStream_t s) {
  ATE_LAUNCH((iivm_score_kernel<T, 4>), dim3(nbx, nseg), dim3(256), sh, s, (const T*)X, ld,
             (const int*)xcols, p, P, (const Seg*)segs, nseg, spf, (const double*)coef, y0, y1,
             d0, d1, w0, w1, vcol, clip, (double*)partial);
  ATE_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// the largest launch of each instantiation, for the debug build's load-time resource check
ATE_KERNEL_SHAPE("iivm_score_kernel<float>", 256, IIVM_LDS_MAX, iivm_score_kernel<float, 4>)
ATE_KERNEL_SHAPE("iivm_score_kernel<double>", 256, IIVM_LDS_MAX, iivm_score_kernel<double, 4>)
ATE_KERNEL_SHAPE("iivm_score_bf16_kernel", 256, IIVM_LDS_MAX, iivm_score_bf16_kernel)
ATE_KERNEL_SHAPE("irm_sum_kernel<15>", 256, 0, irm_sum_kernel<NL>)

// The LATE pass. dtype 1 f32, 2 f64, 3 bf16. (cs, bs): element (c, i) at c*cs + (i/64)*bs +
// i%64 (fp32 / fp64 panels: column-major only, bs = 64). segs [nseg][2] int64 padded row
// ranges; coef [ceil(nseg / segs_per_fold)][5][p+1] fp64, rows (g0, g1, r0, r1, m), intercept
// first; (y0, y1), (d0, d1), (w0, w1): the columns of Y, D and the instrument Z (second = -1
// unless the target is stored as a hi + lo bf16 pair). The argument checks are those of the
// score pass of csrc/irm.hip (-1: rejected, nothing launched); the LDS bound is
// 5 (p+1) esz + 4 p <= 64 KB - 2048. partial: [nseg*nbx][15]; moments: [15].
ATE_API int ate_iivm_moments(int dtype, const void* X, int64_t cs, int64_t bs, const void* xcols,
                             int p, const void* segs, int nseg, int segs_per_fold,
                             const void* coef, int y0, int y1, int d0, int d1, int w0, int w1,
                             int vcol, double clip, int nbx, void* partial, void* moments,
                             void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (dtype < 1 || dtype > 3 || (dtype != 3 && bs != 64)) return -1;
  if (p < 0 || nseg < 1 || nseg > 65535 || segs_per_fold < 1 || nbx < 1 || cs < 64 || bs < 64)
    return -1;
  if (y0 < 0 || d0 < 0 || w0 < 0 || vcol < 0) return -1;
  // what the strides say about the panel's extent, for the debug build's bounds checks
  // (0 = unknown): column-major (bs = 64) has ld = cs rows; 64-row blocked has P = bs / 64
  const int64_t ld = bs == 64 ? cs : 0;
  const int P = bs == 64 ? 0 : (int)(bs / 64);
  if (!(clip >= 0.0 && clip < 0.5)) return -1;
  const size_t esz = dtype == 3 ? sizeof(float) : sizeof(double);
  const size_t sh = (size_t)NV * (p + 1) * esz + (size_t)p * sizeof(int);
  static_assert(16 * NL * sizeof(double) + 64 <= 2048, "static LDS of the pass");
  if (sh > (size_t)IIVM_LDS_MAX) return -1;
  int rc = 0;
  if (dtype == 1)
    rc = iivm_score_t<float>(X, cs, xcols, p, P, segs, nseg, segs_per_fold, coef, y0, y1, d0, d1,
                             w0, w1, vcol, clip, nbx, partial, sh, s);
  else if (dtype == 2)
    rc = iivm_score_t<double>(X, cs, xcols, p, P, segs, nseg, segs_per_fold, coef, y0, y1, d0, d1,
                              w0, w1, vcol, clip, nbx, partial, sh, s);
  else {
    ATE_LAUNCH(iivm_score_bf16_kernel, dim3(nbx, nseg), dim3(256), sh, s, (const bf16_t*)X, cs, bs,
               (const int*)xcols, p, P, ld, (const Seg*)segs, nseg, segs_per_fold,
               (const double*)coef, y0, y1, d0, d1, w0, w1, vcol, clip, (double*)partial);
    ATE_CHECK_LAUNCH();
  }
  if (rc != 0) return rc;
  ATE_LAUNCH(irm_sum_kernel<NL>, dim3(1), dim3(256), 0, s, (const double*)partial, nbx * nseg,
             (double*)moments);
  ATE_CHECK_LAUNCH();
  return 0;
}
