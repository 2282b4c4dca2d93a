// Fused held-out score pass of the cross-fitted interactive model (DML-IRM, AIPW score)
// with linear nuisances.
//
// For every row i of segment s, with the coefficient triple of block k = s / segs_per_fold
// (segs_per_fold = 2: the arm-split layout, segment 2k + a = rows of fold k with W = a;
// 1: a plain K-fold panel):
//   g0_i = c0[0] + x_i . c0[1:],  g1_i = c1[0] + x_i . c1[1:],  m_i = cm[0] + x_i . cm[1:]
//   e_i  = min(max(m_i, clip), 1 - clip)
//   psi_i = g1_i - g0_i + w_i (y_i - g1_i) / e_i - (1 - w_i) (y_i - g0_i) / (1 - e_i)
// and the 8 moments
//   {S psi, S psi^2, n, n_clipped, S w (y - g1)^2, S (1 - w)(y - g0)^2, S (w - m)^2, n_treated}
// are accumulated in fp64: no per-row value is written to HBM (ate_irm_score_moments), or,
// by the same kernels instantiated with ROWS, psi_i itself is written per row for the group
// bootstrap of csrc/gate.hip (ate_irm_scores), or, instantiated with SENS, the 14 moments of
// the sensitivity analysis are accumulated (ate_irm_sens_moments), or, instantiated with
// TARGETS, the 12 moments of the three target populations (ate_irm_target_moments): with
//   q1 = w (y - g1) / e,  q0 = (1 - w)(y - g0) / (1 - e)      (the two quotients of psi)
//   a  = w (y - g0) - e q0            the numerator of the effect on the treated (ATT)
//   c  = -(1 - w)(y - g1) + (1 - e) q1   the numerator of the effect on the controls (ATC)
// psi = a + c algebraically, theta_all = S psi / n, theta_treated = S a / n1, theta_control =
// S c / n0, and the joint 3x3 covariance follows from
//   {S psi, S psi^2, n, n_clipped, S a, S a^2, S a w, S c, S c^2, S c (1 - w), S a c, n_treated}
// (result.TARGET_MOMENTS; the score of DoubleML's IRM(score="ATTE")). w is read from the panel
// on every row, never inferred from the segment. Only the columns in the union of the three
// LASSO supports are read, once each; the coefficient triple is staged in LDS. y / w are
// rebuilt from their hi + lo bf16 columns on bf16 panels. Structure as csrc/dml.hip. What
// the LATE pass of csrc/iivm.hip shares (ld_col, Seg, compact_support_n, irm_psi,
// write_partial, irm_sum_kernel) lives in irm_common.hpp.
#include "irm_common.hpp"

using namespace ate;

namespace {

// What a score pass produces: the 8 moments above, psi per row, the 14 moments of the
// sensitivity analysis (ate_irm_sens_moments below) or the 12 moments of the target
// populations (ate_irm_target_moments below).
enum Mode { MOMENTS = 0, ROWS = 1, SENS = 2, TARGETS = 3 };

// What the third coefficient row predicts: the propensity itself (the linear-probability
// fit) or its logit (the binomial fit of csrc/lognet.hip): m = 1 / (1 + exp(-eta)) in fp64,
// before the score sees it, so n_clipped and S (w - m)^2 are about the probability.
enum Link { IDENTITY = 0, LOGISTIC = 1 };

constexpr int NM = 8;    // moments of MOMENTS
constexpr int NS = 14;   // moments of SENS
constexpr int NT = 12;   // moments of TARGETS
template <int MODE> constexpr int nmom() { return MODE == SENS ? NS : MODE == TARGETS ? NT : NM; }

// Ordered compaction (ascending j: the dot products keep the summation order of the dense
// loop, bit for bit) of the feature columns with a nonzero coefficient in any of the three
// nuisances. c0/c1/cm/xc: dense staged arrays, compacted in place (c*[1+q], xc[q] for
// q < return value). The whole block must call it.
template <typename C>
__device__ int compact_support3(C* c0, C* c1, C* cm, int* xc, int p, int* wcnt /* [>= 16] */) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int base = 0;
  for (int j0 = 0; j0 < p; j0 += blockDim.x) {
    const int j = j0 + threadIdx.x;
    const C v0 = j < p ? c0[1 + j] : C(0), v1 = j < p ? c1[1 + j] : C(0),
            vm = j < p ? cm[1 + j] : C(0);
    const bool keep = v0 != C(0) || v1 != C(0) || vm != C(0);
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
    if (keep) { c0[1 + pos] = v0; c1[1 + pos] = v1; cm[1 + pos] = vm; xc[pos] = c; }
    __syncthreads();
    base = tot;
  }
  return base;
}

// one valid row's contribution to the 8 moments
__device__ __forceinline__ void irm_accumulate(double (&v)[NM], double y, double w, double g0,
                                               double g1, double m, double clip) {
  const double lo = clip, hi = 1.0 - clip;
  const double r1 = y - g1, r0 = y - g0, rm = w - m;
  const double psi = irm_psi(y, w, g0, g1, m, clip);
  v[0] += psi;
  v[1] += psi * psi;
  v[2] += 1.0;
  v[3] += (m < lo || m > hi) ? 1.0 : 0.0;
  v[4] += w * (r1 * r1);
  v[5] += (1.0 - w) * (r0 * r0);
  v[6] += rm * rm;
  v[7] += w;
}

// one valid row's contribution to the 14 moments of the sensitivity analysis, with
//   b = (y - g_w)^2, rr = w / e - (1 - w) / (1 - e), c = 2 (1 / e + 1 / (1 - e)) - rr^2:
//   {S psi, S psi^2, n, n_clipped, S b, S b^2, S c, S c^2, S psi b, S psi c, S b c, S y,
//    S y^2, n_treated}
// psi, psi^2, n, n_clipped and n_treated as irm_accumulate, term for term.
__device__ __forceinline__ void irm_accumulate(double (&v)[NS], double y, double w, double g0,
                                               double g1, double m, double clip) {
  const double lo = clip, hi = 1.0 - clip;
  const double e = m < lo ? lo : (m > hi ? hi : m);
  const double r1 = y - g1, r0 = y - g0;
  const double psi = irm_psi(y, w, g0, g1, m, clip);
  const double b = w != 0.0 ? r1 * r1 : r0 * r0;
  // two fp64 divisions beside the two of psi (the pass is bound by them, not by HBM, once
  // there are six): for w in {0, 1}, w * (1 / e) is w / e to the bit
  const double ie = 1.0 / e, i1e = 1.0 / (1.0 - e);
  const double rr = w * ie - (1.0 - w) * i1e;
  const double c = 2.0 * (ie + i1e) - rr * rr;
  v[0] += psi;
  v[1] += psi * psi;
  v[2] += 1.0;
  v[3] += (m < lo || m > hi) ? 1.0 : 0.0;
  v[4] += b;
  v[5] += b * b;
  v[6] += c;
  v[7] += c * c;
  v[8] += psi * b;
  v[9] += psi * c;
  v[10] += b * c;
  v[11] += y;
  v[12] += y * y;
  v[13] += w;
}

// one valid row's contribution to the 12 moments of the target populations (all, treated,
// controls; the header comment):
//   {S psi, S psi^2, n, n_clipped, S a, S a^2, S a w, S c, S c^2, S c (1 - w), S a c, n_treated}
// psi, psi^2, n, n_clipped and n_treated as irm_accumulate(double (&)[NM], ...), term for
// term: psi goes through irm_psi. No division beside the two of psi: q1 and q0 are the
// quotients irm_psi forms (the same expressions on the same operands, one evaluation), and a
// and c are products and differences of them.
__device__ __forceinline__ void irm_accumulate(double (&v)[NT], double y, double w, double g0,
                                               double g1, double m, double clip) {
  const double lo = clip, hi = 1.0 - clip;
  const double e = m < lo ? lo : (m > hi ? hi : m);
  const double r1 = y - g1, r0 = y - g0;
  const double psi = irm_psi(y, w, g0, g1, m, clip);
  ATE_DASSERT(w == 0.0 || w == 1.0);                    // a and c: a binary treatment only
  const double q1 = w * r1 / e, q0 = (1.0 - w) * r0 / (1.0 - e);
  const double a = w * r0 - e * q0;
  const double c = -(1.0 - w) * r1 + (1.0 - e) * q1;
  v[0] += psi;
  v[1] += psi * psi;
  v[2] += 1.0;
  v[3] += (m < lo || m > hi) ? 1.0 : 0.0;
  v[4] += a;
  v[5] += a * a;
  v[6] += a * w;
  v[7] += c;
  v[8] += c * c;
  v[9] += c * (1.0 - w);
  v[10] += a * c;
  v[11] += w;
}

// fp32 / fp64 column-major panels: fp64 dot products, RPT rows per thread 256 apart.
// MODE ROWS: `partial` is psi[ld] instead -- every row of the segment gets its score (0 on a
// padding row) and no moment is accumulated (ate_irm_scores). SENS: the 14 moments; TARGETS:
// the 12 moments. LINK: the link of the propensity row (fp32 / fp64 panels only).
template <typename T, int RPT, int MODE, int LINK>
__global__ __launch_bounds__(256) void irm_score_kernel(
    const T* __restrict__ X, int64_t ld, const int* __restrict__ xcols, int p, int P,
    const Seg* __restrict__ segs, int nseg, int spf,
    const double* __restrict__ coef /*[nfold][3][p+1]*/, int y0, int y1, int w0, int w1,
    int vcol, double clip, double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double sh[];
  double* c0 = sh;                      // [p+1]
  double* c1 = sh + (p + 1);            // [p+1]
  double* cm = sh + 2 * (p + 1);        // [p+1]
  int* xc = (int*)(sh + 3 * (p + 1));   // [p]
  constexpr int N = nmom<MODE>();
  __shared__ double red[16 * N];        // static LDS: 1024 (SENS: 1792, TARGETS: 1536) + 64
                                        // bytes, inside the 2048 irm_pass leaves free
  __shared__ int wcnt[16];
  const int s = blockIdx.y, k = s / spf;
  ATE_DASSERT(s < nseg && spf >= 1 && y0 >= 0 && w0 >= 0 && vcol >= 0);
  ATE_DASSERT(P == 0 || (y0 < P && w0 < P && vcol < P && y1 < P && w1 < P));
  for (int j = threadIdx.x; j < p; j += blockDim.x) {
    xc[j] = xcols[j];
    ATE_DASSERT(xc[j] >= 0 && (P == 0 || xc[j] < P));
  }
  for (int j = threadIdx.x; j <= p; j += blockDim.x) {
    c0[j] = coef[((int64_t)k * 3 + 0) * (p + 1) + j];
    c1[j] = coef[((int64_t)k * 3 + 1) * (p + 1) + j];
    cm[j] = coef[((int64_t)k * 3 + 2) * (p + 1) + j];
  }
  __syncthreads();
  p = compact_support3(c0, c1, cm, xc, p, wcnt);
  const Seg sg = segs[s];
  ATE_DASSERT(sg.r0 >= 0 && sg.r0 <= sg.r1 && sg.r1 <= ld);
  double v[N] = {};
  for (int64_t base = sg.r0 + (int64_t)blockIdx.x * 256 * RPT; base < sg.r1;
       base += (int64_t)gridDim.x * 256 * RPT) {
    double a0[RPT], a1[RPT], am[RPT];
    int64_t ii[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      ii[r] = base + r * 256 + threadIdx.x;
      a0[r] = c0[0];
      a1[r] = c1[0];
      am[r] = cm[0];
    }
    for (int j = 0; j < p; ++j) {
      const double b0 = c0[1 + j], b1 = c1[1 + j], bm = cm[1 + j];
      const int c = xc[j];
#pragma unroll
      for (int r = 0; r < RPT; ++r) {
        const double x = ii[r] < sg.r1 ? ld_col(X, ld, c, ii[r]) : 0.0;
        a0[r] += b0 * x;
        a1[r] += b1 * x;
        am[r] += bm * x;
      }
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      if (ii[r] >= sg.r1) continue;
      if (ld_col(X, ld, vcol, ii[r]) == 0.0) {                  // padding row
        if (MODE == ROWS) partial[ii[r]] = 0.0;
        continue;
      }
      const double y = ld_col(X, ld, y0, ii[r]) + (y1 >= 0 ? ld_col(X, ld, y1, ii[r]) : 0.0);
      const double w = ld_col(X, ld, w0, ii[r]) + (w1 >= 0 ? ld_col(X, ld, w1, ii[r]) : 0.0);
      ATE_DASSERT(spf != 2 || w == (double)(s & 1));
      const double m = LINK == LOGISTIC ? 1.0 / (1.0 + exp(-am[r])) : am[r];
      if (MODE == ROWS) partial[ii[r]] = irm_psi(y, w, a0[r], a1[r], m, clip);
      else irm_accumulate(v, y, w, a0[r], a1[r], m, clip);
    }
  }
  if (MODE != ROWS) write_partial<N>(v, red, partial);
}

// bf16 panels: each thread owns 8 CONSECUTIVE rows, so every column read is one 16-byte
// load through (cs, bs) (column-major and 64-row blocked panels); dot products in fp32
// (bf16 values are exact in fp32; coefficients rounded to fp32), the score in fp64.
// MODE: as irm_score_kernel.
template <int MODE>
__global__ __launch_bounds__(256) void irm_score_bf16_kernel(
    const bf16_t* __restrict__ X, int64_t cs, int64_t bs, const int* __restrict__ xcols, int p,
    int P, int64_t ld, const Seg* __restrict__ segs, int nseg, int spf,
    const double* __restrict__ coef, int y0, int y1, int w0, int w1, int vcol, double clip,
    double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) float shf[];
  float* c0 = shf;                       // [p+1]
  float* c1 = shf + (p + 1);             // [p+1]
  float* cm = shf + 2 * (p + 1);         // [p+1]
  int* xc = (int*)(shf + 3 * (p + 1));   // [p]
  constexpr int N = nmom<MODE>();
  __shared__ double red[16 * N];
  __shared__ int wcnt[16];
  const int s = blockIdx.y, k = s / spf;
  ATE_DASSERT(s < nseg && spf >= 1 && y0 >= 0 && w0 >= 0 && vcol >= 0);
  ATE_DASSERT(P == 0 || (y0 < P && w0 < P && vcol < P && y1 < P && w1 < P));
  for (int j = threadIdx.x; j < p; j += blockDim.x) {
    xc[j] = xcols[j];
    ATE_DASSERT(xc[j] >= 0 && (P == 0 || xc[j] < P));
  }
  for (int j = threadIdx.x; j <= p; j += blockDim.x) {
    c0[j] = (float)coef[((int64_t)k * 3 + 0) * (p + 1) + j];
    c1[j] = (float)coef[((int64_t)k * 3 + 1) * (p + 1) + j];
    cm[j] = (float)coef[((int64_t)k * 3 + 2) * (p + 1) + j];
  }
  __syncthreads();
  p = compact_support3(c0, c1, cm, xc, p, wcnt);
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
  double v[N] = {};
  for (int64_t i = sg.r0 + ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8; i < sg.r1;
       i += (int64_t)gridDim.x * 256 * 8) {
    float a0[8], a1[8], am[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) { a0[r] = c0[0]; a1[r] = c1[0]; am[r] = cm[0]; }
#pragma unroll 4
    for (int j = 0; j < p; ++j) {
      float x[8];
      ld8(xc[j], i, x);
      const float b0 = c0[1 + j], b1 = c1[1 + j], bm = cm[1 + j];
#pragma unroll
      for (int r = 0; r < 8; ++r) { a0[r] += b0 * x[r]; a1[r] += b1 * x[r]; am[r] += bm * x[r]; }
    }
    float vv[8], ya[8], yb[8], wa[8], wb[8];
    ld8(vcol, i, vv);
    ld8(y0, i, ya);
    ld8(w0, i, wa);
    if (y1 >= 0) ld8(y1, i, yb); else { for (int r = 0; r < 8; ++r) yb[r] = 0.f; }
    if (w1 >= 0) ld8(w1, i, wb); else { for (int r = 0; r < 8; ++r) wb[r] = 0.f; }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      if (vv[r] == 0.f) {                                         // padding row
        if (MODE == ROWS) partial[i + r] = 0.0;
        continue;
      }
      const double y = (double)ya[r] + (double)yb[r];
      const double w = (double)wa[r] + (double)wb[r];
      ATE_DASSERT(spf != 2 || w == (double)(s & 1));
      if (MODE == ROWS) partial[i + r] = irm_psi(y, w, (double)a0[r], (double)a1[r], (double)am[r], clip);
      else irm_accumulate(v, y, w, (double)a0[r], (double)a1[r], (double)am[r], clip);
    }
  }
  if (MODE != ROWS) write_partial<N>(v, red, partial);
}

template <typename T, int MODE, int LINK>
int irm_score_t(const void* X, int64_t ld, const void* xcols, int p, int P, const void* segs,
                int nseg, int spf, const void* coef, int y0, int y1, int w0, int w1, int vcol,
                double clip, int nbx, void* partial, size_t sh, hipStream_t s) {
  ATE_LAUNCH((irm_score_kernel<T, 4, MODE, LINK>), dim3(nbx, nseg), dim3(256), sh, s, (const T*)X, ld,
             (const int*)xcols, p, P, (const Seg*)segs, nseg, spf, (const double*)coef, y0, y1,
             w0, w1, vcol, clip, (double*)partial);
  ATE_CHECK_LAUNCH();
  return 0;
}

// The score pass of every entry point (argument checks and the launch): ROWS writes psi[ld]
// through `out`, otherwise `out` is the partial buffer [nseg*nbx][8] (SENS: [14], TARGETS:
// [12]) of the moment pass. link: IDENTITY or LOGISTIC (fp32 / fp64 panels only).
template <int MODE>
int irm_pass(int link, int dtype, const void* X, int64_t cs, int64_t bs, const void* xcols, int p,
             const void* segs, int nseg, int segs_per_fold, const void* coef, int y0, int y1,
             int w0, int w1, int vcol, double clip, int nbx, void* out, hipStream_t s) {
  if (dtype < 1 || dtype > 3 || (dtype != 3 && bs != 64)) return -1;
  if ((link != IDENTITY && link != LOGISTIC) || (link == LOGISTIC && dtype == 3)) return -1;
  if (p < 0 || nseg < 1 || nseg > 65535 || segs_per_fold < 1 || nbx < 1 || cs < 64 || bs < 64)
    return -1;
  if (y0 < 0 || w0 < 0 || vcol < 0) return -1;
  // what the strides say about the panel's extent, for the debug build's bounds checks
  // (0 = unknown): column-major (bs = 64) has ld = cs rows; 64-row blocked has P = bs / 64
  const int64_t ld = bs == 64 ? cs : 0;
  const int P = bs == 64 ? 0 : (int)(bs / 64);
  if (!(clip >= 0.0 && clip < 0.5)) return -1;
  const size_t esz = dtype == 3 ? sizeof(float) : sizeof(double);
  const size_t sh = (size_t)3 * (p + 1) * esz + (size_t)p * sizeof(int);
  // dynamic + static LDS within the 64 KB default: the static part is 16 N 8 + 64 bytes, at
  // most 1856 (SENS, N = 14; TARGETS, N = 12: 1600)
  static_assert(16 * nmom<MODE>() * sizeof(double) + 64 <= 2048, "static LDS of the pass");
  if (sh > 64 * 1024 - 2048) return -1;
  if (dtype != 3) {
    auto f = dtype == 1 ? (link == LOGISTIC ? irm_score_t<float, MODE, LOGISTIC>
                                            : irm_score_t<float, MODE, IDENTITY>)
                        : (link == LOGISTIC ? irm_score_t<double, MODE, LOGISTIC>
                                            : irm_score_t<double, MODE, IDENTITY>);
    return f(X, cs, xcols, p, P, segs, nseg, segs_per_fold, coef, y0, y1, w0, w1, vcol, clip, nbx,
             out, sh, s);
  }
  ATE_LAUNCH(irm_score_bf16_kernel<MODE>, dim3(nbx, nseg), dim3(256), sh, s, (const bf16_t*)X, cs,
             bs, (const int*)xcols, p, P, ld, (const Seg*)segs, nseg, segs_per_fold,
             (const double*)coef, y0, y1, w0, w1, vcol, clip, (double*)out);
  ATE_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------- S partitions, one pass
// Repeated cross-fitting scores every row under S partitions of the same segments: split t
// gives segment group g = s / segs_per_fold the coefficient block blk[t][g]. The kernels
// below run NSP splits in one pass over the panel: the 3 NSP coefficient vectors of the
// segment are staged in LDS, interleaved per column (cv[j * 3 NSP + 3 t + r]: one column's
// coefficients are one contiguous LDS read), the ordered union of their supports is
// compacted, every column of that union is read ONCE for all splits, and `one`, Y and W are
// read once per row. Every per-row accumulator is a register indexed at compile time (NSP is
// a template parameter, the loops over splits are unrolled).
//
// Shared bits: for every split t the moments carry the bits of ate_irm_score_moments called
// with that split's coefficient blocks at the same nbx. A thread owns the same rows, visits
// the columns in the same ascending-j order, and a column outside split t's own support has
// the coefficient 0 there: fma(0, x, acc) = acc for every finite x, so the wider union leaves
// each dot product as it was (but for an accumulator that is exactly -0.0, which becomes +0.0:
// the score adds, subtracts and compares it, so no moment changes). After the dot products the row goes through the same
// irm_accumulate, the block through the same block_sum<8>, and the partials of one split
// through the same fixed-order sum (irm_sum_multi_kernel: thread i sums blocks i, i + 256,
// ... of its split, then block_sum<8>).
constexpr int IRM_SMAX = 4;   // splits per pass: 0 bytes of scratch and >= 2 waves / SIMD for
                              // every instantiation (profiles/irm_repeated/README.md)

// stage the 3 NSP coefficient vectors of segment group g (splits s0 .. s0 + NSP - 1) and the
// column list; returns the size of the compacted union
template <int NSP, typename C>
__device__ __forceinline__ int stage_multi(C* cv, int* xc, const int* __restrict__ xcols, int p,
                                           int P, const double* __restrict__ coef, int nblk,
                                           const int* __restrict__ blk, int ngroups, int g, int s0,
                                           int* wcnt) {
  ATE_DASSERT(g >= 0 && g < ngroups && nblk >= 1);
  for (int j = threadIdx.x; j < p; j += blockDim.x) {
    xc[j] = xcols[j];
    ATE_DASSERT(xc[j] >= 0 && (P == 0 || xc[j] < P));
  }
#pragma unroll
  for (int t = 0; t < NSP; ++t) {
    const int k = blk[(int64_t)(s0 + t) * ngroups + g];
    ATE_DASSERT(k >= 0 && k < nblk);
    for (int j = threadIdx.x; j <= p; j += blockDim.x)
#pragma unroll
      for (int r = 0; r < 3; ++r)
        cv[(int64_t)j * (3 * NSP) + 3 * t + r] = (C)coef[((int64_t)k * 3 + r) * (p + 1) + j];
  }
  __syncthreads();
  return compact_support_n<3 * NSP>(cv, xc, p, wcnt);
}

template <int NSP>
__device__ __forceinline__ void write_partial_multi(double (&v)[NSP][NM], double* red,
                                                    double* partial, int s0, int nsplit) {
  double* out = partial + (((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * nsplit + s0) * NM;
#pragma unroll
  for (int t = 0; t < NSP; ++t) {
    block_sum<NM>(v[t], red);
    if (threadIdx.x == 0)
#pragma unroll
      for (int q = 0; q < NM; ++q) out[t * NM + q] = v[t][q];
  }
}

// fp32 / fp64 column-major panels: irm_score_kernel<T, RPT, MOMENTS> for NSP splits at once.
// partial: [nseg * nbx][nsplit][8], this pass writes splits s0 .. s0 + NSP - 1.
template <typename T, int RPT, int NSP>
__global__ __launch_bounds__(256) void irm_score_multi_kernel(
    const T* __restrict__ X, int64_t ld, const int* __restrict__ xcols, int p, int P,
    const Seg* __restrict__ segs, int nseg, int spf, const double* __restrict__ coef, int nblk,
    const int* __restrict__ blk /*[nsplit][ngroups]*/, int ngroups, int s0, int nsplit, int y0,
    int y1, int w0, int w1, int vcol, double clip, double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double sh[];
  constexpr int NV = 3 * NSP;
  double* cv = sh;                                // [p+1][NV]
  int* xc = (int*)(sh + (int64_t)NV * (p + 1));   // [p]
  __shared__ double red[16 * NM];
  __shared__ int wcnt[16];
  const int s = blockIdx.y;
  ATE_DASSERT(s < nseg && spf >= 1 && y0 >= 0 && w0 >= 0 && vcol >= 0);
  ATE_DASSERT(P == 0 || (y0 < P && w0 < P && vcol < P && y1 < P && w1 < P));
  ATE_DASSERT(s0 >= 0 && s0 + NSP <= nsplit);
  p = stage_multi<NSP>(cv, xc, xcols, p, P, coef, nblk, blk, ngroups, s / spf, s0, wcnt);
  const Seg sg = segs[s];
  ATE_DASSERT(sg.r0 >= 0 && sg.r0 <= sg.r1 && sg.r1 <= ld);
  double v[NSP][NM] = {};
  for (int64_t base = sg.r0 + (int64_t)blockIdx.x * 256 * RPT; base < sg.r1;
       base += (int64_t)gridDim.x * 256 * RPT) {
    double a[NSP][3][RPT];
    int64_t ii[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      ii[r] = base + r * 256 + threadIdx.x;
#pragma unroll
      for (int t = 0; t < NSP; ++t) {
        a[t][0][r] = cv[3 * t];
        a[t][1][r] = cv[3 * t + 1];
        a[t][2][r] = cv[3 * t + 2];
      }
    }
    for (int j = 0; j < p; ++j) {
      const double* cj = cv + (int64_t)(1 + j) * NV;
      const int c = xc[j];
      double x[RPT];
#pragma unroll
      for (int r = 0; r < RPT; ++r) x[r] = ii[r] < sg.r1 ? ld_col(X, ld, c, ii[r]) : 0.0;
#pragma unroll
      for (int t = 0; t < NSP; ++t) {
        const double b0 = cj[3 * t], b1 = cj[3 * t + 1], bm = cj[3 * t + 2];
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
          a[t][0][r] += b0 * x[r];
          a[t][1][r] += b1 * x[r];
          a[t][2][r] += bm * x[r];
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      if (ii[r] >= sg.r1) continue;
      if (ld_col(X, ld, vcol, ii[r]) == 0.0) continue;          // padding row
      const double y = ld_col(X, ld, y0, ii[r]) + (y1 >= 0 ? ld_col(X, ld, y1, ii[r]) : 0.0);
      const double w = ld_col(X, ld, w0, ii[r]) + (w1 >= 0 ? ld_col(X, ld, w1, ii[r]) : 0.0);
      ATE_DASSERT(spf != 2 || w == (double)(s & 1));
#pragma unroll
      for (int t = 0; t < NSP; ++t)
        irm_accumulate(v[t], y, w, a[t][0][r], a[t][1][r], a[t][2][r], clip);
    }
  }
  write_partial_multi<NSP>(v, red, partial, s0, nsplit);
}

// bf16 panels (column-major and 64-row blocked): irm_score_bf16_kernel<MOMENTS> for NSP splits
// at once -- 8 consecutive rows per thread, fp32 dot products, the score in fp64.
template <int NSP>
__global__ __launch_bounds__(256) void irm_score_multi_bf16_kernel(
    const bf16_t* __restrict__ X, int64_t cs, int64_t bs, const int* __restrict__ xcols, int p,
    int P, int64_t ld, const Seg* __restrict__ segs, int nseg, int spf,
    const double* __restrict__ coef, int nblk, const int* __restrict__ blk, int ngroups, int s0,
    int nsplit, int y0, int y1, int w0, int w1, int vcol, double clip,
    double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) float shf[];
  constexpr int NV = 3 * NSP;
  float* cv = shf;                                 // [p+1][NV]
  int* xc = (int*)(shf + (int64_t)NV * (p + 1));   // [p]
  __shared__ double red[16 * NM];
  __shared__ int wcnt[16];
  const int s = blockIdx.y;
  ATE_DASSERT(s < nseg && spf >= 1 && y0 >= 0 && w0 >= 0 && vcol >= 0);
  ATE_DASSERT(P == 0 || (y0 < P && w0 < P && vcol < P && y1 < P && w1 < P));
  ATE_DASSERT(s0 >= 0 && s0 + NSP <= nsplit);
  p = stage_multi<NSP>(cv, xc, xcols, p, P, coef, nblk, blk, ngroups, s / spf, s0, wcnt);
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
  double v[NSP][NM] = {};
  for (int64_t i = sg.r0 + ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8; i < sg.r1;
       i += (int64_t)gridDim.x * 256 * 8) {
    float a[NSP][3][8];
#pragma unroll
    for (int t = 0; t < NSP; ++t)
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        a[t][0][r] = cv[3 * t];
        a[t][1][r] = cv[3 * t + 1];
        a[t][2][r] = cv[3 * t + 2];
      }
    // 4 splits hold 160 accumulator registers: no second column in flight there
#pragma clang loop unroll_count(NSP >= 4 ? 1 : 2)
    for (int j = 0; j < p; ++j) {
      float x[8];
      ld8(xc[j], i, x);
      const float* cj = cv + (int64_t)(1 + j) * NV;
#pragma unroll
      for (int t = 0; t < NSP; ++t) {
        const float b0 = cj[3 * t], b1 = cj[3 * t + 1], bm = cj[3 * t + 2];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          a[t][0][r] += b0 * x[r];
          a[t][1][r] += b1 * x[r];
          a[t][2][r] += bm * x[r];
        }
      }
    }
    float vv[8], ya[8], yb[8], wa[8], wb[8];
    ld8(vcol, i, vv);
    ld8(y0, i, ya);
    ld8(w0, i, wa);
    if (y1 >= 0) ld8(y1, i, yb); else { for (int r = 0; r < 8; ++r) yb[r] = 0.f; }
    if (w1 >= 0) ld8(w1, i, wb); else { for (int r = 0; r < 8; ++r) wb[r] = 0.f; }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      if (vv[r] == 0.f) continue;                                 // padding row
      const double y = (double)ya[r] + (double)yb[r];
      const double w = (double)wa[r] + (double)wb[r];
      ATE_DASSERT(spf != 2 || w == (double)(s & 1));
#pragma unroll
      for (int t = 0; t < NSP; ++t)
        irm_accumulate(v[t], y, w, (double)a[t][0][r], (double)a[t][1][r], (double)a[t][2][r],
                       clip);
    }
  }
  write_partial_multi<NSP>(v, red, partial, s0, nsplit);
}

// irm_sum_kernel<8> per split: block t sums partial[b][t][:] over b in the order of the
// single-split reduction (thread i: b = i, i + 256, ...; then block_sum<8>).
__global__ __launch_bounds__(256) void irm_sum_multi_kernel(const double* __restrict__ partial,
                                                            int nb, int nsplit,
                                                            double* __restrict__ out) {
  __shared__ double red[16 * NM];
  const int t = blockIdx.x;
  ATE_DASSERT(t < nsplit);
  double v[NM] = {};
  for (int b = threadIdx.x; b < nb; b += 256)
#pragma unroll
    for (int q = 0; q < NM; ++q) v[q] += partial[((int64_t)b * nsplit + t) * NM + q];
  block_sum<NM>(v, red);
  if (threadIdx.x == 0)
#pragma unroll
    for (int q = 0; q < NM; ++q) out[(int64_t)t * NM + q] = v[q];
}

struct MultiArgs {
  int dtype;
  const void* X;
  int64_t cs, bs;
  const void* xcols;
  int p;
  const void* segs;
  int nseg, spf;
  const void* coef;
  int nblk;
  const void* blk;
  int ngroups, nsplit, y0, y1, w0, w1, vcol;
  double clip;
  int nbx;
  void* partial;
};

inline size_t multi_lds(int dtype, int p, int nsp) {
  const size_t esz = dtype == 3 ? sizeof(float) : sizeof(double);
  return (size_t)3 * nsp * (p + 1) * esz + (size_t)p * sizeof(int);
}

// one pass: splits s0 .. s0 + NSP - 1
template <int NSP>
int irm_multi_pass(const MultiArgs& a, int s0, hipStream_t s) {
  const int64_t ld = a.bs == 64 ? a.cs : 0;
  const int P = a.bs == 64 ? 0 : (int)(a.bs / 64);
  const size_t sh = multi_lds(a.dtype, a.p, NSP);
  const dim3 grid(a.nbx, a.nseg), block(256);
  if (a.dtype == 1)
    ATE_LAUNCH((irm_score_multi_kernel<float, 4, NSP>), grid, block, sh, s, (const float*)a.X, a.cs,
               (const int*)a.xcols, a.p, P, (const Seg*)a.segs, a.nseg, a.spf,
               (const double*)a.coef, a.nblk, (const int*)a.blk, a.ngroups, s0, a.nsplit, a.y0,
               a.y1, a.w0, a.w1, a.vcol, a.clip, (double*)a.partial);
  else if (a.dtype == 2)
    ATE_LAUNCH((irm_score_multi_kernel<double, 4, NSP>), grid, block, sh, s, (const double*)a.X,
               a.cs, (const int*)a.xcols, a.p, P, (const Seg*)a.segs, a.nseg, a.spf,
               (const double*)a.coef, a.nblk, (const int*)a.blk, a.ngroups, s0, a.nsplit, a.y0,
               a.y1, a.w0, a.w1, a.vcol, a.clip, (double*)a.partial);
  else
    ATE_LAUNCH(irm_score_multi_bf16_kernel<NSP>, grid, block, sh, s, (const bf16_t*)a.X, a.cs,
               a.bs, (const int*)a.xcols, a.p, P, ld, (const Seg*)a.segs, a.nseg, a.spf,
               (const double*)a.coef, a.nblk, (const int*)a.blk, a.ngroups, s0, a.nsplit, a.y0,
               a.y1, a.w0, a.w1, a.vcol, a.clip, (double*)a.partial);
  ATE_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// dtype 1 f32, 2 f64, 3 bf16. (cs, bs): element (c, i) at c*cs + (i/64)*bs + i%64 (fp32 /
// fp64 panels: column-major only, bs = 64). segs [nseg][2] int64 padded row ranges; coef
// [ceil(nseg / segs_per_fold)][3][p+1] fp64, rows (g0, g1, m), intercept first.
// partial: [nseg*nbx][8]; moments: [8].
ATE_API int ate_irm_score_moments(int dtype, const void* X, int64_t cs, int64_t bs,
                                  const void* xcols, int p, const void* segs, int nseg,
                                  int segs_per_fold, const void* coef, int y0, int y1, int w0,
                                  int w1, int vcol, double clip, int nbx, void* partial,
                                  void* moments, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int rc = irm_pass<MOMENTS>(IDENTITY, dtype, X, cs, bs, xcols, p, segs, nseg, segs_per_fold, coef, y0,
                                 y1, w0, w1, vcol, clip, nbx, partial, s);
  if (rc != 0) return rc;
  ATE_LAUNCH(irm_sum_kernel<NM>, dim3(1), dim3(256), 0, s, (const double*)partial, nbx * nseg,
             (double*)moments);
  ATE_CHECK_LAUNCH();
  return 0;
}

// The same pass, same arguments and dot products, writing the per-row scores instead:
// psi [ld] fp64 in panel row order, 0 on padding rows. Every row inside a segment is
// written; the segments of a panel tile [0, ld).
ATE_API int ate_irm_scores(int dtype, const void* X, int64_t cs, int64_t bs, const void* xcols,
                           int p, const void* segs, int nseg, int segs_per_fold,
                           const void* coef, int y0, int y1, int w0, int w1, int vcol,
                           double clip, int nbx, void* psi, void* stream) {
  return irm_pass<ROWS>(IDENTITY, dtype, X, cs, bs, xcols, p, segs, nseg, segs_per_fold, coef, y0, y1, w0,
                        w1, vcol, clip, nbx, psi, (hipStream_t)stream);
}

// The pass of ate_irm_score_moments -- same arguments and checks, same column reads, dot
// products and psi -- accumulating the 14 moments of the sensitivity analysis (irm_accumulate
// above). partial: [nseg*nbx][14]; moments: [14]. For the same nbx, moments 0-3 and 13 carry
// the bits of moments 0-3 and 7 of ate_irm_score_moments (same per-thread order, same
// reduction shape).
ATE_API int ate_irm_sens_moments(int dtype, const void* X, int64_t cs, int64_t bs,
                                 const void* xcols, int p, const void* segs, int nseg,
                                 int segs_per_fold, const void* coef, int y0, int y1, int w0,
                                 int w1, int vcol, double clip, int nbx, void* partial,
                                 void* moments, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int rc = irm_pass<SENS>(IDENTITY, dtype, X, cs, bs, xcols, p, segs, nseg, segs_per_fold, coef, y0,
                                y1, w0, w1, vcol, clip, nbx, partial, s);
  if (rc != 0) return rc;
  ATE_LAUNCH(irm_sum_kernel<NS>, dim3(1), dim3(256), 0, s, (const double*)partial, nbx * nseg,
             (double*)moments);
  ATE_CHECK_LAUNCH();
  return 0;
}

// The pass of ate_irm_score_moments -- same arguments and checks, same column reads, dot
// products and psi -- accumulating the 12 moments of the target populations (irm_accumulate
// above; result.TARGET_MOMENTS): the average effect over all rows, on the treated and on the
// controls with their joint covariance. partial: [nseg*nbx][12]; moments: [12]. For the same
// nbx, moments 0-3 and 11 carry the bits of moments 0-3 and 7 of ate_irm_score_moments (same
// per-thread order, same reduction shape). An all-zero coefficient row (a nuisance the
// requested targets do not need) adds no column to the support.
ATE_API int ate_irm_target_moments(int dtype, const void* X, int64_t cs, int64_t bs,
                                   const void* xcols, int p, const void* segs, int nseg,
                                   int segs_per_fold, const void* coef, int y0, int y1, int w0,
                                   int w1, int vcol, double clip, int nbx, void* partial,
                                   void* moments, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int rc = irm_pass<TARGETS>(IDENTITY, dtype, X, cs, bs, xcols, p, segs, nseg, segs_per_fold, coef,
                                   y0, y1, w0, w1, vcol, clip, nbx, partial, s);
  if (rc != 0) return rc;
  ATE_LAUNCH(irm_sum_kernel<NT>, dim3(1), dim3(256), 0, s, (const double*)partial, nbx * nseg,
             (double*)moments);
  ATE_CHECK_LAUNCH();
  return 0;
}

// The four passes above with the link of the propensity row chosen by the caller. mode: 0 the
// 8 moments, 1 psi per row (`partial` is psi [ld], `moments` unused), 2 the 14 moments of the
// sensitivity analysis, 3 the 12 moments of the targets. link: 0 identity -- the bits of the
// entry points above -- or 1 logistic: coefficient row 2 holds logit coefficients and
// m = 1 / (1 + exp(-eta)) before the score sees it. fp32 / fp64 panels only with link 1.
ATE_API int ate_irm_score_link(int mode, int link, int dtype, const void* X, int64_t cs,
                               int64_t bs, const void* xcols, int p, const void* segs, int nseg,
                               int segs_per_fold, const void* coef, int y0, int y1, int w0, int w1,
                               int vcol, double clip, int nbx, void* partial, void* moments,
                               void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (mode < MOMENTS || mode > TARGETS) return -1;
  auto pass = mode == MOMENTS ? irm_pass<MOMENTS> : mode == ROWS ? irm_pass<ROWS>
              : mode == SENS  ? irm_pass<SENS> : irm_pass<TARGETS>;
  const int rc = pass(link, dtype, X, cs, bs, xcols, p, segs, nseg, segs_per_fold, coef, y0, y1,
                      w0, w1, vcol, clip, nbx, partial, s);
  if (rc != 0 || mode == ROWS) return rc;
  if (mode == MOMENTS)
    ATE_LAUNCH(irm_sum_kernel<NM>, dim3(1), dim3(256), 0, s, (const double*)partial, nbx * nseg,
               (double*)moments);
  else if (mode == SENS)
    ATE_LAUNCH(irm_sum_kernel<NS>, dim3(1), dim3(256), 0, s, (const double*)partial, nbx * nseg,
               (double*)moments);
  else
    ATE_LAUNCH(irm_sum_kernel<NT>, dim3(1), dim3(256), 0, s, (const double*)partial, nbx * nseg,
               (double*)moments);
  ATE_CHECK_LAUNCH();
  return 0;
}

// The most splits one pass of ate_irm_score_moments_multi serves.
ATE_API int ate_irm_score_multi_smax() { return IRM_SMAX; }

// The pass of ate_irm_score_moments for nsplit partitions of the same segments at once
// (repeated cross-fitting). coef: [nblk][3][p+1] fp64; blk: int32 [nsplit][ngroups] on the
// device, ngroups = ceil(nseg / segs_per_fold) -- segment group g uses block blk[t][g] under
// split t (every entry in [0, nblk): the caller checks them, the debug build asserts it).
// partial: [nseg*nbx][nsplit][8]; moments: [nsplit][8]. moments[t] carries the bits of
// ate_irm_score_moments with coef gathered by blk[t] at the same nbx (see the kernels). The
// panel is read ceil(nsplit / n) times, n = the most splits per pass: IRM_SMAX, or fewer
// when 3 n coefficient vectors would not fit the LDS bound of the single-split pass.
ATE_API int ate_irm_score_moments_multi(int dtype, const void* X, int64_t cs, int64_t bs,
                                        const void* xcols, int p, const void* segs, int nseg,
                                        int segs_per_fold, const void* coef, int nblk,
                                        const void* blk, int nsplit, int y0, int y1, int w0,
                                        int w1, int vcol, double clip, int nbx, void* partial,
                                        void* moments, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (dtype < 1 || dtype > 3 || (dtype != 3 && bs != 64)) return -1;
  if (p < 0 || nseg < 1 || nseg > 65535 || segs_per_fold < 1 || nbx < 1 || cs < 64 || bs < 64)
    return -1;
  if (y0 < 0 || w0 < 0 || vcol < 0) return -1;
  if (nblk < 1 || nsplit < 1 || nsplit > 65535 || blk == nullptr || coef == nullptr) return -1;
  if (!(clip >= 0.0 && clip < 0.5)) return -1;
  int per = IRM_SMAX;                        // dynamic + static LDS within the 64 KB default
  while (per > 1 && multi_lds(dtype, p, per) > 64 * 1024 - 2048) --per;
  if (multi_lds(dtype, p, per) > 64 * 1024 - 2048) return -1;
  const MultiArgs a{dtype, X, cs, bs, xcols, p, segs, nseg, segs_per_fold, coef, nblk, blk,
                    (nseg + segs_per_fold - 1) / segs_per_fold, nsplit, y0, y1, w0, w1, vcol,
                    clip, nbx, partial};
  static_assert(IRM_SMAX == 4, "one case per instantiation below");
  for (int s0 = 0; s0 < nsplit; s0 += per) {
    const int n = nsplit - s0 < per ? nsplit - s0 : per;
    int rc = -1;
    switch (n) {
      case 1: rc = irm_multi_pass<1>(a, s0, s); break;
      case 2: rc = irm_multi_pass<2>(a, s0, s); break;
      case 3: rc = irm_multi_pass<3>(a, s0, s); break;
      case 4: rc = irm_multi_pass<4>(a, s0, s); break;
    }
    if (rc != 0) return rc;
  }
  ATE_LAUNCH(irm_sum_multi_kernel, dim3(nsplit), dim3(256), 0, s, (const double*)partial,
             nbx * nseg, nsplit, (double*)moments);
  ATE_CHECK_LAUNCH();
  return 0;
}
