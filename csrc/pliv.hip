// Fused held-out pass of the cross-fitted partially linear IV model (DML-PLIV, Chernozhukov
// et al. 2018 §4.2; DoubleML DoubleMLPLIV, partialling-out score): a real treatment D with
// an endogeneity problem, Q = 1..4 instruments Z_1..Z_Q, linear nuisances.
//
// The panel is the plain K-fold panel (segment k = fold k) with Y, D and the Q instruments
// in target columns. For every row i of segment s, with the 2 + Q coefficient vectors
// (l, r, m_1..m_Q) of block s:
//   l = E[Y|X]   r = E[D|X]   m_j = E[Z_j|X]
//   y~ = y - l   d~ = d - r   z~_j = z_j - m_j
// and the N(Q) = 4 + 2Q + 2Q(Q+1) moments (result.PlivLayout; T = Q(Q+1)/2)
//   0 n   1 S y~y~   2 S y~d~   3 S d~d~
//   4 + i          S z~_i y~
//   4 + Q + i      S z~_i d~
//   4 + 2Q + t     S z~_i z~_j          (i <= j, t row-major over the upper triangle)
//   4 + 2Q + T + t      Q_yy = S z~_i z~_j y~y~
//   4 + 2Q + 2T + t     Q_yd = S z~_i z~_j y~d~
//   4 + 2Q + 3T + t     Q_dd = S z~_i z~_j d~d~
// are accumulated in fp64; no per-row value is written to HBM. The 2 + Q vectors are staged
// in LDS interleaved per column (cv[j * NV + r]), the ordered union of their supports is
// compacted (irm_common.hpp compact_support_n) and every column of it is read ONCE; `one`
// and the 2 + Q targets once per row (hi + lo pairs on bf16 panels). Per-workgroup partials,
// then ONE single-workgroup launch sums them in a fixed order (no atomics: equal bits run to
// run at a given geometry) and finishes: one lane factors S z~z~' (Cholesky, fp64) and writes
//   res = [theta, SE, pi' S z~d~, rank flag, pi_1..pi_Q]
//   pi    = (S z~z~')^-1 S z~d~
//   theta = pi' S z~y~ / pi' S z~d~
//   Omega = Q_yy - 2 theta Q_yd + theta^2 Q_dd,   SE = sqrt(pi' Omega pi) / (pi' S z~d~)
// A pivot at or below 1e-12 times the largest diagonal entry sets the flag (1.0) and makes
// every other entry NaN. ate_pliv_terms is the same row pass writing a_i = v_i y~_i and
// b_i = v_i d~_i, v_i = z~_i' pi, the per-row terms of the cluster-robust variance
// (csrc/cluster.hip: psi = a - theta b).
#include "irm_common.hpp"

using namespace ate;

namespace {

constexpr int PLIV_QMAX = 4;
constexpr int pliv_n(int Q) { return 4 + 2 * Q + 2 * Q * (Q + 1); }      // 10 / 20 / 34 / 52
// rows per thread of the fp32 / fp64 kernels: the accumulators are 2 N(Q) VGPRs and the dot
// products 2 (2 + Q) RPT, so the wider moment vectors take fewer rows (no scratch)
constexpr int pliv_rpt(int Q) { return Q <= 2 ? 4 : 2; }
// static LDS of a kernel here: red[16 N(4)] = 6656 bytes and wcnt; the dynamic part gets
// what 8 KB leave
constexpr int PLIV_LDS_MAX = 64 * 1024 - 8192;
static_assert(16 * pliv_n(PLIV_QMAX) * sizeof(double) + 64 <= 8192, "static LDS of the pass");

// one valid row's contribution to the N(Q) moments; rz: the Q instrument residuals
template <int Q>
__device__ __forceinline__ void pliv_accumulate(double (&v)[pliv_n(Q)], double ry, double rd,
                                                const double (&rz)[Q]) {
  constexpr int T = Q * (Q + 1) / 2;
  const double yy = ry * ry, yd = ry * rd, dd = rd * rd;
  v[0] += 1.0;
  v[1] += yy;
  v[2] += yd;
  v[3] += dd;
#pragma unroll
  for (int i = 0; i < Q; ++i) {
    v[4 + i] += rz[i] * ry;
    v[4 + Q + i] += rz[i] * rd;
  }
#pragma unroll
  for (int i = 0; i < Q; ++i)
#pragma unroll
    for (int j = i; j < Q; ++j) {
      const int t = i * Q - i * (i - 1) / 2 + (j - i);
      const double zz = rz[i] * rz[j];
      v[4 + 2 * Q + t] += zz;
      v[4 + 2 * Q + T + t] += zz * yy;
      v[4 + 2 * Q + 2 * T + t] += zz * yd;
      v[4 + 2 * Q + 3 * T + t] += zz * dd;
    }
}

// stage the NV coefficient vectors of block k, interleaved per column, the column list and
// the target columns; returns the size of the compacted union
template <int NV, typename C>
__device__ __forceinline__ int pliv_stage(C* cv, int* xc, const int* __restrict__ xcols, int p,
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

// the (first, second) columns of the 2 + Q targets (Y, D, Z_1..Z_Q); second = -1 unless the
// target is stored as a hi + lo bf16 pair
template <int NV>
__device__ __forceinline__ void pliv_targets(const int* __restrict__ tcols, int P, int (&c0)[NV],
                                             int (&c1)[NV]) {
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    c0[q] = tcols[2 * q];
    c1[q] = tcols[2 * q + 1];
    ATE_DASSERT(c0[q] >= 0 && c1[q] >= -1 && (P == 0 || (c0[q] < P && c1[q] < P)));
  }
}

// fp32 / fp64 column-major panels: fp64 dot products, RPT rows per thread 256 apart (the row
// ownership of dml_resid_body). TERMS: write a = v y~, b = v d~ (ta, tb: [ld], 0 on padding
// rows) instead of summing moments; partial is not touched then. partial: [nseg * nbx][N(Q)].
template <typename T, int Q, bool TERMS>
__global__ __launch_bounds__(256) void pliv_kernel(
    const T* __restrict__ X, int64_t ld, const int* __restrict__ xcols, int p,
    const Seg* __restrict__ segs, int nseg, const double* __restrict__ coef /*[nseg][2+Q][p+1]*/,
    const int* __restrict__ tcols /*[2 (2+Q)]*/, int vcol, double* __restrict__ partial,
    const double* __restrict__ pi /*[Q]*/, double* __restrict__ ta, double* __restrict__ tb) {
  constexpr int NV = 2 + Q, NM = pliv_n(Q), RPT = pliv_rpt(Q);
  extern __shared__ __attribute__((aligned(16))) double sh[];
  double* cv = sh;                                // [p+1][NV]
  int* xc = (int*)(sh + (int64_t)NV * (p + 1));   // [p]
  __shared__ double red[TERMS ? 1 : 16 * NM];
  __shared__ int wcnt[16];
  const int s = blockIdx.y;
  ATE_DASSERT(s < nseg && vcol >= 0 && p >= 0);
  int c0[NV], c1[NV];
  pliv_targets<NV>(tcols, 0, c0, c1);
  p = pliv_stage<NV>(cv, xc, xcols, p, 0, coef, s, wcnt);
  const Seg sg = segs[s];
  ATE_DASSERT(sg.r0 >= 0 && sg.r0 <= sg.r1 && sg.r1 <= ld);
  double w[Q];
  if constexpr (TERMS) {
#pragma unroll
    for (int i = 0; i < Q; ++i) w[i] = pi[i];
  }
  double v[NM] = {};
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
      if (ld_col(X, ld, vcol, ii[r]) == 0.0) {                    // padding row
        if constexpr (TERMS) { ta[ii[r]] = 0.0; tb[ii[r]] = 0.0; }
        continue;
      }
      double res[NV];
#pragma unroll
      for (int q = 0; q < NV; ++q)
        res[q] = ld_col(X, ld, c0[q], ii[r]) + (c1[q] >= 0 ? ld_col(X, ld, c1[q], ii[r]) : 0.0) -
                 a[q][r];
      double rz[Q];
#pragma unroll
      for (int i = 0; i < Q; ++i) rz[i] = res[2 + i];
      if constexpr (TERMS) {
        double u = 0.0;
#pragma unroll
        for (int i = 0; i < Q; ++i) u += rz[i] * w[i];
        ta[ii[r]] = u * res[0];
        tb[ii[r]] = u * res[1];
      } else {
        pliv_accumulate<Q>(v, res[0], res[1], rz);
      }
    }
  }
  if constexpr (!TERMS) write_partial<NM>(v, red, partial);
}

// bf16 panels (column-major and 64-row blocked): each thread owns 8 CONSECUTIVE rows, so
// every column read is one 16-byte load through (cs, bs); dot products in fp32 (bf16 values
// are exact in fp32; coefficients rounded to fp32), residuals and moments in fp64 (the row
// ownership and arithmetic of dml_resid_bf16_body).
template <int Q, bool TERMS>
__global__ __launch_bounds__(256) void pliv_bf16_kernel(
    const bf16_t* __restrict__ X, int64_t cs, int64_t bs, const int* __restrict__ xcols, int p,
    int P, int64_t ld, const Seg* __restrict__ segs, int nseg, const double* __restrict__ coef,
    const int* __restrict__ tcols, int vcol, double* __restrict__ partial,
    const double* __restrict__ pi, double* __restrict__ ta, double* __restrict__ tb) {
  constexpr int NV = 2 + Q, NM = pliv_n(Q);
  extern __shared__ __attribute__((aligned(16))) float shf[];
  float* cv = shf;                                 // [p+1][NV]
  int* xc = (int*)(shf + (int64_t)NV * (p + 1));   // [p]
  __shared__ double red[TERMS ? 1 : 16 * NM];
  __shared__ int wcnt[16];
  const int s = blockIdx.y;
  ATE_DASSERT(s < nseg && vcol >= 0 && (P == 0 || vcol < P) && p >= 0);
  int c0[NV], c1[NV];
  pliv_targets<NV>(tcols, P, c0, c1);
  p = pliv_stage<NV>(cv, xc, xcols, p, P, coef, s, wcnt);
  const Seg sg = segs[s];
  ATE_DASSERT(sg.r0 >= 0 && sg.r0 <= sg.r1 && (ld == 0 || sg.r1 <= ld) && (sg.r0 & 7) == 0 &&
              (sg.r1 & 7) == 0);
  auto ld8 = [&](int c, int64_t i, float (&o)[8]) {
    ATE_DASSERT((i & 7) == 0 && c >= 0 && (P == 0 || c < P) && (ld == 0 || i + 8 <= ld));
    // (c, i) at c*cs + (i/64)*bs + i%64; the 8 rows never straddle a block (i % 8 == 0)
    const uint4 u = *reinterpret_cast<const uint4*>(X + (int64_t)c * cs + (i >> 6) * bs + (i & 63));
    const uint32_t wd[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      o[2 * q] = __uint_as_float(wd[q] << 16);
      o[2 * q + 1] = __uint_as_float(wd[q] & 0xFFFF0000u);
    }
  };
  double w[Q];
  if constexpr (TERMS) {
#pragma unroll
    for (int i = 0; i < Q; ++i) w[i] = pi[i];
  }
  double v[NM] = {};
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
    // the residuals, target by target: each frees its fp32 dot products as it goes
    double res[NV][8];
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      float hi[8], lo[8];
      ld8(c0[q], i, hi);
      if (c1[q] >= 0) ld8(c1[q], i, lo); else { for (int r = 0; r < 8; ++r) lo[r] = 0.f; }
#pragma unroll
      for (int r = 0; r < 8; ++r) res[q][r] = ((double)hi[r] + (double)lo[r]) - (double)a[q][r];
    }
    float vv[8];
    ld8(vcol, i, vv);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      if (vv[r] == 0.f) {                                         // padding row
        if constexpr (TERMS) { ta[i + r] = 0.0; tb[i + r] = 0.0; }
        continue;
      }
      double rz[Q];
#pragma unroll
      for (int q = 0; q < Q; ++q) rz[q] = res[2 + q][r];
      if constexpr (TERMS) {
        double u = 0.0;
#pragma unroll
        for (int q = 0; q < Q; ++q) u += rz[q] * w[q];
        ta[i + r] = u * res[0][r];
        tb[i + r] = u * res[1][r];
      } else {
        pliv_accumulate<Q>(v, res[0][r], res[1][r], rz);
      }
    }
  }
  if constexpr (!TERMS) write_partial<NM>(v, red, partial);
}

// upper-triangle entry (i, j) of a row-major packed symmetric matrix
__device__ __forceinline__ int pliv_tri(int Q, int i, int j) {
  const int a = i < j ? i : j, b = i < j ? j : i;
  return a * Q - a * (a - 1) / 2 + (b - a);
}

// One workgroup of 256 threads: thread i sums partials i, i + 256, ... (fixed order), a
// fixed-shape block reduction (irm_sum_kernel's), then thread 0 finishes (the file header's
// formulas; the CPU twin is estimators/pliv.py pliv_finalize, operation by operation).
template <int Q>
__global__ __launch_bounds__(256) void pliv_finish_kernel(const double* __restrict__ partial,
                                                          int nb, double* __restrict__ mom,
                                                          double* __restrict__ res /*[4+Q]*/) {
  constexpr int NM = pliv_n(Q), T = Q * (Q + 1) / 2;
  __shared__ double red[16 * NM];
  __shared__ double m[NM];
  double v[NM] = {};
  for (int b = threadIdx.x; b < nb; b += 256)
#pragma unroll
    for (int q = 0; q < NM; ++q) v[q] += partial[(int64_t)b * NM + q];
  block_sum<NM>(v, red);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int q = 0; q < NM; ++q) { mom[q] = v[q]; m[q] = v[q]; }
  // from here on the indices are run-time values: the moments are read from LDS
  const double* sy = m + 4;
  const double* sd = m + 4 + Q;
  const double* S = m + 4 + 2 * Q;
  const double* Qyy = S + T;
  const double* Qyd = S + 2 * T;
  const double* Qdd = S + 3 * T;
  __shared__ double L[PLIV_QMAX][PLIV_QMAX], pv[PLIV_QMAX], f[PLIV_QMAX];   // one lane's
  double dmax = 0.0;
  for (int i = 0; i < Q; ++i) dmax = fmax(dmax, S[pliv_tri(Q, i, i)]);
  bool bad = !(dmax > 0.0);
  for (int j = 0; j < Q && !bad; ++j) {
    double d = S[pliv_tri(Q, j, j)];
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 1e-12 * dmax)) { bad = true; break; }
    L[j][j] = sqrt(d);
    for (int i = j + 1; i < Q; ++i) {
      double t = S[pliv_tri(Q, i, j)];
      for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
      L[i][j] = t / L[j][j];
    }
  }
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  if (bad) {
    res[0] = nan; res[1] = nan; res[2] = nan; res[3] = 1.0;
    for (int i = 0; i < Q; ++i) res[4 + i] = nan;
    return;
  }
  for (int i = 0; i < Q; ++i) {                   // L f = S z~d~
    double t = sd[i];
    for (int k = 0; k < i; ++k) t -= L[i][k] * f[k];
    f[i] = t / L[i][i];
  }
  for (int i = Q - 1; i >= 0; --i) {              // L' pi = f
    double t = f[i];
    for (int k = i + 1; k < Q; ++k) t -= L[k][i] * pv[k];
    pv[i] = t / L[i][i];
  }
  double num = 0.0, den = 0.0;
  for (int i = 0; i < Q; ++i) { num += pv[i] * sy[i]; den += pv[i] * sd[i]; }
  const double th = num / den;
  double var = 0.0;
  for (int i = 0; i < Q; ++i)
    for (int j = 0; j < Q; ++j) {
      const int t = pliv_tri(Q, i, j);
      var += pv[i] * pv[j] * (Qyy[t] - 2.0 * th * Qyd[t] + th * th * Qdd[t]);
    }
  res[0] = th;
  res[1] = sqrt(var > 0.0 ? var : 0.0) / den;
  res[2] = den;
  res[3] = 0.0;
  for (int i = 0; i < Q; ++i) res[4 + i] = pv[i];
}

struct PlivArgs {
  int dtype;
  const void* X;
  int64_t cs, bs;
  const void* xcols;
  int p;
  const void* segs;
  int nseg;
  const void* coef;
  const void* tcols;
  int vcol, nbx;
  void* partial;
  const void* pi;
  void* ta;
  void* tb;
  hipStream_t s;
};

// the row pass of one Q: the moment kernel (TERMS false) or the term kernel
template <int Q, bool TERMS>
int pliv_launch(const PlivArgs& a) {
  constexpr int NV = 2 + Q;
  const size_t esz = a.dtype == 3 ? sizeof(float) : sizeof(double);
  const size_t sh = (size_t)NV * (a.p + 1) * esz + (size_t)a.p * sizeof(int);
  if (sh > (size_t)PLIV_LDS_MAX) return -1;
  const dim3 grid(a.nbx, a.nseg);
  // what the strides say about the panel's extent, for the debug build's bounds checks
  // (0 = unknown): column-major (bs = 64) has ld = cs rows; 64-row blocked has P = bs / 64
  const int64_t ld = a.bs == 64 ? a.cs : 0;
  const int P = a.bs == 64 ? 0 : (int)(a.bs / 64);
  if (a.dtype == 1)
    ATE_LAUNCH((pliv_kernel<float, Q, TERMS>), grid, dim3(256), sh, a.s, (const float*)a.X, a.cs,
               (const int*)a.xcols, a.p, (const Seg*)a.segs, a.nseg, (const double*)a.coef,
               (const int*)a.tcols, a.vcol, (double*)a.partial, (const double*)a.pi,
               (double*)a.ta, (double*)a.tb);
  else if (a.dtype == 2)
    ATE_LAUNCH((pliv_kernel<double, Q, TERMS>), grid, dim3(256), sh, a.s, (const double*)a.X,
               a.cs, (const int*)a.xcols, a.p, (const Seg*)a.segs, a.nseg, (const double*)a.coef,
               (const int*)a.tcols, a.vcol, (double*)a.partial, (const double*)a.pi,
               (double*)a.ta, (double*)a.tb);
  else
    ATE_LAUNCH((pliv_bf16_kernel<Q, TERMS>), grid, dim3(256), sh, a.s, (const bf16_t*)a.X, a.cs,
               a.bs, (const int*)a.xcols, a.p, P, ld, (const Seg*)a.segs, a.nseg,
               (const double*)a.coef, (const int*)a.tcols, a.vcol, (double*)a.partial,
               (const double*)a.pi, (double*)a.ta, (double*)a.tb);
  ATE_CHECK_LAUNCH();
  return 0;
}

template <int Q>
int pliv_moments_q(const PlivArgs& a, void* moments, void* res) {
  const int rc = pliv_launch<Q, false>(a);
  if (rc != 0) return rc;
  ATE_LAUNCH(pliv_finish_kernel<Q>, dim3(1), dim3(256), 0, a.s, (const double*)a.partial,
             a.nbx * a.nseg, (double*)moments, (double*)res);
  ATE_CHECK_LAUNCH();
  return 0;
}

// the argument checks both entry points share (-1: rejected, nothing launched)
bool pliv_args_ok(int dtype, int64_t cs, int64_t bs, int p, int nseg, int q, int vcol, int nbx) {
  if (dtype < 1 || dtype > 3 || (dtype != 3 && bs != 64)) return false;
  if (p < 0 || nseg < 1 || nseg > 65535 || nbx < 1 || cs < 64 || bs < 64) return false;
  return q >= 1 && q <= PLIV_QMAX && vcol >= 0;
}

}  // namespace

// the largest launch of each instantiation, for the debug build's load-time resource check
#define PLIV_SHAPE(tag, Q, name, lds, ...) \
  static ate::KernelShapeReg pliv_kshape_##tag##Q((const void*)(__VA_ARGS__), name, 256, lds);
#define PLIV_SHAPES(Q)                                                                       \
  PLIV_SHAPE(f, Q, "pliv_kernel<float," #Q ">", PLIV_LDS_MAX, pliv_kernel<float, Q, false>)   \
  PLIV_SHAPE(d, Q, "pliv_kernel<double," #Q ">", PLIV_LDS_MAX, pliv_kernel<double, Q, false>) \
  PLIV_SHAPE(b, Q, "pliv_bf16_kernel<" #Q ">", PLIV_LDS_MAX, pliv_bf16_kernel<Q, false>)      \
  PLIV_SHAPE(tf, Q, "pliv_terms_kernel<float," #Q ">", PLIV_LDS_MAX,                          \
             pliv_kernel<float, Q, true>)                                                     \
  PLIV_SHAPE(td, Q, "pliv_terms_kernel<double," #Q ">", PLIV_LDS_MAX,                         \
             pliv_kernel<double, Q, true>)                                                    \
  PLIV_SHAPE(tb, Q, "pliv_terms_bf16_kernel<" #Q ">", PLIV_LDS_MAX, pliv_bf16_kernel<Q, true>) \
  PLIV_SHAPE(s, Q, "pliv_finish_kernel<" #Q ">", 0, pliv_finish_kernel<Q>)
PLIV_SHAPES(1)
PLIV_SHAPES(2)
PLIV_SHAPES(3)
PLIV_SHAPES(4)

// The dynamic LDS one workgroup of the pass may use: (2 + q)(p + 1) esz + 4 p must fit
// (esz: 4 on bf16 panels, 8 otherwise); the host checks it before any device work.
ATE_API int ate_pliv_lds_max() { return PLIV_LDS_MAX; }

// The PLIV pass. dtype 1 f32, 2 f64, 3 bf16. (cs, bs): element (c, i) at c*cs + (i/64)*bs +
// i%64 (fp32 / fp64 panels: column-major only, bs = 64). segs [nseg][2] int64 padded row
// ranges; coef [nseg][2+q][p+1] fp64, rows (l, r, m_1..m_q), intercept first; tcols
// [2 (2+q)] int32 on the device: the (first, second) columns of Y, D, Z_1..Z_q (second = -1
// unless the target is a hi + lo bf16 pair). partial: [nseg*nbx][N(q)]; moments: [N(q)];
// res: [4+q] = [theta, SE, pi'S z~d~, rank flag, pi]. -1 (nothing launched): a dtype, stride,
// q outside 1..4, count or column the pass does not take, or (2+q)(p+1) esz + 4 p over the LDS.
ATE_API int ate_pliv_moments(int dtype, const void* X, int64_t cs, int64_t bs, const void* xcols,
                             int p, const void* segs, int nseg, int q, const void* coef,
                             const void* tcols, int vcol, int nbx, void* partial, void* moments,
                             void* res, void* stream) {
  if (!pliv_args_ok(dtype, cs, bs, p, nseg, q, vcol, nbx)) return -1;
  if (!X || !xcols || !segs || !coef || !tcols || !partial || !moments || !res) return -1;
  const PlivArgs a{dtype, X, cs, bs, xcols, p, segs, nseg, coef, tcols, vcol, nbx, partial,
                   nullptr, nullptr, nullptr, (hipStream_t)stream};
  switch (q) {
    case 1: return pliv_moments_q<1>(a, moments, res);
    case 2: return pliv_moments_q<2>(a, moments, res);
    case 3: return pliv_moments_q<3>(a, moments, res);
    default: return pliv_moments_q<4>(a, moments, res);
  }
}

// The same row pass -- same arguments, same dot products, same residuals -- writing every
// row's a = v y~ and b = v d~ with v = z~' pi (ta, tb: [ld] fp64, panel row order, 0 on
// padding rows); pi [q] fp64 on the device (res + 4 of ate_pliv_moments, written earlier on
// the stream). The segments must tile [0, ld): every row is written.
ATE_API int ate_pliv_terms(int dtype, const void* X, int64_t cs, int64_t bs, const void* xcols,
                           int p, const void* segs, int nseg, int q, const void* coef,
                           const void* tcols, int vcol, int nbx, const void* pi, void* ta,
                           void* tb, void* stream) {
  if (!pliv_args_ok(dtype, cs, bs, p, nseg, q, vcol, nbx)) return -1;
  if (!X || !xcols || !segs || !coef || !tcols || !pi || !ta || !tb) return -1;
  const PlivArgs a{dtype, X, cs, bs, xcols, p, segs, nseg, coef, tcols, vcol, nbx, nullptr,
                   pi, ta, tb, (hipStream_t)stream};
  switch (q) {
    case 1: return pliv_launch<1, true>(a);
    case 2: return pliv_launch<2, true>(a);
    case 3: return pliv_launch<3, true>(a);
    default: return pliv_launch<4, true>(a);
  }
}
