// Fused held-out score pass of the cross-fitted interactive model with a MULTI-VALUED
// treatment (DML-APOS: DoubleML DoubleMLAPO / DoubleMLAPOS, grf multi_arm_causal_forest): the
// mean potential outcome of every treatment level, with their joint second moments.
//
// D takes L levels 0..L-1 (2 <= L <= 8, a compile-time parameter). The panel is the
// level-split fold panel: segment L k + c = the rows of fold k with D = c. The coefficients
// are coef [nfold][2L][p+1] fp64, intercept first: rows 0..L-1 the outcome regressions
// g_c = E[Y | X, D = c], rows L..2L-1 the one-vs-rest propensities m_c = P(D = c | X). A
// workgroup of segment s, with k = s / L and its level lev = s % L, scores its rows by
//   e     = min(max(m_lev, clip), 1 - clip)
//   ind   = 1{D = lev}                        (D is read from the panel on every row)
//   psi_c = g_c + 1{c = lev} ind (y - g_lev) / e             c = 0..L-1
// and accumulates in fp64, with no per-row value written to HBM, the N(L) = 1 + L +
// L(L+1)/2 + 4L moments (result.apo_layout; 14 at L = 2, 77 at L = 8)
//   [0]                n
//   [1 + c]            S psi_c
//   [1 + L + t(c,c')]  S psi_c psi_c'   c <= c', row-major over the upper triangle
//   [B + 4c + 0..3]    n_c, n_clipped_c (rows of level c with m_c outside the clip),
//                      S 1{D=c}(y - g_c)^2, S 1{D=c} / e_c            B = 1 + L + L(L+1)/2
// A row costs L + 1 dot products (every g_c, and only its own level's m) and ONE fp64
// division: 1 / e, which the score and the weight sum share.
//
// The L outcome vectors of block k and the one propensity vector of level lev are staged in
// LDS interleaved per column (cv[j * (L+1) + r], as csrc/iivm.hip), the ordered union of
// their supports is compacted, every column of that union is read ONCE, and `one`, Y and D
// once per row. A workgroup's rows all have one level, so of the 4L per-level moments only
// its own four can be nonzero: a thread carries NA(L) = 1 + L + L(L+1)/2 + 4 accumulators,
// block_sum reduces those, and thread 0 writes the N(L)-long partial with zeros in the other
// levels' slots (write_level_partial: write_partial of irm_common.hpp with that expansion).
// The partials go through apo_sum_kernel<N>: irm_sum_kernel<N>'s fixed-order sum, moment by
// moment, spread over workgroups of 16 moments; no atomics.
//
// Shared bits at L = 2, at the same nbx: row ownership, column order and the zero
// coefficients of a wider union are those of irm_score_kernel / irm_score_bf16_kernel (the
// argument of csrc/iivm.hip's header), (y - g_lev)^2 is multiplied by exactly 1.0 where
// irm_accumulate multiplies by w or 1 - w, and a workgroup of the other level contributes an
// exact zero where irm_accumulate adds 0 * r^2. So S 1{D=0}(y-g_0)^2, S 1{D=1}(y-g_1)^2, n
// and n_1 carry the bits of ate_irm_score_moments [5], [4], [2], [7] called with the rows
// (g_0, g_1, m_1).
#include "irm_common.hpp"

using namespace ate;

namespace {

constexpr int APO_LMAX = 8;
constexpr int ntri(int L) { return L * (L + 1) / 2; }
constexpr int apo_na(int L) { return 1 + L + ntri(L) + 4; }        // a thread's accumulators
constexpr int apo_n(int L) { return 1 + L + ntri(L) + 4 * L; }     // the moments
// static LDS of a score kernel: red[16 NA] doubles + wcnt[16] ints
constexpr int apo_static_lds(int L) { return 16 * apo_na(L) * 8 + 64; }
// rows per thread of the fp32 / fp64 kernel: 4 (irm_score_kernel's) while the accumulators
// leave room for 4 (L+1) fp64 dot products, 2 beyond (profiles/apos/README.md)
constexpr int apo_rpt(int L) { return L <= 4 ? 4 : 2; }

// one valid row's contribution; g: the L outcome regressions, m: the raw propensity of lev
template <int L>
__device__ __forceinline__ void apo_accumulate(double (&v)[apo_na(L)], double y, double d, int lev,
                                               const double (&g)[L], double m, double clip) {
  const double lo = clip, hi = 1.0 - clip;
  const double e = m < lo ? lo : (m > hi ? hi : m);
  const double ind = d == (double)lev ? 1.0 : 0.0;
  double gl = g[0];
#pragma unroll
  for (int c = 1; c < L; ++c) gl = c == lev ? g[c] : gl;   // selects: no dynamic register index
  const double r = y - gl;
  const double ie = 1.0 / e;
  const double t = ind * (r * ie);
  double psi[L];
#pragma unroll
  for (int c = 0; c < L; ++c) psi[c] = c == lev ? g[c] + t : g[c];
  v[0] += 1.0;
#pragma unroll
  for (int c = 0; c < L; ++c) v[1 + c] += psi[c];
  int q = 1 + L;
#pragma unroll
  for (int c = 0; c < L; ++c)
#pragma unroll
    for (int c2 = c; c2 < L; ++c2) v[q++] += psi[c] * psi[c2];
  v[q] += ind;
  v[q + 1] += ind * ((m < lo || m > hi) ? 1.0 : 0.0);
  v[q + 2] += ind * (r * r);
  v[q + 3] += ind * ie;
}

// write_partial (irm_common.hpp) for the NA accumulators of a workgroup of level lev: the
// block sum, then the N-long partial with the four per-level sums in lev's slots
template <int L>
__device__ __forceinline__ void write_level_partial(double (&v)[apo_na(L)], int lev, double* red,
                                                    double* partial) {
  constexpr int NA = apo_na(L), N = apo_n(L), B = 1 + L + ntri(L);
  block_sum<NA>(v, red);
  if (threadIdx.x == 0) {
    double* out = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * N;
#pragma unroll
    for (int q = 0; q < B; ++q) out[q] = v[q];
#pragma unroll
    for (int c = 0; c < L; ++c)
#pragma unroll
      for (int q = 0; q < 4; ++q) out[B + 4 * c + q] = c == lev ? v[B + q] : 0.0;
  }
}

// A workgroup that owns no row of its segment (the grid is sized for the largest one) writes
// its all-zero partial and leaves before any staging: the zeros block_sum would have given it.
// Block-uniform, so the whole workgroup returns together. True when it left.
template <int L>
__device__ __forceinline__ bool idle_partial(const Seg& sg, int64_t rows_per_block,
                                             double* __restrict__ partial) {
  constexpr int N = apo_n(L);
  static_assert(N <= 256, "one thread per moment");
  if (sg.r0 + (int64_t)blockIdx.x * rows_per_block < sg.r1) return false;
  if (threadIdx.x < N)
    partial[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * N + threadIdx.x] = 0.0;
  return true;
}

// stage g_0..g_{L-1} of block k and m_lev, interleaved per column, and the column list;
// returns the size of the compacted union
template <int L, typename C>
__device__ __forceinline__ int stage_levels(C* cv, int* xc, const int* __restrict__ xcols, int p,
                                            int P, const double* __restrict__ coef, int k, int lev,
                                            int* wcnt) {
  constexpr int NV = L + 1;
  for (int j = threadIdx.x; j < p; j += blockDim.x) {
    xc[j] = xcols[j];
    ATE_DASSERT(xc[j] >= 0 && (P == 0 || xc[j] < P));
  }
  for (int j = threadIdx.x; j <= p; j += blockDim.x) {
#pragma unroll
    for (int r = 0; r < L; ++r)
      cv[(int64_t)j * NV + r] = (C)coef[((int64_t)k * 2 * L + r) * (p + 1) + j];
    cv[(int64_t)j * NV + L] = (C)coef[((int64_t)k * 2 * L + L + lev) * (p + 1) + j];
  }
  __syncthreads();
  return compact_support_n<NV>(cv, xc, p, wcnt);
}

// fp32 / fp64 column-major panels: fp64 dot products, RPT rows per thread 256 apart (at
// RPT = 4 the row ownership of irm_score_kernel). partial: [nseg * nbx][N(L)].
template <typename T, int L>
__global__ __launch_bounds__(256) void apo_score_kernel(
    const T* __restrict__ X, int64_t ld, const int* __restrict__ xcols, int p, int P,
    const Seg* __restrict__ segs, int nseg, const double* __restrict__ coef /*[nseg/L][2L][p+1]*/,
    int y0, int y1, int d0, int d1, int vcol, double clip, double* __restrict__ partial) {
  constexpr int NV = L + 1, NA = apo_na(L), RPT = apo_rpt(L);
  extern __shared__ __attribute__((aligned(16))) double sh[];
  double* cv = sh;                                // [p+1][L+1]
  int* xc = (int*)(sh + (int64_t)NV * (p + 1));   // [p]
  __shared__ double red[16 * NA];
  __shared__ int wcnt[16];
  const int s = blockIdx.y, k = s / L, lev = s % L;
  ATE_DASSERT(s < nseg && nseg % L == 0 && k < nseg / L && y0 >= 0 && d0 >= 0 && vcol >= 0);
  ATE_DASSERT(P == 0 || (y0 < P && d0 < P && vcol < P && y1 < P && d1 < P));
  const Seg sg = segs[s];
  ATE_DASSERT(sg.r0 >= 0 && sg.r0 <= sg.r1 && sg.r1 <= ld);
  if (idle_partial<L>(sg, 256 * RPT, partial)) return;
  p = stage_levels<L>(cv, xc, xcols, p, P, coef, k, lev, wcnt);
  double v[NA] = {};
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
      ATE_DASSERT(d == (double)lev);
      double g[L];
#pragma unroll
      for (int q = 0; q < L; ++q) g[q] = a[q][r];
      apo_accumulate<L>(v, y, d, lev, g, a[L][r], clip);
    }
  }
  write_level_partial<L>(v, lev, red, partial);
}

// bf16 panels (column-major and 64-row blocked): each thread owns 8 CONSECUTIVE rows, so
// every column read is one 16-byte load through (cs, bs); dot products in fp32 (bf16 values
// are exact in fp32; coefficients rounded to fp32), the score in fp64 (the row ownership and
// arithmetic of irm_score_bf16_kernel).
template <int L>
__global__ __launch_bounds__(256) void apo_score_bf16_kernel(
    const bf16_t* __restrict__ X, int64_t cs, int64_t bs, const int* __restrict__ xcols, int p,
    int P, int64_t ld, const Seg* __restrict__ segs, int nseg, const double* __restrict__ coef,
    int y0, int y1, int d0, int d1, int vcol, double clip, double* __restrict__ partial) {
  constexpr int NV = L + 1, NA = apo_na(L), UNROLL = L >= 6 ? 1 : 2;
  extern __shared__ __attribute__((aligned(16))) float shf[];
  float* cv = shf;                                 // [p+1][L+1]
  int* xc = (int*)(shf + (int64_t)NV * (p + 1));   // [p]
  __shared__ double red[16 * NA];
  __shared__ int wcnt[16];
  const int s = blockIdx.y, k = s / L, lev = s % L;
  ATE_DASSERT(s < nseg && nseg % L == 0 && k < nseg / L && y0 >= 0 && d0 >= 0 && vcol >= 0);
  ATE_DASSERT(P == 0 || (y0 < P && d0 < P && vcol < P && y1 < P && d1 < P));
  const Seg sg = segs[s];
  ATE_DASSERT(sg.r0 >= 0 && sg.r0 <= sg.r1 && (ld == 0 || sg.r1 <= ld) && (sg.r0 & 7) == 0 &&
              (sg.r1 & 7) == 0);
  if (idle_partial<L>(sg, 256 * 8, partial)) return;
  p = stage_levels<L>(cv, xc, xcols, p, P, coef, k, lev, wcnt);
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
  double v[NA] = {};
  for (int64_t i = sg.r0 + ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8; i < sg.r1;
       i += (int64_t)gridDim.x * 256 * 8) {
    float a[NV][8];
#pragma unroll
    for (int q = 0; q < NV; ++q)
#pragma unroll
      for (int r = 0; r < 8; ++r) a[q][r] = cv[q];
    // two columns in flight while the accumulators leave registers for them (L <= 5)
#pragma unroll UNROLL
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
    float vv[8], ya[8], yb[8], da[8], db[8];
    ld8(vcol, i, vv);
    ld8_pair(y0, y1, i, ya, yb);
    ld8_pair(d0, d1, i, da, db);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      if (vv[r] == 0.f) continue;                                 // padding row
      const double y = (double)ya[r] + (double)yb[r];
      const double d = (double)da[r] + (double)db[r];
      ATE_DASSERT(d == (double)lev);
      double g[L];
#pragma unroll
      for (int q = 0; q < L; ++q) g[q] = (double)a[q][r];
      apo_accumulate<L>(v, y, d, lev, g, (double)a[L][r], clip);
    }
  }
  write_level_partial<L>(v, lev, red, partial);
}

// irm_sum_kernel<N> (irm_common.hpp) over SUM_CH moments per workgroup: moment q is summed by
// workgroup q / SUM_CH with, per moment, the operations of irm_sum_kernel -- thread i adds
// partials i, i + 256, ... in order, then the fixed-shape block reduction -- so a moment has
// the bits irm_sum_kernel<N> gives it. One workgroup holding all 64 or 77 sums per thread
// spills to scratch; 16 per workgroup do not, at any L.
constexpr int SUM_CH = 16;
template <int N>
__global__ __launch_bounds__(256) void apo_sum_kernel(const double* __restrict__ partial, int nb,
                                                      double* __restrict__ out) {
  __shared__ double red[16 * SUM_CH];
  const int q0 = blockIdx.x * SUM_CH;
  ATE_DASSERT(q0 < N);
  double v[SUM_CH] = {};
  for (int b = threadIdx.x; b < nb; b += 256)
#pragma unroll
    for (int q = 0; q < SUM_CH; ++q)
      if (q0 + q < N) v[q] += partial[(int64_t)b * N + q0 + q];
  block_sum<SUM_CH>(v, red);
  if (threadIdx.x == 0)
#pragma unroll
    for (int q = 0; q < SUM_CH; ++q)
      if (q0 + q < N) out[q0 + q] = v[q];
}

struct ApoArgs {
  int dtype;
  const void* X;
  int64_t cs, bs;
  const void* xcols;
  int p;
  const void* segs;
  int nseg;
  const void* coef;
  int y0, y1, d0, d1, vcol;
  double clip;
  int nbx;
  void* partial;
  void* moments;
  hipStream_t s;
};

// the pass at one L: the LDS bound, the score launch of the panel's type and the fixed-order sum
template <int L>
int apo_pass(const ApoArgs& a) {
  constexpr int N = apo_n(L);
  // what the strides say about the panel's extent, for the debug build's bounds checks
  // (0 = unknown): column-major (bs = 64) has ld = cs rows; 64-row blocked has P = bs / 64
  const int64_t ld = a.bs == 64 ? a.cs : 0;
  const int P = a.bs == 64 ? 0 : (int)(a.bs / 64);
  const size_t esz = a.dtype == 3 ? sizeof(float) : sizeof(double);
  const size_t sh = (size_t)(L + 1) * (a.p + 1) * esz + (size_t)a.p * sizeof(int);
  if (sh + (size_t)apo_static_lds(L) > 64 * 1024) return -1;
  const dim3 grid(a.nbx, a.nseg), block(256);
  if (a.dtype == 1)
    ATE_LAUNCH((apo_score_kernel<float, L>), grid, block, sh, a.s, (const float*)a.X, a.cs,
               (const int*)a.xcols, a.p, P, (const Seg*)a.segs, a.nseg, (const double*)a.coef,
               a.y0, a.y1, a.d0, a.d1, a.vcol, a.clip, (double*)a.partial);
  else if (a.dtype == 2)
    ATE_LAUNCH((apo_score_kernel<double, L>), grid, block, sh, a.s, (const double*)a.X, a.cs,
               (const int*)a.xcols, a.p, P, (const Seg*)a.segs, a.nseg, (const double*)a.coef,
               a.y0, a.y1, a.d0, a.d1, a.vcol, a.clip, (double*)a.partial);
  else
    ATE_LAUNCH(apo_score_bf16_kernel<L>, grid, block, sh, a.s, (const bf16_t*)a.X, a.cs, a.bs,
               (const int*)a.xcols, a.p, P, ld, (const Seg*)a.segs, a.nseg, (const double*)a.coef,
               a.y0, a.y1, a.d0, a.d1, a.vcol, a.clip, (double*)a.partial);
  ATE_CHECK_LAUNCH();
  ATE_LAUNCH(apo_sum_kernel<N>, dim3((N + SUM_CH - 1) / SUM_CH), dim3(256), 0, a.s,
             (const double*)a.partial, a.nbx * a.nseg, (double*)a.moments);
  ATE_CHECK_LAUNCH();
  return 0;
}

constexpr int apo_dyn_max(int L) { return 64 * 1024 - apo_static_lds(L); }

}  // namespace

// the largest launch of each instantiation, for the debug build's load-time resource check
ATE_KERNEL_SHAPE("apo_score<float,2>", 256, apo_dyn_max(2), apo_score_kernel<float, 2>)
ATE_KERNEL_SHAPE("apo_score<float,3>", 256, apo_dyn_max(3), apo_score_kernel<float, 3>)
ATE_KERNEL_SHAPE("apo_score<float,4>", 256, apo_dyn_max(4), apo_score_kernel<float, 4>)
ATE_KERNEL_SHAPE("apo_score<float,5>", 256, apo_dyn_max(5), apo_score_kernel<float, 5>)
ATE_KERNEL_SHAPE("apo_score<float,6>", 256, apo_dyn_max(6), apo_score_kernel<float, 6>)
ATE_KERNEL_SHAPE("apo_score<float,7>", 256, apo_dyn_max(7), apo_score_kernel<float, 7>)
ATE_KERNEL_SHAPE("apo_score<float,8>", 256, apo_dyn_max(8), apo_score_kernel<float, 8>)
ATE_KERNEL_SHAPE("apo_score<double,2>", 256, apo_dyn_max(2), apo_score_kernel<double, 2>)
ATE_KERNEL_SHAPE("apo_score<double,3>", 256, apo_dyn_max(3), apo_score_kernel<double, 3>)
ATE_KERNEL_SHAPE("apo_score<double,4>", 256, apo_dyn_max(4), apo_score_kernel<double, 4>)
ATE_KERNEL_SHAPE("apo_score<double,5>", 256, apo_dyn_max(5), apo_score_kernel<double, 5>)
ATE_KERNEL_SHAPE("apo_score<double,6>", 256, apo_dyn_max(6), apo_score_kernel<double, 6>)
ATE_KERNEL_SHAPE("apo_score<double,7>", 256, apo_dyn_max(7), apo_score_kernel<double, 7>)
ATE_KERNEL_SHAPE("apo_score<double,8>", 256, apo_dyn_max(8), apo_score_kernel<double, 8>)
ATE_KERNEL_SHAPE("apo_score_bf16<2>", 256, apo_dyn_max(2), apo_score_bf16_kernel<2>)
ATE_KERNEL_SHAPE("apo_score_bf16<3>", 256, apo_dyn_max(3), apo_score_bf16_kernel<3>)
ATE_KERNEL_SHAPE("apo_score_bf16<4>", 256, apo_dyn_max(4), apo_score_bf16_kernel<4>)
ATE_KERNEL_SHAPE("apo_score_bf16<5>", 256, apo_dyn_max(5), apo_score_bf16_kernel<5>)
ATE_KERNEL_SHAPE("apo_score_bf16<6>", 256, apo_dyn_max(6), apo_score_bf16_kernel<6>)
ATE_KERNEL_SHAPE("apo_score_bf16<7>", 256, apo_dyn_max(7), apo_score_bf16_kernel<7>)
ATE_KERNEL_SHAPE("apo_score_bf16<8>", 256, apo_dyn_max(8), apo_score_bf16_kernel<8>)
ATE_KERNEL_SHAPE("apo_sum_kernel<14>", 256, 0, apo_sum_kernel<apo_n(2)>)
ATE_KERNEL_SHAPE("apo_sum_kernel<22>", 256, 0, apo_sum_kernel<apo_n(3)>)
ATE_KERNEL_SHAPE("apo_sum_kernel<31>", 256, 0, apo_sum_kernel<apo_n(4)>)
ATE_KERNEL_SHAPE("apo_sum_kernel<41>", 256, 0, apo_sum_kernel<apo_n(5)>)
ATE_KERNEL_SHAPE("apo_sum_kernel<52>", 256, 0, apo_sum_kernel<apo_n(6)>)
ATE_KERNEL_SHAPE("apo_sum_kernel<64>", 256, 0, apo_sum_kernel<apo_n(7)>)
ATE_KERNEL_SHAPE("apo_sum_kernel<77>", 256, 0, apo_sum_kernel<apo_n(8)>)

// The potential-outcome pass. dtype 1 f32, 2 f64, 3 bf16. (cs, bs): element (c, i) at c*cs +
// (i/64)*bs + i%64 (fp32 / fp64 panels: column-major only, bs = 64). segs [nseg][2] int64
// padded row ranges, segment L k + c = fold k, level c; coef [nseg / L][2L][p+1] fp64, rows
// g_0..g_{L-1}, m_0..m_{L-1}, intercept first; (y0, y1), (d0, d1): the columns of Y and of the
// level D (second = -1 unless the target is stored as a hi + lo bf16 pair). Rejected with -1,
// nothing launched: L outside 2..8, nseg not a multiple of L, a missing target column, clip
// outside [0, 0.5), or dynamic LDS (L+1)(p+1) esz + 4 p plus the static 128 NA(L) + 64 bytes
// over 64 KB. partial: [nseg*nbx][N(L)]; moments: [N(L)].
ATE_API int ate_apo_moments(int dtype, const void* X, int64_t cs, int64_t bs, const void* xcols,
                            int p, const void* segs, int nseg, int levels, const void* coef,
                            int y0, int y1, int d0, int d1, int vcol, double clip, int nbx,
                            void* partial, void* moments, void* stream) {
  if (dtype < 1 || dtype > 3 || (dtype != 3 && bs != 64)) return -1;
  if (levels < 2 || levels > APO_LMAX) return -1;
  if (p < 0 || nseg < 1 || nseg > 65535 || nseg % levels != 0 || nbx < 1 || cs < 64 || bs < 64)
    return -1;
  if (y0 < 0 || d0 < 0 || vcol < 0) return -1;
  if (!(clip >= 0.0 && clip < 0.5)) return -1;
  const ApoArgs a{dtype, X, cs, bs, xcols, p, segs, nseg, coef, y0, y1, d0, d1, vcol, clip, nbx,
                  partial, moments, (hipStream_t)stream};
  switch (levels) {
    case 2: return apo_pass<2>(a);
    case 3: return apo_pass<3>(a);
    case 4: return apo_pass<4>(a);
    case 5: return apo_pass<5>(a);
    case 6: return apo_pass<6>(a);
    case 7: return apo_pass<7>(a);
    default: return apo_pass<8>(a);
  }
}
