// Cluster-robust variance: the deterministic segmented reduction behind ate_dml(clusters=)
// and ate_dml_irm(clusters=).
//
// Every score is psi_i = a_i - theta b_i. With the rows of cluster j listed in
// order[starts[j] .. starts[j+1]) (a CSR over panel rows), the pass forms per cluster
//   A_j = sum a, B_j = sum b (b null: B_j = n_j), t_j = A_j - theta B_j
// and returns out[4] = { sum_j t_j^2, sum_j t_j, sum_j n_j^2, max_j n_j } in fp64.
//
// The cost must not depend on the size distribution, and the launch geometry must not
// depend on the cluster contents (the launches are captured in a hipGraph whose replays
// carry new clusters). So the work is cut by POSITION, not by cluster: workgroup T owns the
// CHUNK positions [T CHUNK, (T+1) CHUNK) of `order`, gathers their values into LDS once
// (coalesced index reads; run-structured orders gather whole lines), and finds the clusters
// that overlap its chunk by a wave-wide 64-ary search of `starts`. Within the chunk
//   * a piece of at most SMALL rows is summed by one lane (many tiny clusters: 256 per step),
//   * a longer piece is summed by the wave that owns it, 64 rows per step,
//   * a cluster cut by the chunk's edge leaves its piece (A, B) as one of the chunk's two
//     open pieces; a cluster longer than CHUNK is therefore split into CHUNK-sized pieces.
// A second, single-workgroup launch adds the chunks' partial moments in a fixed order and
// joins the open pieces in chunk order (each carries its row count: no second look at starts).
// No floating-point atomics anywhere: the same inputs give the same bits at a given geometry,
// whoever runs first.
//
// Memory safety does not depend on the contents of starts / order: rows outside [0, ld)
// read as 0, piece bounds are clamped to the chunk, and the search stays inside starts[0..J].
#include "common.hpp"

using namespace ate;

namespace {

constexpr int CL_THREADS = 256;
constexpr int CL_CHUNK = 2048;   // positions per workgroup (8 per thread)
constexpr int CL_SMALL = 32;     // pieces up to this many rows: one lane
constexpr int CL_WORK = 10;      // doubles per chunk: 4 moments, 2 x (A, B), 2 + 2 int32 (keys, rows)

// first q in [0, J] with starts[q] > x, J + 1 when there is none: a 64-ary search by the
// whole wave (every lane probes, one ballot per level: 4 levels at J = 1e7). All 64 lanes
// must call it; terminates on any contents (the range shrinks every level).
__device__ __forceinline__ int wave_upper(const int* __restrict__ starts, int J, int64_t x) {
  const int lane = threadIdx.x & 63;
  int64_t lo = 0, hi = (int64_t)J + 1;          // the answer lies in [lo, hi]
  while (lo < hi) {
    const int64_t stride = (hi - lo + 63) >> 6;
    const int64_t q = lo + lane * stride;
    ATE_DASSERT(q >= 0);
    const bool above = q >= hi || (int64_t)starts[q] > x;
    const uint64_t m = __ballot(above);
    const int first = m ? __ffsll((unsigned long long)m) - 1 : 64;
    if (first == 0) return (int)lo;
    const int64_t nhi = lo + first * stride;
    lo = lo + (first - 1) * stride + 1;
    hi = nhi < hi ? nhi : hi;
  }
  return (int)lo;
}

struct Moments {
  double s[3] = {0, 0, 0};   // sum t^2, sum t, sum n_j^2
  double nmax = 0;
  __device__ __forceinline__ void finish(double A, double B, double theta, double cnt) {
    const double t = A - theta * B;
    s[0] += t * t;
    s[1] += t;
    s[2] += cnt * cnt;
    nmax = cnt > nmax ? cnt : nmax;
  }
};

// block-wide fixed-shape reduction of the moments; the result is valid in thread 0
__device__ __forceinline__ void block_moments(Moments& m, double* red /*[16*3]*/,
                                              double* redm /*[16]*/) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  m.nmax = wave_max(m.nmax);
  if (lane == 0) redm[wid] = m.nmax;
  block_sum<3>(m.s, red);                       // syncs: redm is visible after it
  if (threadIdx.x == 0)
    for (int w = 0; w < nw; ++w) m.nmax = redm[w] > m.nmax ? redm[w] : m.nmax;
}

template <bool HASB>
__global__ __launch_bounds__(CL_THREADS) void cluster_chunk_kernel(
    const double* __restrict__ a, const double* __restrict__ b, int64_t ld,
    const int* __restrict__ starts, const int* __restrict__ order, int64_t n, int J,
    const double* __restrict__ theta, double* __restrict__ work /* [4 nt | 2 nt A | 2 nt B |
    2 nt int32 keys | 2 nt int32 rows] */) {
  __shared__ double va[CL_CHUNK];
  __shared__ double vb[HASB ? CL_CHUNK : 1];
  __shared__ double red[16 * 3], redm[16];
  __shared__ double open_ab[4];
  __shared__ int open_key[2], open_len[2];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t c0 = (int64_t)blockIdx.x * CL_CHUNK;
  const int64_t c1 = c0 + CL_CHUNK < n ? c0 + CL_CHUNK : n;
  if (threadIdx.x < 2) open_key[threadIdx.x] = -1;
#pragma unroll
  for (int r = 0; r < CL_CHUNK / CL_THREADS; ++r) {
    const int q = r * CL_THREADS + threadIdx.x;
    const int64_t i = c0 + q;
    double x = 0.0, y = 0.0;
    if (i < c1) {
      const int64_t row = order[i];
      if (row >= 0 && row < ld) {
        x = a[row];
        if (HASB) y = b[row];
      }
    }
    va[q] = x;
    if (HASB) vb[q] = y;
  }
  // the clusters that overlap [c0, c1): jlo = the last one starting at or before c0,
  // jhi = the last one starting before c1
  int64_t jlo = 0, jhi = -1;
  if (c0 < c1) {
    jlo = (int64_t)wave_upper(starts, J, c0) - 1;
    jhi = (int64_t)wave_upper(starts, J, c1 - 1) - 1;
    jlo = jlo < 0 ? 0 : jlo;
    jhi = jhi > (int64_t)J - 1 ? (int64_t)J - 1 : jhi;
  }
  __syncthreads();
  const double th = *theta;
  Moments mom;
  const int64_t nc = jhi - jlo + 1;
  // cluster c of the chunk goes to wave c % 4, lane (c / 4) % 64: neighbouring long pieces
  // land on different waves
  for (int64_t base = 0; base < nc; base += CL_THREADS) {
    const int64_t c = base + lane * 4 + wid;
    const bool live = c < nc;
    const int64_t j = jlo + c;
    const int64_t s0 = live ? (int64_t)starts[j] : 0, e0 = live ? (int64_t)starts[j + 1] : 0;
    const int64_t s = s0 > c0 ? s0 : c0, e = e0 < c1 ? e0 : c1;
    const int len = live && e > s ? (int)(e - s) : 0;
    const int off = len > 0 ? (int)(s - c0) : 0;
    ATE_DASSERT(off >= 0 && off + len <= CL_CHUNK);
    const bool big = len > CL_SMALL;
    double A = 0.0, B = 0.0;
    if (!big) {
      for (int q = 0; q < len; ++q) {
        A += va[off + q];
        if (HASB) B += vb[off + q];
      }
      if (!HASB) B = (double)len;
    }
    uint64_t m = __ballot(big);
    while (m) {
      const int src = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      const int o = __shfl(off, src, 64), l = __shfl(len, src, 64);
      double x = 0.0, y = 0.0;
      for (int q = lane; q < l; q += 64) {
        x += va[o + q];
        if (HASB) y += vb[o + q];
      }
      x = wave_sum(x);
      if (HASB) y = wave_sum(y);
      if (lane == src) {
        A = x;
        B = HASB ? y : (double)l;
      }
    }
    if (!live) continue;
    if (s0 >= c0 && e0 <= c1) {
      mom.finish(A, B, th, e0 > s0 ? (double)(e0 - s0) : 0.0);
    } else if (len > 0) {
      const int slot = s0 < c0 ? 0 : 1;         // cut on the left | only on the right
      open_ab[2 * slot] = A;
      open_ab[2 * slot + 1] = B;
      open_key[slot] = (int)j;
      open_len[slot] = len;
    }
  }
  block_moments(mom, red, redm);                // syncs: the open pieces are visible after it
  if (threadIdx.x == 0) {
    const int64_t nt = gridDim.x, T = blockIdx.x;
    double* w = work + 4 * T;
    w[0] = mom.s[0]; w[1] = mom.s[1]; w[2] = mom.s[2]; w[3] = mom.nmax;
    int* pk = reinterpret_cast<int*>(work + 8 * nt);
    int* pl = reinterpret_cast<int*>(work + 9 * nt);
    for (int q = 0; q < 2; ++q) {
      work[4 * nt + 2 * T + q] = open_ab[2 * q];
      work[6 * nt + 2 * T + q] = open_ab[2 * q + 1];
      pk[2 * T + q] = open_key[q];
      pl[2 * T + q] = open_key[q] >= 0 ? open_len[q] : 0;
    }
  }
}

// A run of pieces of one cluster: its key and the sums of a, b and rows so far.
struct Run { int key; double A, B, L; };

// Folds pieces that arrive in order: equal neighbouring keys join; a cluster that begins and
// ends strictly inside the sequence is finished, the first and the last run stay open for
// the level above (they may continue in the neighbouring sequences).
struct Fold {
  Run first{-1, 0, 0, 0}, cur{-1, 0, 0, 0};
  int nrun = 0;
  __device__ __forceinline__ void push(const Run& r, Moments& m, double th) {
    if (r.key < 0) return;
    if (r.key == cur.key) { cur.A += r.A; cur.B += r.B; cur.L += r.L; return; }
    if (cur.key >= 0) {
      if (nrun == 0) first = cur; else m.finish(cur.A, cur.B, th, cur.L);
      ++nrun;
    }
    cur = r;
  }
  __device__ __forceinline__ void ends(Run& f, Run& l) const {
    f = nrun == 0 ? cur : first;
    l = nrun == 0 ? Run{-1, 0, 0, 0} : cur;
  }
};

constexpr int CL_JOIN = 1024;    // threads of the joining workgroup

// One workgroup: the chunks' moments in a fixed order (thread i: chunks i, i + 1024, ...), and
// the open pieces joined in chunk order, in three levels: the 2 nt pieces are cut into 1024
// consecutive spans, one per thread; lane 0 of each wave folds its wave's 128 open runs;
// thread 0 folds the 32 that remain. A cluster is finished at the level where it begins and
// ends strictly inside a sequence; a piece carries its row count, so nothing but `work` is read.
__global__ __launch_bounds__(CL_JOIN) void cluster_join_kernel(
    const double* __restrict__ work, int64_t nt, const double* __restrict__ theta,
    double* __restrict__ out) {
  __shared__ double red[16 * 3], redm[16];
  __shared__ double eA[2 * CL_JOIN], eB[2 * CL_JOIN], eL[2 * CL_JOIN];
  __shared__ int eK[2 * CL_JOIN];
  __shared__ double gA[32], gB[32], gL[32];
  __shared__ int gK[32];
  const double th = *theta;
  const double* pA = work + 4 * nt;
  const double* pB = work + 6 * nt;
  const int* pK = reinterpret_cast<const int*>(work + 8 * nt);
  const int* pL = reinterpret_cast<const int*>(work + 9 * nt);
  Moments mom;
  for (int64_t t = threadIdx.x; t < nt; t += CL_JOIN) {
    const double* w = work + 4 * t;
    mom.s[0] += w[0];
    mom.s[1] += w[1];
    mom.s[2] += w[2];
    mom.nmax = w[3] > mom.nmax ? w[3] : mom.nmax;
  }
  const int64_t np = 2 * nt, per = (np + CL_JOIN - 1) / CL_JOIN;
  const int64_t p0 = threadIdx.x * per, p1 = p0 + per < np ? p0 + per : np;
  Run f, l;
  {
    Fold fold;
    for (int64_t q = p0; q < p1; ++q)
      fold.push(Run{pK[q], pA[q], pB[q], (double)pL[q]}, mom, th);
    fold.ends(f, l);
  }
  eK[2 * threadIdx.x] = f.key; eA[2 * threadIdx.x] = f.A; eB[2 * threadIdx.x] = f.B;
  eL[2 * threadIdx.x] = f.L;
  eK[2 * threadIdx.x + 1] = l.key; eA[2 * threadIdx.x + 1] = l.A; eB[2 * threadIdx.x + 1] = l.B;
  eL[2 * threadIdx.x + 1] = l.L;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    const int wid = threadIdx.x >> 6;
    Fold fold;
    for (int q = 128 * wid; q < 128 * wid + 128; ++q)
      fold.push(Run{eK[q], eA[q], eB[q], eL[q]}, mom, th);
    fold.ends(f, l);
    gK[2 * wid] = f.key; gA[2 * wid] = f.A; gB[2 * wid] = f.B; gL[2 * wid] = f.L;
    gK[2 * wid + 1] = l.key; gA[2 * wid + 1] = l.A; gB[2 * wid + 1] = l.B; gL[2 * wid + 1] = l.L;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Fold fold;
    for (int q = 0; q < 32; ++q) fold.push(Run{gK[q], gA[q], gB[q], gL[q]}, mom, th);
    fold.ends(f, l);
    if (f.key >= 0) mom.finish(f.A, f.B, th, f.L);
    if (l.key >= 0) mom.finish(l.A, l.B, th, l.L);
  }
  block_moments(mom, red, redm);
  if (threadIdx.x == 0) {
    out[0] = mom.s[0]; out[1] = mom.s[1]; out[2] = mom.s[2]; out[3] = mom.nmax;
  }
}

}  // namespace

ATE_KERNEL_SHAPE("cluster_chunk_kernel<b>", CL_THREADS, 0, cluster_chunk_kernel<true>)
ATE_KERNEL_SHAPE("cluster_chunk_kernel<1>", CL_THREADS, 0, cluster_chunk_kernel<false>)
ATE_KERNEL_SHAPE("cluster_join_kernel", CL_JOIN, 0, cluster_join_kernel)

// The positions one workgroup owns; a cluster longer than this is split into pieces.
ATE_API int ate_cluster_chunk() { return CL_CHUNK; }

// fp64 entries of the workspace of ate_cluster_moments for n positions
ATE_API int64_t ate_cluster_work(int64_t n) {
  if (n < 0) return -1;
  const int64_t nt = (n + CL_CHUNK - 1) / CL_CHUNK;
  return (nt < 1 ? 1 : nt) * CL_WORK;
}

// a [ld] fp64, b [ld] fp64 or null (b == 1), starts [J + 1] int32 (positions of `order`),
// order [n] int32 (rows of a / b), theta [1] fp64 on the device (written earlier on the
// stream), work [ate_cluster_work(n)] fp64, out [4] fp64. The launch geometry depends on n
// alone. Returns -1 (no launch) for J < 1, ld < 0, n < 0, n or ld at or above 2^31, or a
// null pointer other than b.
ATE_API int ate_cluster_moments(const void* a, const void* b, int64_t ld, const void* starts,
                                const void* order, int64_t n, int J, const void* theta,
                                void* work, void* out, void* stream) {
  if (J < 1 || ld < 0 || n < 0 || n >= (int64_t)1 << 31 || ld >= (int64_t)1 << 31) return -1;
  if (!a || !starts || !order || !theta || !work || !out) return -1;
  hipStream_t s = (hipStream_t)stream;
  int64_t nt = (n + CL_CHUNK - 1) / CL_CHUNK;
  nt = nt < 1 ? 1 : nt;
  if (b)
    ATE_LAUNCH(cluster_chunk_kernel<true>, dim3((unsigned)nt), dim3(CL_THREADS), 0, s,
               (const double*)a, (const double*)b, ld, (const int*)starts, (const int*)order, n,
               J, (const double*)theta, (double*)work);
  else
    ATE_LAUNCH(cluster_chunk_kernel<false>, dim3((unsigned)nt), dim3(CL_THREADS), 0, s,
               (const double*)a, (const double*)nullptr, ld, (const int*)starts,
               (const int*)order, n, J, (const double*)theta, (double*)work);
  ATE_CHECK_LAUNCH();
  ATE_LAUNCH(cluster_join_kernel, dim3(1), dim3(CL_JOIN), 0, s, (const double*)work, nt,
             (const double*)theta, (double*)out);
  ATE_CHECK_LAUNCH();
  return 0;
}
