// Exact depth-2 policy trees on per-row scores (policy learning on the AIPW scores of
// DML-IRM; estimators/policy.py; Athey & Wager 2021, Zhou, Athey & Wager 2023).
//
// Rows carry a score psi, a code use (-1 skip, 0 training row, 1 held-out row) and d <= 32
// features binned to uint8 codes < nb[j] <= 64 (feature-major [d][ld]). With
// q = rint((psi - cost) 2^e) as int64 (0 when not finite; e read from device memory) every
// sum that decides the tree is an integer, so every launch geometry, the numpy twin and every
// world size pick the same tree bit for bit.
//
// ate_policy_pair_hist: for every feature pair j1 <= j2 (diagonal included) a 64 x 64 tile of
// (S q, row count) over the training rows, cell [code_j1][code_j2]:
// out [d (d + 1) / 2][2][64][64] int64, pair (a, b) at a d - a (a - 1) / 2 + (b - a).
// A workgroup owns one j1 and up to JT consecutive j2 (blockIdx.y) and every nbx-th chunk of
// 512 x 4 rows (blockIdx.x; four rows per thread, read as 32-bit words of use and codes; one
// row per thread when ld is no multiple of 4): psi, use and codes[j1] are read once per row
// for the JT tiles, which are accumulated in LDS with integer atomics (int64 sums, int32
// counts: 48 KB a tile, 144 KB of the 160 KB) and flushed with global int64 atomics into the
// zeroed output -- integer adds commute, so the output has the same bits for every nbx.
// Small tiles: with nb1 nb2 <= 64 (a binary x binary tile has 4 live cells) the 64 lanes of a
// wave would queue on the same few LDS addresses. Such a tile keeps one copy of its cells per
// lane instead, slot cell * 64 + lane (the lanes of a wave never meet, consecutive lanes are
// consecutive addresses), and the 64 copies are summed by a wave reduction at the flush.
// priv = 0 selects the plain path for every tile (A/B comparison).
//
// ate_policy_search: three plain launches, no host sync.
//  1. policy_prefix_kernel  2-D inclusive prefix sums of every tile plane: P[ta][tb] = the sum
//     over the rows with code_a <= ta and code_b <= tb (cells past nb are 0, so index 63
//     reads a margin).
//  2. policy_child_kernel   for every root split (j1, t1) and side, the best depth-1 subtree:
//     leaf first, then every (j2, t2) in ascending order, a later candidate replacing the
//     incumbent only if strictly better; tiles with j2 < j1 are read transposed.
//  3. policy_pick_kernel    the best root under the same rule, and the tree record
//     rec[16] int64: (j, t) of the root, the left and the right child (-1, -1 for a leaf), the
//     four leaf actions (LL, LR, RL, RR; a leaf node repeats its action), the total value in
//     q units, the training-row count.
// A split (j, t), 0 <= t <= nb[j] - 2, sends codes <= t left; both sides must hold at least
// min_leaf training rows. A leaf with sum S has value max(S, 0) and treats iff S > 0.
#include "common.hpp"

using namespace ate;

namespace {

constexpr int NBMAX = 64;            // bins per feature (at most)
constexpr int TILE = NBMAX * NBMAX;  // cells of a tile
constexpr int DMAX = 32;             // features (at most)
constexpr int JT = 3;                // tiles per workgroup
constexpr int HT = 512;              // threads per workgroup of the histogram pass
constexpr int ST = 256;              // threads per workgroup of the search kernels
constexpr int REC = 16;              // entries of the tree record

__host__ __device__ inline int pair_index(int d, int a, int b) {   // a <= b
  return a * d - a * (a - 1) / 2 + (b - a);
}
inline int hist_groups(int d) {
  int g = 0;
  for (int j = 0; j < d; ++j) g += (d - j + JT - 1) / JT;
  return g;
}
__device__ __forceinline__ int clamp_nb(int v) { return v < 1 ? 1 : (v > NBMAX ? NBMAX : v); }

// V rows per thread and step: 4 when ld is a multiple of 4 (use and the codes are then read
// as aligned 32-bit words, and the loads of four rows are in flight together), else 1
template <int V>
__global__ __launch_bounds__(HT) void policy_pair_hist_kernel(
    const double* __restrict__ psi, const double* __restrict__ cost, const int* __restrict__ ep,
    const int8_t* __restrict__ use, const uint8_t* __restrict__ codes,
    const int* __restrict__ nb, int64_t ld, int d, int priv,
    unsigned long long* __restrict__ out) {
  __shared__ unsigned long long ss[JT][TILE];   // S q (two's complement)
  __shared__ int sc[JT][TILE];                  // rows
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  // blockIdx.y -> (j1, first j2)
  int g = blockIdx.y, j1 = 0;
  for (; j1 < d; ++j1) {
    const int ng = (d - j1 + JT - 1) / JT;
    if (g < ng) break;
    g -= ng;
  }
  ATE_DASSERT(j1 < d);
  if (j1 >= d) return;
  const int j2a = j1 + g * JT;
  const int nt = (d - j2a) < JT ? (d - j2a) : JT;
  ATE_DASSERT(nt >= 1 && j2a + nt <= d);
  const int nb1 = clamp_nb(nb[j1]);
  int nb2[JT];
  bool small[JT];
#pragma unroll
  for (int k = 0; k < JT; ++k) {
    nb2[k] = k < nt ? clamp_nb(nb[j2a + k]) : 1;
    small[k] = priv != 0 && nb1 * nb2[k] <= 64;
  }
  for (int c = t; c < JT * TILE; c += HT) {
    (&ss[0][0])[c] = 0ull;
    (&sc[0][0])[c] = 0;
  }
  __syncthreads();
  const double cst = cost[0];
  const int e = ep[0];
  const uint8_t* c1p = codes + (int64_t)j1 * ld;
  ATE_DASSERT(V == 1 || ld % V == 0);
  for (int64_t i = ((int64_t)blockIdx.x * HT + t) * V; i < ld; i += (int64_t)gridDim.x * HT * V) {
    // V == 4: i is a multiple of 4 and i + 3 < ld; every row pointer is 4-byte aligned
    uint32_t uw, c1w, c2w[JT];
    if (V == 4) {
      uw = *reinterpret_cast<const uint32_t*>(use + i);
      if ((uw & 0xFFu) && (uw & 0xFF00u) && (uw & 0xFF0000u) && (uw & 0xFF000000u)) continue;
      c1w = *reinterpret_cast<const uint32_t*>(c1p + i);
#pragma unroll
      for (int k = 0; k < JT; ++k)
        c2w[k] = k < nt ? *reinterpret_cast<const uint32_t*>(codes + (int64_t)(j2a + k) * ld + i) : 0u;
    } else {
      uw = (uint8_t)use[i];
      if (uw) continue;
      c1w = c1p[i];
#pragma unroll
      for (int k = 0; k < JT; ++k) c2w[k] = k < nt ? codes[(int64_t)(j2a + k) * ld + i] : 0u;
    }
    double pv[V];
#pragma unroll
    for (int v = 0; v < V; ++v) pv[v] = psi[i + v];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if ((uw >> (8 * v)) & 0xFFu) continue;      // not a training row
      const int c1 = (c1w >> (8 * v)) & 0xFFu;
      if (c1 >= nb1) continue;                    // a code past nb leaves the row out
      const double r = pv[v] - cst;
      const long long q = isfinite(r) ? __double2ll_rn(ldexp(r, e)) : 0ll;
#pragma unroll
      for (int k = 0; k < JT; ++k) {
        if (k < nt) {
          const int c2 = (c2w[k] >> (8 * v)) & 0xFFu;
          if (c2 < nb2[k]) {
            const int slot = small[k] ? (c1 * nb2[k] + c2) * 64 + lane : c1 * NBMAX + c2;
            ATE_DASSERT(slot >= 0 && slot < TILE);
            atomicAdd(&ss[k][slot], (unsigned long long)q);
            atomicAdd(&sc[k][slot], 1);
          }
        }
      }
    }
  }
  __syncthreads();
  for (int k = 0; k < nt; ++k) {
    unsigned long long* o = out + (int64_t)pair_index(d, j1, j2a + k) * 2 * TILE;
    if (small[k]) {
      // cell by cell: a wave sums the 64 lane copies, lane 0 adds the total
      for (int cell = wid; cell < nb1 * nb2[k]; cell += HT / 64) {
        const long long v = wave_sum((long long)ss[k][cell * 64 + lane]);
        const int n = wave_sum(sc[k][cell * 64 + lane]);
        if (lane == 0 && n != 0) {
          const int at = (cell / nb2[k]) * NBMAX + cell % nb2[k];
          atomicAdd(&o[at], (unsigned long long)v);
          atomicAdd(&o[TILE + at], (unsigned long long)n);
        }
      }
    } else {
      for (int c = t; c < nb1 * NBMAX; c += HT) {
        const int n = sc[k][c];
        if (n != 0) {
          atomicAdd(&o[c], ss[k][c]);
          atomicAdd(&o[TILE + c], (unsigned long long)n);
        }
      }
    }
  }
}

// ---------------------------------------------------------------- search
// one workgroup of 64 threads per tile plane: rows, then columns
__global__ __launch_bounds__(64) void policy_prefix_kernel(const long long* __restrict__ H,
                                                           long long* __restrict__ P) {
  __shared__ long long s[NBMAX][NBMAX + 1];
  const int t = threadIdx.x;
  const long long* h = H + (int64_t)blockIdx.x * TILE;
  long long* p = P + (int64_t)blockIdx.x * TILE;
  for (int r = 0; r < NBMAX; ++r) s[r][t] = h[r * NBMAX + t];
  __syncthreads();
  long long a = 0;
  for (int c = 0; c < NBMAX; ++c) { a += s[t][c]; s[t][c] = a; }   // row t
  __syncthreads();
  a = 0;
  for (int r = 0; r < NBMAX; ++r) { a += s[r][t]; s[r][t] = a; }   // column t
  __syncthreads();
  for (int r = 0; r < NBMAX; ++r) p[r * NBMAX + t] = s[r][t];
}

// the sum (plane 0) or row count (plane 1) over the training rows with code_a <= ta and
// code_b <= tb; t = 63 leaves that feature free
__device__ __forceinline__ long long psum(const long long* __restrict__ P, int d, int a, int ta,
                                          int b, int tb, int plane) {
  ATE_DASSERT(a >= 0 && a < d && b >= 0 && b < d && ta >= 0 && ta < NBMAX && tb >= 0 && tb < NBMAX);
  return a <= b ? P[((int64_t)pair_index(d, a, b) * 2 + plane) * TILE + ta * NBMAX + tb]
                : P[((int64_t)pair_index(d, b, a) * 2 + plane) * TILE + tb * NBMAX + ta];
}
__device__ __forceinline__ long long pos(long long v) { return v > 0 ? v : 0; }

struct Best {
  long long v;
  int key;      // -1 leaf, else j * 64 + t
};
// candidates in key order, a later one only if strictly better: the first maximum
__device__ __forceinline__ void take(Best& b, long long v, int key) {
  if (v > b.v || (v == b.v && key < b.key)) { b.v = v; b.key = key; }
}
__device__ inline Best block_best(Best b, Best* sh) {
  sh[threadIdx.x] = b;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int q = 1; q < (int)blockDim.x; ++q) take(b, sh[q].v, sh[q].key);
  __syncthreads();
  return b;     // valid in thread 0
}

// child [d * 64][4] int64: (value, key) of the left side's best depth-1 subtree, then the
// right side's; key -2 in slot 1 marks a root split that is not allowed
__global__ __launch_bounds__(ST) void policy_child_kernel(const long long* __restrict__ P,
                                                          const int* __restrict__ nb, int d,
                                                          long long min_leaf,
                                                          long long* __restrict__ child) {
  __shared__ Best sh[ST];
  const int j1 = blockIdx.x >> 6, t1 = blockIdx.x & 63;
  long long* o = child + (int64_t)blockIdx.x * 4;
  ATE_DASSERT(j1 < d);
  const long long ST0 = psum(P, d, 0, 63, 0, 63, 0), NT0 = psum(P, d, 0, 63, 0, 63, 1);
  const long long SL = psum(P, d, j1, t1, j1, 63, 0), NL = psum(P, d, j1, t1, j1, 63, 1);
  const long long SR = ST0 - SL, NR = NT0 - NL;
  if (t1 > clamp_nb(nb[j1]) - 2 || NL < min_leaf || NR < min_leaf) {    // block-uniform
    if (threadIdx.x == 0) { o[0] = 0; o[1] = -2; o[2] = 0; o[3] = -2; }
    return;
  }
  Best bl = {pos(SL), -1}, br = {pos(SR), -1};
  for (int key = threadIdx.x; key < d * 64; key += ST) {
    const int j2 = key >> 6, t2 = key & 63;
    if (t2 > clamp_nb(nb[j2]) - 2) continue;
    const long long SLL = psum(P, d, j1, t1, j2, t2, 0), NLL = psum(P, d, j1, t1, j2, t2, 1);
    const long long SAL = psum(P, d, j2, t2, j2, 63, 0), NAL = psum(P, d, j2, t2, j2, 63, 1);
    const long long SLR = SL - SLL, NLR = NL - NLL;
    const long long SRL = SAL - SLL, NRL = NAL - NLL;
    const long long SRR = SR - SRL, NRR = NR - NRL;
    ATE_DASSERT(NLL >= 0 && NLR >= 0 && NRL >= 0 && NRR >= 0);
    if (NLL >= min_leaf && NLR >= min_leaf) take(bl, pos(SLL) + pos(SLR), key);
    if (NRL >= min_leaf && NRR >= min_leaf) take(br, pos(SRL) + pos(SRR), key);
  }
  bl = block_best(bl, sh);
  br = block_best(br, sh);
  if (threadIdx.x == 0) { o[0] = bl.v; o[1] = bl.key; o[2] = br.v; o[3] = br.key; }
}

// node (j, t) and the two leaf actions of one side's best depth-1 subtree
__device__ inline void write_side(const long long* P, int d, int j1, int t1, bool right, int key,
                                  long long* node, long long* act) {
  const long long SL = psum(P, d, j1, t1, j1, 63, 0);
  const long long S = right ? psum(P, d, 0, 63, 0, 63, 0) - SL : SL;
  if (key < 0) {
    node[0] = -1; node[1] = -1;
    act[0] = act[1] = S > 0;
    return;
  }
  const int j2 = key >> 6, t2 = key & 63;
  const long long SLL = psum(P, d, j1, t1, j2, t2, 0);
  const long long lo = right ? psum(P, d, j2, t2, j2, 63, 0) - SLL : SLL;
  node[0] = j2; node[1] = t2;
  act[0] = lo > 0;
  act[1] = S - lo > 0;
}

__global__ __launch_bounds__(ST) void policy_pick_kernel(const long long* __restrict__ P,
                                                         const long long* __restrict__ child,
                                                         const int* __restrict__ nb, int d,
                                                         int depth, long long min_leaf,
                                                         long long* __restrict__ rec) {
  __shared__ Best sh[ST];
  const long long ST0 = psum(P, d, 0, 63, 0, 63, 0), NT0 = psum(P, d, 0, 63, 0, 63, 1);
  Best b = {pos(ST0), -1};
  if (depth >= 1)
    for (int key = threadIdx.x; key < d * 64; key += ST) {
      const int j1 = key >> 6, t1 = key & 63;
      if (t1 > clamp_nb(nb[j1]) - 2) continue;
      if (depth >= 2) {
        const long long* c = child + (int64_t)key * 4;
        if (c[1] != -2) take(b, c[0] + c[2], key);
      } else {
        const long long SL = psum(P, d, j1, t1, j1, 63, 0), NL = psum(P, d, j1, t1, j1, 63, 1);
        if (NL >= min_leaf && NT0 - NL >= min_leaf) take(b, pos(SL) + pos(ST0 - SL), key);
      }
    }
  b = block_best(b, sh);
  if (threadIdx.x != 0) return;
  for (int q = 0; q < REC; ++q) rec[q] = 0;
  rec[10] = b.v;
  rec[11] = NT0;
  if (b.key < 0) {
    for (int q = 0; q < 6; ++q) rec[q] = -1;
    for (int q = 6; q < 10; ++q) rec[q] = ST0 > 0;
    return;
  }
  const int j1 = b.key >> 6, t1 = b.key & 63;
  rec[0] = j1; rec[1] = t1;
  const int kl = depth >= 2 ? (int)child[(int64_t)b.key * 4 + 1] : -1;
  const int kr = depth >= 2 ? (int)child[(int64_t)b.key * 4 + 3] : -1;
  write_side(P, d, j1, t1, false, kl, rec + 2, rec + 6);
  write_side(P, d, j1, t1, true, kr, rec + 4, rec + 8);
}

}  // namespace

ATE_KERNEL_SHAPE("policy_pair_hist_kernel<4>", HT, 0, policy_pair_hist_kernel<4>)
ATE_KERNEL_SHAPE("policy_pair_hist_kernel<1>", HT, 0, policy_pair_hist_kernel<1>)
ATE_KERNEL_SHAPE("policy_prefix_kernel", 64, 0, policy_prefix_kernel)
ATE_KERNEL_SHAPE("policy_child_kernel", ST, 0, policy_child_kernel)
ATE_KERNEL_SHAPE("policy_pick_kernel", ST, 0, policy_pick_kernel)

// entries (int64) of the histogram of d features, also of the prefix-sum workspace of
// ate_policy_search, which needs d * 64 * 4 more for the children; -1: bad arguments
ATE_API int64_t ate_policy_pair_hist_scratch(int d) {
  if (d < 1 || d > DMAX) return -1;
  return (int64_t)(d * (d + 1) / 2) * 2 * TILE;
}

// psi [ld] fp64, cost [1] fp64 and e [1] int32 on the device, use [ld] int8 (0: a training
// row), codes [d][ld] uint8, nb [d] int32 on the device (bins per feature, 1..64; a row whose
// code of a feature is >= nb is left out of that feature's tiles, in every build: nothing is
// indexed past a tile. The search expects histograms of codes < nb). out [d (d + 1) / 2][2][64][64] int64, zeroed here. nbx: workgroups
// along the rows. priv: 1 gives tiles of at most 64 cells per-lane copies, 0 the plain path.
ATE_API int ate_policy_pair_hist(const void* psi, const void* cost, const void* e, const void* use,
                                 const void* codes, const void* nb, int64_t ld, int d, int nbx,
                                 int priv, void* out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (d < 1 || d > DMAX || nbx < 1 || nbx > 65535) return -1;
  if (ld < 1 || ld >= ((int64_t)1 << 31)) return -1;    // per-workgroup int32 counts
  const int64_t bytes = ate_policy_pair_hist_scratch(d) * 8;
  const hipError_t me = hipMemsetAsync(out, 0, bytes, s);
  if (me != hipSuccess) return (int)me;
  const bool words = ld % 4 == 0 && (uintptr_t)use % 4 == 0 && (uintptr_t)codes % 4 == 0;
  if (words)
    ATE_LAUNCH(policy_pair_hist_kernel<4>, dim3(nbx, hist_groups(d)), dim3(HT), 0, s,
               (const double*)psi, (const double*)cost, (const int*)e, (const int8_t*)use,
               (const uint8_t*)codes, (const int*)nb, ld, d, priv, (unsigned long long*)out);
  else
    ATE_LAUNCH(policy_pair_hist_kernel<1>, dim3(nbx, hist_groups(d)), dim3(HT), 0, s,
               (const double*)psi, (const double*)cost, (const int*)e, (const int8_t*)use,
               (const uint8_t*)codes, (const int*)nb, ld, d, priv, (unsigned long long*)out);
  ATE_CHECK_LAUNCH();
  return 0;
}

// hist: the (all-reduced) output of ate_policy_pair_hist; nb [d] int32 on the device.
// work: ate_policy_pair_hist_scratch(d) + d * 64 * 4 int64 entries. rec [16] int64.
ATE_API int ate_policy_search(const void* hist, const void* nb, int d, int depth,
                              int64_t min_leaf, void* work, void* rec, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (d < 1 || d > DMAX || depth < 0 || depth > 2 || min_leaf < 1) return -1;
  const int64_t np = (int64_t)(d * (d + 1) / 2);
  long long* P = (long long*)work;
  long long* child = P + np * 2 * TILE;
  ATE_LAUNCH(policy_prefix_kernel, dim3((unsigned)(np * 2)), dim3(64), 0, s,
             (const long long*)hist, P);
  ATE_CHECK_LAUNCH();
  if (depth >= 2) {
    ATE_LAUNCH(policy_child_kernel, dim3(d * 64), dim3(ST), 0, s, (const long long*)P,
               (const int*)nb, d, (long long)min_leaf, child);
    ATE_CHECK_LAUNCH();
  }
  ATE_LAUNCH(policy_pick_kernel, dim3(1), dim3(ST), 0, s, (const long long*)P,
             (const long long*)child, (const int*)nb, d, depth, (long long)min_leaf,
             (long long*)rec);
  ATE_CHECK_LAUNCH();
  return 0;
}
