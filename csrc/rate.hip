// Half-sample bootstrap of the rank-weighted average treatment effect of a priority rule
// (AUTOC, Qini and the TOC curve of DML-IRM's per-row scores; estimators/rate.py).
//
// The n evaluation rows arrive sorted by priority (order[j] = the panel row at position j,
// flags[j] below); rows of equal priority form a run that enters at once. For replicate b,
// with I_i^b in {0, 1} the half-sample inclusion of row i, along the positions j:
//   A_b(j) = S_{j' <= j} I psi,   M_b(j) = S_{j' <= j} I            (prefix sums)
// and at every run end k_r, with c = M_b(k_r) - M_b(k_{r-1}) the run's included count,
//   U_b += c A_b / M_b,   V_b += c A_b,   W_b += c M_b              (c > 0 only)
// At the flagged grid positions e_j the pair (A_b(e_j), M_b(e_j)) is stored. out [B + 1]
// [5 + 2 Q] = n_b, A_b(n), U_b, V_b, W_b, Q pairs; row 0 is the full sample (every row
// included), rows 1.. the replicates, all from the same walk.
//
// Inclusion: replicate b of the row with global id `id` is bit (b % 128) of
// rand4(seed, P_HALF, b / 128, id), the replicate -> (stream, word, bit) mapping of
// csrc/boot_common.hpp (parallel/rng.half_sample on the host). The full sample is replicate
// slot B: its bit is forced to 1 when a row's words are staged, so it costs no stream of its
// own unless B is a multiple of 128.
//
// Shape: the geometry of boot_common.hpp for B + 1 slots -- 32 threads per stream, four
// replicates per thread in registers, workgroups of CH = 64..256 threads. The positions are
// cut into nbx contiguous pieces [n bx / nbx, n (bx + 1) / nbx), one workgroup per (piece,
// stream block). A workgroup stages sub-chunks of CH positions in LDS (psi gathered through
// the order, the flags, the rows' Philox words) and every thread walks them in order: the
// prefix sums are sequential adds in registers, both LDS reads of a position are broadcasts.
//   1. rate_walk_kernel<false>: per (piece, replicate) the piece's S I psi, S I and the
//      local M at its last run end (-1: the piece holds no run end).
//   2. rate_offsets_kernel: per replicate, over the pieces in ascending order, each piece's
//      starting A, starting M and the M at the last run end before it (0: none yet). M never
//      decreases, so that one integer is enough to form c at a run end whose predecessor
//      lies any number of pieces back.
//   3. rate_walk_kernel<true>: the same walk from those offsets; U, V, W per workgroup, the
//      grid pairs and (from the last piece) n_b, A_b(n) straight to `out`.
//   then rate_sum_kernel adds the workgroups' U, V, W in piece order. No atomics and no
// workgroup waits on another: one launch geometry gives one set of bits. (A_b(n), n_b) is the
// walk's own state at the last position, so a grid point there repeats it bit for bit.
#include "boot_common.hpp"

using namespace ate;

namespace {

constexpr int QMAX = 64;

// flags[j]: bit 0 = position j ends a run; bits 1..7 = 1 + the first grid point whose rows
// end at j (0: none); bits 8..14 = how many consecutive grid points end there.
__device__ __forceinline__ int flag_grid0(int f) { return ((f >> 1) & 127) - 1; }
__device__ __forceinline__ int flag_gridn(int f) { return (f >> 8) & 127; }

// replicate slot of (stream, k, bit); slot B is the full sample, above it nothing
__device__ __forceinline__ int slot_of(int stream, int k, int bit) {
  return stream * 128 + k * 32 + bit;
}
__device__ __forceinline__ int64_t out_row(int slot, int B) { return slot == B ? 0 : slot + 1; }

// [(by * nbx + bx)][k < 4][CH] slabs: A / M / E of launches 1-2, then U / V / W of launch 3
template <bool PASS2>
__global__ __launch_bounds__(CHMAX) void rate_walk_kernel(
    const double* __restrict__ psi, const int* __restrict__ order, const int* __restrict__ flags,
    const int64_t* __restrict__ rid, int64_t ld, int64_t n, int Q, int B, int nst, uint64_t seed,
    double* __restrict__ SA, long long* __restrict__ SM, long long* __restrict__ SE,
    double* __restrict__ PU, double* __restrict__ PV, long long* __restrict__ PW,
    double* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint4 sw[CHMAX * SPWMAX];   // the positions' words
  __shared__ __attribute__((aligned(16))) double sp[CHMAX];           // psi through the order
  __shared__ int sf[CHMAX];                                           // flags
  const int CH = blockDim.x, nsw = CH >> 5;
  const int t = threadIdx.x, s = t >> 5, bit = t & 31;
  const int stream0 = blockIdx.y * nsw;
  const bool active = stream0 + s < nst;
  const int nbx = gridDim.x, bx = blockIdx.x;
  ATE_DASSERT(CH <= CHMAX && (CH & 63) == 0 && Q >= 1 && Q <= QMAX && n >= 1 && n <= ld);
  ATE_DASSERT(bx < nbx && nst == (B >> 7) + 1);
  const int64_t p0 = n * bx / nbx, p1 = n * (bx + 1) / nbx;           // n < 2^31, nbx < 2^16
  const int64_t slab = (((int64_t)blockIdx.y * nbx + bx) * 4) * CH + t;
  const int fs = B >> 7, fw = (B & 127) >> 5;                         // the full-sample slot
  const uint32_t fb = 1u << (B & 31);
  double a[4], u[4], v[4];
  long long m[4], last[4], w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t o = slab + (int64_t)k * CH;
    a[k] = PASS2 ? SA[o] : 0.0;
    m[k] = PASS2 ? SM[o] : 0;
    last[k] = PASS2 ? SE[o] : -1;
    u[k] = v[k] = 0.0;
    w[k] = 0;
  }
  for (int64_t c0 = p0; c0 < p1; c0 += CH) {
    const int cnt = (int)(p1 - c0 < CH ? p1 - c0 : CH);
    __syncthreads();                      // every thread has left the previous sub-chunk's walk
    if (t < cnt) {
      ATE_DASSERT(c0 + t >= 0 && c0 + t < n);
      const int64_t o = order[c0 + t];
      ATE_DASSERT(o >= 0 && o < ld);
      sp[t] = psi[o];
      sf[t] = flags[c0 + t];
      const int64_t id = rid[o];
      ATE_DASSERT(id >= 0);
      for (int q = 0; q < nsw; ++q) {
        const int st = stream0 + q;
        if (st < nst) {
          const u32x4 r = rand4(seed, P_HALF, (uint32_t)st, (uint64_t)id);
          uint32_t wd[4] = {r.x, r.y, r.z, r.w};
          if (st == fs) wd[fw] |= fb;
          ATE_DASSERT(t * nsw + q < CHMAX * SPWMAX);
          sw[t * nsw + q] = make_uint4(wd[0], wd[1], wd[2], wd[3]);
        }
      }
    }
    __syncthreads();
    if (!active) continue;
#pragma unroll 2
    for (int r = 0; r < cnt; ++r) {
      ATE_DASSERT(r < CH && r * nsw + s < CHMAX * SPWMAX);
      const double p = sp[r];
      const uint4 wq = sw[r * nsw + s];
      const int f = sf[r];
      const uint32_t wk[4] = {wq.x, wq.y, wq.z, wq.w};
      const int plo = __double2loint(p), phi = __double2hiint(p);
#pragma unroll
      for (int k = 0; k < 4; ++k) {       // e = -1 where the row is in the half sample, else 0
        const int e = __builtin_amdgcn_sbfe((int)wk[k], bit, 1);
        m[k] -= e;
        a[k] += __hiloint2double(phi & e, plo & e);                   // + psi, or + 0.0
      }
      if (f & 1) {                        // a run ends here (uniform)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (PASS2) {
            const long long c = m[k] - last[k];
            ATE_DASSERT(c >= 0);
            if (c > 0) {
              const double cd = (double)c, md = (double)m[k];
              u[k] = fma(cd, a[k] / md, u[k]);
              v[k] = fma(cd, a[k], v[k]);
              w[k] += c * m[k];
            }
          }
          last[k] = m[k];
        }
      }
      if (PASS2 && (f >> 1) != 0) {       // grid points whose rows end here (uniform)
        const int j0 = flag_grid0(f), jn = flag_gridn(f);
        ATE_DASSERT(j0 >= 0 && jn >= 1 && j0 + jn <= Q);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int slot = slot_of(stream0 + s, k, bit);
          if (slot > B) continue;
          double* row = out + out_row(slot, B) * (5 + 2 * Q) + 5;
          const double ga = m[k] > 0 ? a[k] : 0.0, gm = (double)m[k];
          for (int j = j0; j < j0 + jn; ++j) {
            row[2 * j] = ga;
            row[2 * j + 1] = gm;
          }
        }
      }
    }
  }
  if (!active) return;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t o = slab + (int64_t)k * CH;
    if (PASS2) {
      PU[o] = u[k];
      PV[o] = v[k];
      PW[o] = w[k];
      const int slot = slot_of(stream0 + s, k, bit);
      if (bx == nbx - 1 && slot <= B) {   // the last piece ends at position n - 1
        double* row = out + out_row(slot, B) * (5 + 2 * Q);
        row[0] = (double)m[k];
        row[1] = a[k];
      }
    } else {
      SA[o] = a[k];
      SM[o] = m[k];
      SE[o] = last[k];
    }
  }
}

// the slab entry (by, k, t) of thread g and its replicate slot; false past the slots of the
// ((B >> 7) + 1) streams in use (`all`), or past the B + 1 slots that have an output row
__device__ __forceinline__ bool slab_entry(int g, int B, int CH, int nby, bool all, int& by,
                                           int& kt, int& slot) {
  if (g >= nby * 4 * CH) return false;
  by = g / (4 * CH);
  kt = g - by * 4 * CH;
  const int k = kt / CH, t = kt - k * CH;
  slot = slot_of(by * (CH >> 5) + (t >> 5), k, t & 31);
  return all ? slot < ((B >> 7) + 1) * 128 : slot <= B;
}

// launch 2: the pieces' sums of launch 1 -> their exclusive prefixes, in place, in piece order
__global__ __launch_bounds__(256) void rate_offsets_kernel(
    double* __restrict__ SA, long long* __restrict__ SM, long long* __restrict__ SE, int B, int CH,
    int nbx, int nby) {
  int by, kt, slot;
  if (!slab_entry(blockIdx.x * 256 + threadIdx.x, B, CH, nby, true, by, kt, slot)) return;
  double ra = 0.0;
  long long rm = 0, re = 0;
#pragma unroll 4
  for (int bx = 0; bx < nbx; ++bx) {
    ATE_DASSERT(bx < nbx && kt < 4 * CH);
    const int64_t o = ((int64_t)by * nbx + bx) * 4 * CH + kt;
    const double pa = SA[o];
    const long long pm = SM[o], pe = SE[o];
    ATE_DASSERT(pm >= 0 && pe >= -1 && pe <= pm);
    SA[o] = ra;
    SM[o] = rm;
    SE[o] = re;
    if (pe >= 0) re = rm + pe;
    ra += pa;
    rm += pm;
  }
}

// after launch 3: U, V, W of the workgroups in piece order -> out[row][2..4]
__global__ __launch_bounds__(256) void rate_sum_kernel(
    const double* __restrict__ PU, const double* __restrict__ PV, const long long* __restrict__ PW,
    int Q, int B, int CH, int nbx, int nby, double* __restrict__ out) {
  int by, kt, slot;
  if (!slab_entry(blockIdx.x * 256 + threadIdx.x, B, CH, nby, false, by, kt, slot)) return;
  double su = 0.0, sv = 0.0;
  long long swt = 0;
#pragma unroll 4
  for (int bx = 0; bx < nbx; ++bx) {
    const int64_t o = ((int64_t)by * nbx + bx) * 4 * CH + kt;
    su += PU[o];
    sv += PV[o];
    swt += PW[o];
  }
  double* row = out + out_row(slot, B) * (5 + 2 * Q);
  row[2] = su;
  row[3] = sv;
  row[4] = (double)swt;
}

inline bool bad_rate(int Q, int B, int nbx, int64_t ld = 1) {
  return Q < 1 || Q > QMAX || bad_boot(B, nbx, ld);
}

}  // namespace

ATE_KERNEL_SHAPE("rate_walk_kernel<sums>", CHMAX, 0, rate_walk_kernel<false>)
ATE_KERNEL_SHAPE("rate_walk_kernel<walk>", CHMAX, 0, rate_walk_kernel<true>)
ATE_KERNEL_SHAPE("rate_offsets_kernel", 256, 0, rate_offsets_kernel)
ATE_KERNEL_SHAPE("rate_sum_kernel", 256, 0, rate_sum_kernel)

// bytes of the workspace of ate_rate_boot(Q, B, nbx); -1: bad arguments
ATE_API int64_t ate_rate_boot_scratch(int Q, int B, int nbx) {
  if (bad_rate(Q, B, nbx)) return -1;
  return slab_elems(geometry(B + 1), 1, nbx) * 6 * 8;
}

// psi [ld] fp64 and rid [ld] int64 global row ids in panel row order; order [n] int32 the
// panel row at every sorted position, flags [n] int32 (above). out [(B + 1) * (5 + 2 Q)]
// fp64. scratch: ate_rate_boot_scratch bytes, 16-byte aligned. nbx: pieces of the ranking.
ATE_API int ate_rate_boot(const void* psi, const void* order, const void* flags, const void* rid,
                          int64_t ld, int64_t n, int Q, int B, uint64_t seed, int nbx,
                          void* scratch, void* out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (bad_rate(Q, B, nbx, ld) || n < 1 || n > ld) return -1;
  const Geo q = geometry(B + 1);
  const int64_t na = slab_elems(q, 1, nbx);
  double* SA = (double*)scratch;
  long long* SM = (long long*)(SA + na);
  long long* SE = SM + na;
  double* PU = (double*)(SE + na);
  double* PV = PU + na;
  long long* PW = (long long*)(PV + na);
  const int small = (q.nby * 4 * q.CH + 255) / 256;
  ATE_LAUNCH(rate_walk_kernel<false>, dim3(nbx, q.nby), dim3(q.CH), 0, s, (const double*)psi,
             (const int*)order, (const int*)flags, (const int64_t*)rid, ld, n, Q, B, q.nst, seed,
             SA, SM, SE, PU, PV, PW, (double*)out);
  ATE_CHECK_LAUNCH();
  ATE_LAUNCH(rate_offsets_kernel, dim3(small), dim3(256), 0, s, SA, SM, SE, B, q.CH, nbx, q.nby);
  ATE_CHECK_LAUNCH();
  ATE_LAUNCH(rate_walk_kernel<true>, dim3(nbx, q.nby), dim3(q.CH), 0, s, (const double*)psi,
             (const int*)order, (const int*)flags, (const int64_t*)rid, ld, n, Q, B, q.nst, seed,
             SA, SM, SE, PU, PV, PW, (double*)out);
  ATE_CHECK_LAUNCH();
  ATE_LAUNCH(rate_sum_kernel, dim3(small), dim3(256), 0, s, (const double*)PU, (const double*)PV,
             (const long long*)PW, Q, B, q.CH, nbx, q.nby, (double*)out);
  ATE_CHECK_LAUNCH();
  return 0;
}
