// The Rademacher multiplier bootstrap core shared by the kernels that sum xi-weighted row
// terms per bucket: csrc/gate.hip (bucket = group) and csrc/cate.hip (bucket = knot span).
// What decides the draws, the launch geometry and the order of every partial sum lives here,
// once; what differs on purpose stays per file (each file's walk_run, cate's band sums).
//
// Multipliers: replicate b of the row with global id `id` has xi = +1 / -1 from bit
// (b % 128) of rand4(seed, P_MULT, b / 128, id): Philox stream b / 128, word (b % 128) / 32,
// bit b % 32 (parallel/rng.rademacher on the host). One Philox call serves 128 replicates of
// a row. In a workgroup of CH threads that owns the CH / 32 streams from stream0 on, thread t
// owns bit t % 32 of the four words of stream stream0 + t / 32, i.e. the four replicates
//   b = (stream0 + t / 32) * 128 + k * 32 + t % 32,   k < 4,
// and its partial sums sit at [(by * nbx + bx)][slot][k][t] of the workgroup slabs.
#pragma once
#include "common.hpp"

namespace ate {

constexpr int CHMAX = 256;   // rows per chunk = threads per workgroup (at most)
constexpr int SPWMAX = 8;    // Philox streams per workgroup (at most): CHMAX / 32

// Launch geometry for B replicates (estimators/gate.py multiplier_geometry on the host):
// nst streams of 128 replicates, 32 threads per stream, up to SPWMAX streams per workgroup of
// CH threads, nby workgroups along the streams.
struct Geo { int nst, CH, nsw, nby; };
inline Geo geometry(int B) {
  Geo q;
  q.nst = (B + 127) / 128;
  const int spw = q.nst < SPWMAX ? q.nst : SPWMAX;
  q.CH = 64 * ((spw + 1) / 2);
  q.nsw = q.CH / 32;
  q.nby = (q.nst + q.nsw - 1) / q.nsw;
  return q;
}
// fp64 elements of the [(by * nbx + bx)][slot][k < 4][CH] slabs
inline int64_t slab_elems(const Geo& q, int slots, int nbx) {
  return (int64_t)q.nby * nbx * slots * 4 * q.CH;
}

// replicates, workgroups along the rows, rows (per-workgroup integer counts: ld < 2^31)
inline bool bad_boot(int B, int nbx, int64_t ld = 1) {
  return B < 1 || B > 4096 || nbx < 1 || nbx > 65535 || ld < 1 || ld >= ((int64_t)1 << 31);
}

// Stable counting sort of a chunk's rows by key < KMAX (a power of two, at most 64): returns
// this row's position in bucket order (valid rows only; rows of a bucket keep their order)
// and leaves the run starts in start[0 .. KMAX]. wcnt: [CH / 64][KMAX]. Every thread of the
// workgroup calls it; three barriers inside, the first of which also ends the previous
// chunk's walks (they read what the caller writes next), the last of which publishes start.
template <int KMAX>
__device__ __forceinline__ int bucket_rows(bool valid, int key, int (*wcnt)[KMAX], int* start) {
  static_assert(KMAX <= 64 && (KMAX & (KMAX - 1)) == 0, "one lane of wave 0 per bucket");
  const int CH = blockDim.x, nw = CH >> 6;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  for (int q = t; q < nw * KMAX; q += CH) (&wcnt[0][0])[q] = 0;
  // lanes of this wave holding the same key, by ballots over its bits
  uint64_t same = __ballot(valid);
#pragma unroll
  for (int k = 0; (1 << k) < KMAX; ++k) {
    const uint64_t bk = __ballot(valid && ((key >> k) & 1));
    same &= ((key >> k) & 1) ? bk : ~bk;
  }
  const int rank = __popcll(same & ((1ull << lane) - 1ull));
  __syncthreads();          // table zeroed; every thread has left the previous chunk's walk
  if (valid && rank == 0) wcnt[wid][key] = __popcll(same);
  __syncthreads();
  if (t < 64) {             // wave 0: exclusive scan of the bucket totals, per-wave offsets
    int tot = 0;
    if (t < KMAX)
      for (int w = 0; w < nw; ++w) tot += wcnt[w][t];
    int inc = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(inc, o, 64);
      if (lane >= o) inc += u;
    }
    if (t < KMAX) {
      int off = inc - tot;
      start[t] = off;
      if (t == KMAX - 1) start[KMAX] = inc;
      for (int w = 0; w < nw; ++w) {
        const int cw = wcnt[w][t];
        wcnt[w][t] = off;
        off += cw;
      }
    }
  }
  __syncthreads();
  int pos = 0;
  if (valid) {
    pos = wcnt[wid][key] + rank;
    ATE_DASSERT(pos >= 0 && pos < CH && pos >= start[key] && pos < start[key + 1]);
  }
  return pos;
}

// The Philox words of the row with global id `id`, for the workgroup's nsw streams from
// stream0 on, to sw[pos * nsw + q]. Stored inverted: a set bit is the multiplier -1 (the
// walk_run of each file reads the sign from it).
__device__ __forceinline__ void store_words(uint4* sw, int pos, int nsw, int stream0, int nst,
                                            uint64_t seed, int64_t id) {
  for (int q = 0; q < nsw; ++q) {
    if (stream0 + q < nst) {
      const u32x4 r = rand4(seed, P_MULT, (uint32_t)(stream0 + q), (uint64_t)id);
      sw[pos * nsw + q] = make_uint4(~r.x, ~r.y, ~r.z, ~r.w);
    }
  }
}

// Fixed-order sum of the workgroup slabs PA (and the integer slabs PZ, when WITH_Z), for a
// grid of ceil(nby * slots * 4 * CH / 16) workgroups of 256 threads. A workgroup sums 16
// consecutive slab entries: thread (j, sl) adds the workgroups sl, sl + 16, ... of entry j
// in ascending order and the 16 slices are then added in slice order (deterministic for a
// given launch geometry). True for the one thread per entry that then holds the sums (a, z)
// of replicate b < B in `slot`. One barrier inside; every thread calls it.
template <bool WITH_Z>
__device__ __forceinline__ bool slab_sum(const double* __restrict__ PA, const int* __restrict__ PZ,
                                         int slots, int B, int CH, int nbx, int nby, double& a,
                                         long long& z, int& b, int& slot) {
  __shared__ double ra[16][16];
  __shared__ long long rz[WITH_Z ? 16 : 1][16];
  const int64_t per = (int64_t)slots * 4 * CH;      // a multiple of 16
  const int j = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int64_t idx = (int64_t)blockIdx.x * 16 + j;
  const int by = (int)(idx / per);
  const int64_t rem = idx - by * per;
  a = 0.0;
  z = 0;
  if (by < nby)
#pragma unroll 4
    for (int bx = sl; bx < nbx; bx += 16) {
      const int64_t o = ((int64_t)by * nbx + bx) * per + rem;
      a += PA[o];
      if (WITH_Z) z += PZ[o];
    }
  ra[sl][j] = a;
  if (WITH_Z) rz[sl][j] = z;
  __syncthreads();
  if (sl != 0 || by >= nby) return false;
  for (int q = 1; q < 16; ++q) {
    a += ra[q][j];
    if (WITH_Z) z += rz[q][j];
  }
  const int t = (int)(rem % CH), k = (int)((rem / CH) & 3);
  slot = (int)(rem / (4 * CH));
  b = (by * (CH >> 5) + (t >> 5)) * 128 + k * 32 + (t & 31);
  ATE_DASSERT(slot < slots);
  return b < B;
}

}  // namespace ate
