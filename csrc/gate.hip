// Grouped Rademacher multiplier bootstrap of per-row scores (group ATEs of DML-IRM with a
// simultaneous confidence band; estimators/gate.py).
//
// For every group g < G and replicate b < B, over the rows i with gid_i = g:
//   mom[g] = (n_g, S psi_i, S psi_i^2),   A[b][g] = S xi_i^b psi_i,   Z[b][g] = S xi_i^b
// with the Rademacher multipliers xi_i^b of csrc/boot_common.hpp (the draws, the bit ->
// replicate mapping, the launch geometry, the bucketing and the slab sum are shared with
// csrc/cate.hip there). The multipliers never leave registers / LDS. The centred sums of the
// bootstrap are A - theta_g Z, so no group mean is needed inside the pass.
//
// Shape: a workgroup of CH = 64..256 threads owns CH / 32 Philox streams (blockIdx.y picks
// which) and walks chunks of CH rows (blockIdx.x, grid stride). Per chunk: one row per
// thread is loaded, the rows are bucketed by group with a stable counting sort
// (bucket_rows), and psi plus the rows' Philox words are written to LDS
// in bucket order. Thread t then owns bit t % 32 of the four words of stream t / 32 -- four
// replicates -- and walks each group's run of rows with four fp64 accumulators and four
// integer bit counts: both LDS reads of a row (psi, the 16-byte word quad) are broadcasts.
// The group loop is wave-uniform, so no accumulator is indexed at run time: for G <= 8 they
// stay in registers for the whole kernel (the loop is unrolled), above that each thread
// keeps them in its own slots of the workgroup's partial slab. Z is accumulated as integers
// (rows - 2 x the count of -1s). The group moments are summed at load time by the first
// stream block: lane g of each wave collects group g's rows from the wave's 64 lanes
// (readlane, row order). No atomics: per-workgroup partials, combined in a fixed order by
// gate_sum_kernel, so one launch geometry gives one set of bits.
#include "boot_common.hpp"

using namespace ate;

namespace {

constexpr int GREG = 8;      // up to this many groups: accumulators in registers
constexpr int GMAX = 64;

struct Acc {
  double a[4];
  int z[4];
};

__device__ __forceinline__ void acc_zero(Acc& c) {
#pragma unroll
  for (int k = 0; k < 4; ++k) { c.a[k] = 0.0; c.z[k] = 0; }
}

// one group's run [r0, r1) of the bucketed chunk into this thread's four replicates. The
// words are stored inverted: e = the bit as a sign-extended field is 0 where the multiplier is
// +1 and -1 where it is -1, so xi = e | 1 and the count of -1s is the sum of -e.
__device__ __forceinline__ void walk_run(const double* sp, const uint4* sw, int nsw, int s,
                                         int bit, int r0, int r1, Acc& c) {
  int n[4] = {0, 0, 0, 0};
#pragma unroll 2
  for (int r = r0; r < r1; ++r) {
    const double p = sp[r];
    const uint4 w = sw[r * nsw + s];
    const uint32_t wk[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = __builtin_amdgcn_sbfe((int)wk[k], bit, 1);
      n[k] -= e;
      c.a[k] = fma(p, (double)(e | 1), c.a[k]);     // p * (+1 | -1) is exact: an add of +/-p
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) c.z[k] += (r1 - r0) - 2 * n[k];
}

// partial slabs: PA / PZ [(by * nbx + bx)][g][k < 4][CH], PM [bx][g][3]
template <bool REG>
__global__ __launch_bounds__(CHMAX) void gate_boot_kernel(
    const double* __restrict__ psi, const int* __restrict__ gid, const int64_t* __restrict__ rid,
    int64_t ld, int G, int nst, uint64_t seed, double* __restrict__ PA, int* __restrict__ PZ,
    double* __restrict__ PM) {
  __shared__ __attribute__((aligned(16))) uint4 sw[CHMAX * SPWMAX];   // bucketed Philox words
  __shared__ __attribute__((aligned(16))) double sp[CHMAX];           // bucketed psi
  __shared__ __attribute__((aligned(16))) double lm[CHMAX / 64][GMAX * 3];   // moments per wave
  __shared__ int wcnt[CHMAX / 64][GMAX];                              // rows per (wave, group)
  __shared__ int start[GMAX + 1];                                     // run starts
  const int CH = blockDim.x, nsw = CH >> 5, nw = CH >> 6;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int s = t >> 5, bit = t & 31;
  const int stream0 = blockIdx.y * nsw;
  const bool active = stream0 + s < nst;
  const bool domom = blockIdx.y == 0;     // the first stream block also sums the moments:
  double m1 = 0.0, m2 = 0.0;              // lane g of every wave holds group g's, over the
  int mn = 0;                             // wave's 64 rows of every chunk, in row order
  ATE_DASSERT(G >= 1 && G <= GMAX && (!REG || G <= GREG) && CH <= CHMAX && (CH & 63) == 0);
  const int64_t slab = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * G * 4 * CH;
  Acc c[REG ? GREG : 1];
  if (REG) {
#pragma unroll
    for (int g = 0; g < (REG ? GREG : 1); ++g) acc_zero(c[g]);
  } else {
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        PA[slab + ((int64_t)g * 4 + k) * CH + t] = 0.0;
        PZ[slab + ((int64_t)g * 4 + k) * CH + t] = 0;
      }
  }
  const int64_t nchunk = (ld + CH - 1) / CH;
  for (int64_t ck = blockIdx.x; ck < nchunk; ck += gridDim.x) {
    const int64_t i = ck * CH + t;
    int g = i < ld ? gid[i] : -1;
    ATE_DASSERT(g >= -1 && g < G);
    const bool valid = g >= 0 && g < G;
    if (!valid) g = 0;
    const double p = valid ? psi[i] : 0.0;
    if (domom) {
      const int gv = valid ? g : -1, plo = __double2loint(p), phi = __double2hiint(p);
#pragma unroll 8
      for (int k = 0; k < 64; ++k) {
        const int sg = __builtin_amdgcn_readlane(gv, k);
        const double q = __hiloint2double(__builtin_amdgcn_readlane(phi, k),
                                          __builtin_amdgcn_readlane(plo, k));
        if (lane == sg) { m1 += q; m2 += q * q; mn += 1; }
      }
    }
    const int64_t id = valid ? rid[i] : 0;
    ATE_DASSERT(id >= 0);
    const int pos = bucket_rows<GMAX>(valid, g, wcnt, start);
    if (valid) {
      sp[pos] = p;
      store_words(sw, pos, nsw, stream0, nst, seed, id);
    }
    __syncthreads();
    if (active) {
      if (REG) {
#pragma unroll
        for (int gg = 0; gg < (REG ? GREG : 1); ++gg)
          if (gg < G) walk_run(sp, sw, nsw, s, bit, start[gg], start[gg + 1], c[gg]);
      } else {
        for (int gg = 0; gg < G; ++gg) {
          const int r0 = start[gg], r1 = start[gg + 1];
          if (r0 == r1) continue;
          const int64_t o = slab + (int64_t)gg * 4 * CH + t;
#pragma unroll
          for (int k = 0; k < 4; ++k) { c[0].a[k] = PA[o + (int64_t)k * CH]; c[0].z[k] = PZ[o + (int64_t)k * CH]; }
          walk_run(sp, sw, nsw, s, bit, r0, r1, c[0]);
#pragma unroll
          for (int k = 0; k < 4; ++k) { PA[o + (int64_t)k * CH] = c[0].a[k]; PZ[o + (int64_t)k * CH] = c[0].z[k]; }
        }
      }
    }
  }
  if (REG) {
#pragma unroll
    for (int g = 0; g < (REG ? GREG : 1); ++g)
      if (g < G)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          PA[slab + ((int64_t)g * 4 + k) * CH + t] = c[g].a[k];
          PZ[slab + ((int64_t)g * 4 + k) * CH + t] = c[g].z[k];
        }
  }
  if (domom) {                            // uniform: the waves' moments in wave order
    __syncthreads();
    lm[wid][lane * 3 + 0] = (double)mn;
    lm[wid][lane * 3 + 1] = m1;
    lm[wid][lane * 3 + 2] = m2;
    __syncthreads();
    for (int q = t; q < G * 3; q += CH) {   // G * 3 may exceed the workgroup
      double v = 0.0;
      for (int w = 0; w < nw; ++w) v += lm[w][q];
      PM[(int64_t)blockIdx.x * G * 3 + q] = v;
    }
  }
}

// out = mom [G][3] | A [B][G] | Z [B][G]: the group moments of the workgroups in ascending
// order, A and Z by the fixed-order slab_sum.
__global__ __launch_bounds__(256) void gate_sum_kernel(
    const double* __restrict__ PA, const int* __restrict__ PZ, const double* __restrict__ PM,
    int G, int B, int CH, int nbx, int nby, double* __restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x < G * 3) {
    double v = 0.0;
    for (int bx = 0; bx < nbx; ++bx) v += PM[(int64_t)bx * G * 3 + threadIdx.x];
    out[threadIdx.x] = v;
  }
  double a;
  long long z;
  int b, g;
  if (!slab_sum<true>(PA, PZ, G, B, CH, nbx, nby, a, z, b, g)) return;
  out[(int64_t)G * 3 + (int64_t)b * G + g] = a;
  out[(int64_t)G * 3 + (int64_t)B * G + (int64_t)b * G + g] = (double)z;
}

}  // namespace

ATE_KERNEL_SHAPE("gate_boot_kernel<reg>", CHMAX, 0, gate_boot_kernel<true>)
ATE_KERNEL_SHAPE("gate_boot_kernel<slab>", CHMAX, 0, gate_boot_kernel<false>)

// bytes of the partial workspace of ate_group_boot(G, B, nbx); -1: bad arguments
ATE_API int64_t ate_group_boot_scratch(int G, int B, int nbx) {
  if (G < 1 || G > GMAX || bad_boot(B, nbx)) return -1;
  return slab_elems(geometry(B), G, nbx) * 12 + (int64_t)nbx * G * 3 * 8;
}

// psi [ld] fp64, gid [ld] int32 (group in [0, G), -1: skip the row), rid [ld] int64 global
// row ids (read where gid >= 0). out [G*3 + 2*B*G] fp64: mom | A | Z. scratch:
// ate_group_boot_scratch bytes, 16-byte aligned. nbx: workgroups along the rows.
ATE_API int ate_group_boot(const void* psi, const void* gid, const void* rid, int64_t ld, int G,
                           int B, uint64_t seed, int nbx, void* scratch, void* out,
                           void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (G < 1 || G > GMAX || bad_boot(B, nbx, ld)) return -1;
  const Geo q = geometry(B);
  const int64_t na = slab_elems(q, G, nbx);
  double* PA = (double*)scratch;
  double* PM = PA + na;
  int* PZ = (int*)(PM + (int64_t)nbx * G * 3);
  if (G <= GREG)
    ATE_LAUNCH(gate_boot_kernel<true>, dim3(nbx, q.nby), dim3(q.CH), 0, s, (const double*)psi,
               (const int*)gid, (const int64_t*)rid, ld, G, q.nst, seed, PA, PZ, PM);
  else
    ATE_LAUNCH(gate_boot_kernel<false>, dim3(nbx, q.nby), dim3(q.CH), 0, s, (const double*)psi,
               (const int*)gid, (const int64_t*)rid, ld, G, q.nst, seed, PA, PZ, PM);
  ATE_CHECK_LAUNCH();
  const int64_t items = (int64_t)q.nby * G * 4 * q.CH;
  ATE_LAUNCH(gate_sum_kernel, dim3((unsigned)((items + 15) / 16)), dim3(256), 0, s,
             (const double*)PA, (const int*)PZ, (const double*)PM, G, B, q.CH, nbx, q.nby,
             (double*)out);
  ATE_CHECK_LAUNCH();
  return 0;
}
