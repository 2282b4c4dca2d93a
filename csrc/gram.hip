// K01 gram_syrk_mfma: G_s = X_s' D X_s for every row segment s (cross-fit fold),
// X column-major [P][ld] (bf16 or fp32), D = diag(w) optional (fp32 path).
//
// Work decomposition (tall-skinny SYRK, reduction dim = rows):
//   workgroup = (row chunk c, upper-triangular output tile t). Chunks never cross
//   a segment, so per-fold Grams fall out of the same launch. Each workgroup
//   writes its fp32 tile partial to a slab; a second kernel reduces the slab
//   per segment in a FIXED chunk order in fp64 (bitwise reproducible, no atomics).
//   Block ids are remapped so that all tiles of one row chunk run on the same
//   XCD (they re-read the same rows of X from that XCD's L2).
//
// bf16 path: 128x128 tile / 256 threads (2x2 waves of 64x64), K-step 64 rows,
//   mfma_f32_16x16x32_bf16, A/B tiles staged through LDS with a per-column XOR
//   swizzle of the 16-byte chunks (conflict-reduced ds_read_b128), register
//   double-buffered global loads. Padding rows are all-zero, so they add nothing.
// fp32/fp64 path: 64x64 tile, K-step 16 rows, mfma_f32_16x16x4f32 / mfma_f64_16x16x4f64
//   (fp64 = the parity mode, exact enough for lm-style rank detection), optional
//   row weights fused into the A-tile staging.
#include "common.hpp"

using namespace ate;

struct Chunk { int64_t row0, row1; int seg, pad; };

__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  // bijective remap: blocks b, b+8, b+16... (same XCD label) get consecutive logical ids
  int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (bid >> 3);
}

// ------------------------------------------------------------------ bf16 128x128
constexpr int BT = 128;      // tile
constexpr int BK = 64;       // rows per K-step

__global__ __launch_bounds__(256) void gram_bf16_kernel(
    const bf16_t* __restrict__ X, int64_t ld, const int2* __restrict__ tiles, int ntiles,
    const Chunk* __restrict__ chunks, int nchunks, float* __restrict__ slab) {
  __shared__ __attribute__((aligned(16))) bf16_t lds[2][2][BT * BK];   // [buf][A/B][col*64+row]
  const int L = xcd_remap(blockIdx.x, gridDim.x);
  const int c = L / ntiles, t = L % ntiles;
  const Chunk ch = chunks[c];
  const int2 tl = tiles[t];
  const bool diag = tl.x == tl.y;
  const int a0 = tl.x * BT, b0 = tl.y * BT;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // staging map: 128 cols x 8 chunks of 16B = 1024 loads; thread does 4 (A) + 4 (B)
  uint4 ra[4], rb[4];
  auto gload = [&](int64_t i0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int idx = r * 256 + tid, col = idx >> 3, cc = idx & 7;
      ra[r] = *reinterpret_cast<const uint4*>(X + (int64_t)(a0 + col) * ld + i0 + cc * 8);
      if (!diag) rb[r] = *reinterpret_cast<const uint4*>(X + (int64_t)(b0 + col) * ld + i0 + cc * 8);
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int idx = r * 256 + tid, col = idx >> 3, cc = idx & 7;
      int off = col * BK + ((cc ^ (col & 7)) << 3);
      *reinterpret_cast<uint4*>(&lds[buf][0][off]) = ra[r];
      if (!diag) *reinterpret_cast<uint4*>(&lds[buf][1][off]) = rb[r];
    }
  };

  const int64_t nsteps = (ch.row1 - ch.row0) / BK;
  if (nsteps > 0) {
    gload(ch.row0);
    lstore(0);
  }
  __syncthreads();
  for (int64_t s = 0; s < nsteps; ++s) {
    const int buf = s & 1;
    if (s + 1 < nsteps) gload(ch.row0 + (s + 1) * BK);
    const bf16_t* As = lds[buf][0];
    const bf16_t* Bs = diag ? lds[buf][0] : lds[buf][1];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int cc = kk * 4 + (lane >> 4);
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        int col = wr * 64 + m * 16 + (lane & 15);
        af[m] = *reinterpret_cast<const bf16x8*>(&As[col * BK + ((cc ^ (col & 7)) << 3)]);
      }
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        int col = wc * 64 + n * 16 + (lane & 15);
        bfr[n] = *reinterpret_cast<const bf16x8*>(&Bs[col * BK + ((cc ^ (col & 7)) << 3)]);
      }
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[m], bfr[n], acc[m][n], 0, 0, 0);
    }
    if (s + 1 < nsteps) lstore(buf ^ 1);
    __syncthreads();
  }
  // epilogue: acc reg r of lane l = C[row=(l>>4)*4+r][col=l&15]
  float* out = slab + ((int64_t)c * ntiles + t) * (BT * BT);
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = wr * 64 + m * 16 + (lane >> 4) * 4 + r;
        int col = wc * 64 + n * 16 + (lane & 15);
        out[row * BT + col] = acc[m][n][r];
      }
}

// ------------------------------------------------------------------ bf16 256x256, LDS-DMA staged
// 512 threads = 8 waves as 2 (rows) x 4 (cols); each wave owns a 128x64 output block
// (8x4 tiles of mfma_f32_16x16x32_bf16 -> 128 accumulator registers). Per 64-row
// K-step the A and B panels (256 columns x 64 rows x bf16 = 32 KB each) are copied
// global -> LDS with global_load_lds_dwordx4 (no VGPR round trip), double buffered so
// the copy of step s+1 overlaps the 64 MFMAs/wave of step s. The LDS image is written
// lane-linearly, so the per-column XOR swizzle of the 16-byte chunks is applied on the
// SOURCE address (chunk (l&7)^(col&7) lands at position l&7) and undone on the read.
constexpr int GT = 256;
constexpr int GK = 64;

typedef const __attribute__((address_space(1))) char* gptr_t;   // a global-memory address
__device__ __forceinline__ void glds16(gptr_t src, bf16_t* lds_base) {
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)(lds_base), 16, 0, 0);
}
__device__ __forceinline__ void glds16(const void* src, bf16_t* lds_base) {
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)(lds_base), 16, 0, 0);
}

__global__ __launch_bounds__(512) void gram_bf16_256_kernel(
    const bf16_t* __restrict__ X, int64_t ld, const int2* __restrict__ tiles, int ntiles,
    const Chunk* __restrict__ chunks, int nchunks, float* __restrict__ slab) {
  __shared__ __attribute__((aligned(16))) bf16_t lds[2][2][GT * GK];   // 128 KB
  const int L = xcd_remap(blockIdx.x, gridDim.x);
  const int c = L / ntiles, t = L % ntiles;
  const Chunk ch = chunks[c];
  const int2 tl = tiles[t];
  const bool diag = tl.x == tl.y;
  const int a0 = tl.x * GT, b0 = tl.y * GT;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 2, wc = wid & 3;

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // each wave issues 4 x 1 KB pieces per panel: piece q covers columns q*8 .. q*8+7
  auto stage = [&](int st, int64_t i0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = wid * 4 + r;
      const int col = q * 8 + (lane >> 3);
      const int cc = (lane & 7) ^ (col & 7);
      glds16(X + (int64_t)(a0 + col) * ld + i0 + cc * 8, &lds[st][0][q * 8 * GK]);
      if (!diag) glds16(X + (int64_t)(b0 + col) * ld + i0 + cc * 8, &lds[st][1][q * 8 * GK]);
    }
  };

  const int64_t nsteps = (ch.row1 - ch.row0) / GK;
  if (nsteps > 0) stage(0, ch.row0);
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
  __syncthreads();
  for (int64_t s = 0; s < nsteps; ++s) {
    const int cur = s & 1;
    if (s + 1 < nsteps) stage(cur ^ 1, ch.row0 + (s + 1) * GK);
    const bf16_t* As = lds[cur][0];
    const bf16_t* Bs = diag ? lds[cur][0] : lds[cur][1];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int cc = kk * 4 + (lane >> 4);
      bf16x8 af[8], bfr[4];
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const int col = wr * 128 + m * 16 + (lane & 15);
        af[m] = *reinterpret_cast<const bf16x8*>(&As[col * GK + ((cc ^ (col & 7)) << 3)]);
      }
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int col = wc * 64 + n * 16 + (lane & 15);
        bfr[n] = *reinterpret_cast<const bf16x8*>(&Bs[col * GK + ((cc ^ (col & 7)) << 3)]);
      }
#pragma unroll
      for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[m], bfr[n], acc[m][n], 0, 0, 0);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): next stage landed
    __syncthreads();
  }
  float* out = slab + ((int64_t)c * ntiles + t) * (GT * GT);
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wr * 128 + m * 16 + (lane >> 4) * 4 + r;
        const int col = wc * 64 + n * 16 + (lane & 15);
        out[row * GT + col] = acc[m][n][r];
      }
}

// ------------------------------------------------------------------ bf16 paired-tile kernel
// Symmetry-aware decomposition for P % 512 == 0. For a pair of 256-column tiles (a, b)
// two workgroups stream the SAME 512 columns of a row chunk:
//   type 0: the off-diagonal tile (a, b), 8 waves x (128 x 64) = 256 16x16 MFMA blocks;
//   type 1: the upper TRIANGLES of both diagonal tiles (a, a) and (b, b) = 2 x 136 blocks.
//           Per diagonal tile: two waves own the 8 x 8-block rectangle (rows 0-127 x cols
//           128-255, 32 blocks each) and two waves the triangles I <= J inside rows/cols
//           0-127 and 128-255 (36 blocks each, 8 fragments serve as both A and B);
//   type 2: type 1 for a single diagonal tile (odd tile count; b's waves idle).
// So MFMA work is 528 blocks per 512 columns instead of 768 (three full 256 tiles), and
// the two workgroups of a chunk read identical byte streams in lockstep (one of them
// hits L2 on what the other fetched). Every wave writes its 16x16 blocks contiguously
// into a 272-block slab slot; a host-built table maps slab blocks to Gram blocks.
constexpr int PAIR_SLOTS = 272;
constexpr int PAIR_LDS = 2 * 2 * GT * GK;   // bf16 elements: two stages of an A and a B image
// Variants measured and not kept (a ring of 32-row stages, crossed issue orders, a
// non-temporal panel stream, balanced 34-block roles, a split-triangle kernel): profiles/.
#ifndef GRAM_PRIO
// s_setprio 1 for waves 4-7 of the paired-tile kernel (see gram_bf16_pair_kernel):
// 1 = in every workgroup, 2 = in diagonal-pair workgroups only (their waves 4-7 are the
// heavier triangle waves; the off-diagonal tile's waves are symmetric). Tile kernel, one
// box: none 2.66-2.67, 1: 2.60, 2: 2.57 ms, same bits (profiles/r05_gram_sync)
#define GRAM_PRIO 2
#endif

__device__ __forceinline__ int tri_index(int m, int n) {   // m <= n < 8, row-major triangle
  return m * 8 - (m * (m - 1)) / 2 + (n - m);
}

constexpr int PAIR_RECT = 0, PAIR_RECT_D0 = 1, PAIR_TRI = 2, PAIR_RECT_D1 = 3;
template <int MODE> struct PairRole {
  static constexpr bool TRI = MODE == PAIR_TRI;
  static constexpr int NB = TRI ? 36 : 32;
};

// The MFMAs of one 32-deep k-step of a wave role: a rectangle (8 A x 4 B fragments) or a
// triangle (8 fragments as A and B, blocks m <= n in tri_index order).
// COLS (triangle): the same blocks column by column (n outer), so block column n needs
// fragments 0..n only and a fragment made in registers can follow the MFMAs of the columns
// before it; every accumulator still gets one product per call.
template <int MODE, bool COLS = false>
__device__ __forceinline__ void pair_mfma(f32x4* acc, const bf16x8* af, const bf16x8* bfr) {
  if constexpr (MODE == PAIR_TRI && COLS) {
#pragma unroll
    for (int n = 0; n < 8; ++n)
#pragma unroll
      for (int m = 0; m <= n; ++m)
        acc[tri_index(m, n)] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af[m], af[n], acc[tri_index(m, n)], 0, 0, 0);
  } else if constexpr (MODE != PAIR_TRI) {
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n)
        acc[m * 4 + n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[m], bfr[n], acc[m * 4 + n],
                                                                 0, 0, 0);
  } else {
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = m; n < 8; ++n)
        acc[tri_index(m, n)] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af[m], af[n], acc[tri_index(m, n)], 0, 0, 0);
  }
}

// One wave role for the whole K-loop (MODE: PAIR_TRI = triangle wave, else a rectangle wave;
// PAIR_RECT_D0 / D1 = the rectangle waves of a diagonal-pair workgroup, halves 0 / 1). Each
// instantiation keeps only its own accumulators live; every wave runs the same number of
// barriers.
// One-byte columns (X8 != null; P == 512): physical columns 384..511 -- tile b's second half,
// the panel's {0, 1}-valued columns (data/device_dgp.synthetic_panel puts them there) -- are
// also kept as bytes, [row block][128 columns][64 rows], byte 0x3F for 1. The B image of a
// stage then holds tile b's columns 0..127 as bf16 and 128..255 as bytes (24 KB instead of
// 32: a chunk streams 896 instead of 1,024 bytes per row). A byte column's 16-byte piece q
// (rows 8q..8q+7 and 32+8q..32+8q+7, csrc/dgp.hip x8_pos) sits at slot q ^ ((column >> 1) & 2):
// lane l reads both MFMA halves' rows of its column with one ds_read_b128, conflict-free over
// that instruction's 16-lane groups. v_perm puts each byte into the high byte of a bf16
// (0x3F00 = 0.5), so the MFMA products are exact halves and the slab reduce scales them back
// by 2 per byte column: the same Gram bits.
__device__ __forceinline__ bf16x8 bytes_to_bf16x8(uint2 d) {
  uint4 w;
  w.x = __builtin_amdgcn_perm(0u, d.x, 0x010C000Cu);
  w.y = __builtin_amdgcn_perm(0u, d.x, 0x030C020Cu);
  w.z = __builtin_amdgcn_perm(0u, d.y, 0x010C000Cu);
  w.w = __builtin_amdgcn_perm(0u, d.y, 0x030C020Cu);
  return __builtin_bit_cast(bf16x8, w);
}
constexpr int PAIR_BYTE0 = 384;   // first one-byte column (P == 512)

// Bit columns (COL_BITS; the same 128 columns from the panel's bit image, csrc/dgp.hip
// x1_byte): 16 bytes per row and 1 KB per stage instead of 128 and 8 KB, so a chunk streams
// 784 bytes per row. The 1 KB is one LDS-DMA piece (wave 0 copies it verbatim). A lane's 16
// bits of a column -- both halves' rows -- are one halfword: low byte the even rows, high
// byte the odd rows, bit t for rows 2j, 2j+1 of half t >> 2 (j = t & 3). The halfwords of
// the four column blocks of a 64-column plane are 8 contiguous bytes per lane, lane-linear:
// a rectangle wave reads its plane with one ds_read_b64 per stage and a triangle wave both
// planes with two (stride 8 over 32 lanes: every bank once per lane group). bits_rep spreads
// a halfword as bytes [lo, hi, hi, lo]; dword t of the fragments is then (w << (14 - t)) &
// 0x40004000: a one is bf16 0x4000 = 2.0, so the products are exact doubles (or fourfolds)
// and the slab reduce scales them back by 0.5 per bit column: the same Gram bits.
template <int HW>
__device__ __forceinline__ uint32_t bits_rep(uint32_t d) {
  return __builtin_amdgcn_perm(0u, d, HW ? 0x02030302u : 0x00010100u);
}
template <int H>
__device__ __forceinline__ bf16x8 bits_to_bf16x8(uint32_t w) {
  uint4 v;
  v.x = (w << (14 - 4 * H)) & 0x40004000u;
  v.y = (w << (13 - 4 * H)) & 0x40004000u;
  v.z = (w << (12 - 4 * H)) & 0x40004000u;
  v.w = (w << (11 - 4 * H)) & 0x40004000u;
  return __builtin_bit_cast(bf16x8, v);
}
// column modes of the paired-tile kernel: all bf16, or physical columns 384..511 as one-byte
// or as bit columns
constexpr int COL_BF16 = 0, COL_BYTES = 1, COL_BITS = 2;
template <int MASK, int N>
__device__ __forceinline__ void sched_group() {
  if constexpr (N > 0) __builtin_amdgcn_sched_group_barrier(MASK, N, 0);
}

// Schedules of the double-buffered K-loop (ate_gram_bf16_pair `sched`, ops/gram.py GRAM_SCHED):
// lockstep: all eight waves run one program; stagger: waves 4-7 run half a stage behind their
// SIMD partners 0-3 (LATE below). An L2 warm-ahead of the panel stream was measured with both
// and dropped (profiles/gram_handoff).
constexpr int SCHED_LOCKSTEP = 0, SCHED_STAGGER = 1;

// BYTES: the launch streams one-byte columns (X8 != null); BY: this wave's B fragments
// (rectangle) or all its fragments (triangle) are byte columns.
// LATE (waves 4-7 of the stagger schedule): the K-loop is rotated by half a stage. Between
// barriers s-1 and s the wave multiplies half 1 of stage s-1 from the registers that hold it
// since before barrier s-1 (beside its reads of half 0 of stage s), issues its copies of stage
// s+1, then multiplies half 0 of stage s beside its reads of half 1 of stage s; the last half 1
// follows the last barrier. So while waves 0-3 of the same SIMDs issue their copies and wait
// for their first fragments, the matrix pipe runs the late waves' held half. Every wave still
// reads stage s from LDS only between barriers s-1 and s and executes 1 + nsteps barriers
// (the loop's barriers sit outside every role- or idle-dependent branch), and every
// accumulator still adds half 0 then half 1 of the stages in stage order: the same bits.
// CM: the launch's column mode (COL_*; X8 = the byte or the bit image, null for COL_BF16).
template <int MODE, int CM, bool BY, bool LATE, bool SADDR>
__device__ __forceinline__ void pair_wave(const bf16_t* __restrict__ X, int64_t cs, int64_t bs, int a0,
                                          int b0, bool haveB, bool idle, int abuf, int bbuf,
                                          int arow0, int bcol0, const Chunk& ch,
                                          bf16_t* lds_raw, float* __restrict__ out,
                                          const uint8_t* __restrict__ X8) {
  constexpr bool BYTES = CM != COL_BF16;   // tile b's columns 128..255 are not staged as bf16
  constexpr bool BITS = CM == COL_BITS;
  constexpr bool TRI = PairRole<MODE>::TRI;
  constexpr int NB = PairRole<MODE>::NB;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  f32x4 acc[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16_t (*lds)[2][GT * GK] = reinterpret_cast<bf16_t (*)[2][GT * GK]>(lds_raw);
  // SADDR (the schedules other than lockstep): every piece's address is a wave-uniform base
  // plus ONE per-lane byte offset -- lane l of a piece reads chunk (l & 7) ^ (l >> 3) of column
  // l >> 3 of its 8 columns, whichever piece it is -- so the copies need one address register
  // instead of a pointer per piece (the late waves have none to spare)
  const int wu = __builtin_amdgcn_readfirstlane(wid);
  const uint32_t voff_ = (uint32_t)(((lane >> 3) * cs + (((lane & 7) ^ (lane >> 3)) << 3)) * 2);
  const uint32_t voff8_ = BITS ? (uint32_t)(lane * 16)
                               : (uint32_t)((lane >> 2) * GK + (((lane & 3) ^ ((lane >> 3) & 2)) << 4));
  auto stage = [&](int st, int64_t i0) {
    if constexpr (SADDR) {
      gptr_t Xk0 = (gptr_t) reinterpret_cast<const char*>(X + (i0 >> 6) * bs);
      // (opaque per stage: a sum of base and offset hoisted out of the K-loop would be a
      // 64-bit pointer per piece again)
      uint32_t voff = voff_, voff8 = voff8_;
#if defined(__HIP_DEVICE_COMPILE__)
      asm volatile("" : "+v"(voff), "+v"(voff8));
#endif
      const int nbp = 2;              // bytes: B pieces per wave of its bf16 half
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = wu * 4 + r;
        glds16(Xk0 + (int64_t)(a0 + q * 8) * cs * 2 + voff, &lds[st][0][q * 8 * GK]);
        if (!BYTES && haveB)
          glds16(Xk0 + (int64_t)(b0 + q * 8) * cs * 2 + voff, &lds[st][1][q * 8 * GK]);
      }
      if constexpr (BYTES) {
#pragma unroll
        for (int r = 0; r < nbp; ++r) {
          const int q = wu * 2 + r;
          glds16(Xk0 + (int64_t)(b0 + q * 8) * cs * 2 + voff, &lds[st][1][q * 8 * GK]);
        }
        if constexpr (BITS) {
          // the stage's 1 KB of bits, verbatim (voff8 = 16 * lane): one piece, wave 0
          if (wu == 0)
            glds16((gptr_t) reinterpret_cast<const char*>(X8) + (i0 >> 6) * 1024 + voff8,
                   &lds[st][1][128 * GK]);
        } else {
          glds16((gptr_t) reinterpret_cast<const char*>(X8) + (i0 >> 6) * (128 * GK) + wu * 1024 + voff8,
                 reinterpret_cast<bf16_t*>(reinterpret_cast<uint8_t*>(&lds[st][1][128 * GK]) +
                                           wu * 1024));
        }
      }
      return;
    }
    if constexpr (BITS) {
      const bf16_t* Xk0 = X + (i0 >> 6) * bs;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = wid * 4 + r;
        const int col = q * 8 + (lane >> 3);
        const int cc = (lane & 7) ^ (col & 7);
        glds16(Xk0 + cc * 8 + (int64_t)(a0 + col) * cs, &lds[st][0][q * 8 * GK]);
      }
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int q = wid * 2 + r;
        const int col = q * 8 + (lane >> 3);
        const int cc = (lane & 7) ^ (col & 7);
        glds16(Xk0 + cc * 8 + (int64_t)(b0 + col) * cs, &lds[st][1][q * 8 * GK]);
      }
      if (wu == 0) glds16(X8 + (i0 >> 6) * 1024 + lane * 16, &lds[st][1][128 * GK]);
      return;
    }
    if constexpr (BYTES) {
      // A: 32 pieces of 8 bf16 columns (4 per wave); B: 16 pieces of its bf16 half (2 per
      // wave) and 8 pieces of 16 byte columns (1 per wave)
      const bf16_t* Xk0 = X + (i0 >> 6) * bs;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = wid * 4 + r;
        const int col = q * 8 + (lane >> 3);
        const int cc = (lane & 7) ^ (col & 7);
        glds16(Xk0 + cc * 8 + (int64_t)(a0 + col) * cs, &lds[st][0][q * 8 * GK]);
      }
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int q = wid * 2 + r;
        const int col = q * 8 + (lane >> 3);
        const int cc = (lane & 7) ^ (col & 7);
        glds16(Xk0 + cc * 8 + (int64_t)(b0 + col) * cs, &lds[st][1][q * 8 * GK]);
      }
      const int cb = wid * 16 + (lane >> 2);                  // byte column 0..127
      const int pc = (lane & 3) ^ ((cb >> 1) & 2);             // its 16-byte piece this lane moves
      glds16(X8 + (i0 >> 6) * (128 * GK) + cb * GK + pc * 16,
             reinterpret_cast<bf16_t*>(reinterpret_cast<uint8_t*>(&lds[st][1][128 * GK]) +
                                       wid * 1024));
      return;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = wid * 4 + r;
      const int col = q * 8 + (lane >> 3);
      const int cc = (lane & 7) ^ (col & 7);
      const bf16_t* Xk = X + (i0 >> 6) * bs + cc * 8;      // i0: multiple of GK = 64
      glds16(Xk + (int64_t)(a0 + col) * cs, &lds[st][0][q * 8 * GK]);
      if (haveB) glds16(Xk + (int64_t)(b0 + col) * cs, &lds[st][1][q * 8 * GK]);
    }
  };
  auto frag = [&](const bf16_t* P_, int col, int cc) {
    return *reinterpret_cast<const bf16x8*>(&P_[col * GK + ((cc ^ (col & 7)) << 3)]);
  };
  // a byte column's raw fragments (image column col >= 128: byte column col - 128): both
  // halves of the stage for lane l, rows 8r..8r+7 (.xy) and 32+8r..32+8r+7 (.zw), r = l >> 4.
  // (Round 6 first read each half with its own ds_read_b64 from a 16-row-chunk layout; the
  // compiler paired those into ds_read2st64_b64, which banks mod 32 over 16 lanes: 4e7
  // conflict cycles per launch, profiles/r06_pmc.)
  auto raw16 = [&](const bf16_t* P_, int col) {
    const int cb = col - 128;
    const uint8_t* b8 = reinterpret_cast<const uint8_t*>(P_ + 128 * GK);
    const int slot = (lane >> 4) ^ ((cb >> 1) & 2);
    return *reinterpret_cast<const uint4*>(b8 + cb * GK + slot * 16);
  };
  // bit columns: the lane's replicated halfwords of the four column blocks from image column
  // col0 (128 or 192: plane 0 or 1), one ds_read_b64
  auto bits4 = [&](const bf16_t* P_, int col0, uint32_t* w) {
    const uint8_t* b1 = reinterpret_cast<const uint8_t*>(P_ + 128 * GK);
    const uint2 q = *reinterpret_cast<const uint2*>(b1 + ((col0 - 128) >> 6) * 512 + lane * 8);
    w[0] = bits_rep<0>(q.x);
    w[1] = bits_rep<1>(q.x);
    w[2] = bits_rep<0>(q.y);
    w[3] = bits_rep<1>(q.y);
  };
  const int64_t nsteps = (ch.row1 - ch.row0) / GK;
  if (nsteps > 0) stage(0, ch.row0);
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
  __syncthreads();
  // LATE: half 1 of the stage before (zeros ahead of stage 0: they add +0 to the +0 sums)
  bf16x8 ha[LATE ? 8 : 1], hb[LATE && !TRI ? 4 : 1];
  if constexpr (LATE) {
#pragma unroll
    for (int m = 0; m < 8; ++m) ha[m] = bf16x8{};
    if constexpr (!TRI) {
#pragma unroll
      for (int n = 0; n < 4; ++n) hb[n] = bf16x8{};
    }
  }
  for (int64_t s = 0; s < nsteps; ++s) {
    const int cur = s & 1;
    const bf16_t* As = lds[cur][abuf];
    const bf16_t* Bs = lds[cur][bbuf];
    if constexpr (LATE) {
      // half 1 of stage s-1 from registers beside the reads of half 0 of stage s ...
      bf16x8 na[8], nb[TRI ? 1 : 4];
      uint4 raw[BY && !BITS ? (TRI ? 8 : 4) : 1];
      uint32_t bw[BY && BITS ? (TRI ? 8 : 4) : 1];
      const int c0 = lane >> 4, c1 = 4 + (lane >> 4);
      if (!idle) {
        if constexpr (BY && BITS && !TRI) {
          bits4(Bs, bcol0, bw);
#pragma unroll
          for (int m = 0; m < 8; ++m) na[m] = frag(As, arow0 + m * 16 + (lane & 15), c0);
          // (the B halfwords stay packed until the second block)
          pair_mfma<MODE>(acc, ha, hb);
#pragma unroll
          for (int i = 0; i < 9; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          }
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);      // bits_rep
          __builtin_amdgcn_sched_group_barrier(0x008, NB - 10, 0);
        } else if constexpr (BY && BITS) {
          bits4(As, arow0, bw);
          bits4(As, arow0 + 64, bw + 4);
#pragma unroll
          for (int m = 0; m < 8; ++m) na[m] = bits_to_bf16x8<0>(bw[m]);
          pair_mfma<MODE>(acc, ha, ha);
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          }
#pragma unroll
          for (int i = 0; i < 32; ++i) {                          // bits_rep, then half 0
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
          }
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
          }
        } else if constexpr (BY && !TRI) {
#pragma unroll
          for (int n = 0; n < 4; ++n) raw[n] = raw16(Bs, bcol0 + n * 16 + (lane & 15));
#pragma unroll
          for (int m = 0; m < 8; ++m) na[m] = frag(As, arow0 + m * 16 + (lane & 15), c0);
          // (the raw B bytes stay raw until the second block: 16 registers fewer here)
          pair_mfma<MODE>(acc, ha, hb);
#pragma unroll
          for (int i = 0; i < 12; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          }
          __builtin_amdgcn_sched_group_barrier(0x008, NB - 12, 0);
        } else if constexpr (BY) {
#pragma unroll
          for (int m = 0; m < 8; ++m) raw[m] = raw16(As, arow0 + m * 16 + (lane & 15));
#pragma unroll
          for (int m = 0; m < 8; ++m) na[m] = bytes_to_bf16x8(make_uint2(raw[m].x, raw[m].y));
          pair_mfma<MODE>(acc, ha, ha);
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          }
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
          }
          __builtin_amdgcn_sched_group_barrier(0x008, NB - 24, 0);
        } else if constexpr (!TRI) {
#pragma unroll
          for (int m = 0; m < 8; ++m) na[m] = frag(As, arow0 + m * 16 + (lane & 15), c0);
#pragma unroll
          for (int n = 0; n < 4; ++n) nb[n] = frag(Bs, bcol0 + n * 16 + (lane & 15), c0);
          pair_mfma<MODE>(acc, ha, hb);
#pragma unroll
          for (int i = 0; i < 12; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          }
          __builtin_amdgcn_sched_group_barrier(0x008, NB - 12, 0);
        } else {
#pragma unroll
          for (int m = 0; m < 8; ++m) na[m] = frag(As, arow0 + m * 16 + (lane & 15), c0);
          pair_mfma<MODE>(acc, ha, ha);
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          }
          __builtin_amdgcn_sched_group_barrier(0x008, NB - 8, 0);
        }
      }
      // ... the copies of stage s+1 behind those MFMAs ...
      if (s + 1 < nsteps) stage(cur ^ 1, ch.row0 + (s + 1) * GK);
      // ... and half 0 of stage s beside the reads of its half 1 into the registers just freed
      if (!idle) {
        if constexpr (BY && BITS && !TRI) {
#pragma unroll
          for (int m = 0; m < 8; ++m) ha[m] = frag(As, arow0 + m * 16 + (lane & 15), c1);
#pragma unroll
          for (int n = 0; n < 4; ++n) nb[n] = bits_to_bf16x8<0>(bw[n]);
#pragma unroll
          for (int n = 0; n < 4; ++n) hb[n] = bits_to_bf16x8<1>(bw[n]);
          pair_mfma<MODE>(acc, na, nb);
          __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);      // B fragment 0 of half 0
#pragma unroll
          for (int i = 0; i < 3; ++i) {                           // fragments 1-3 beside the
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // first MFMAs
            __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
          }
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          }
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
          }
          __builtin_amdgcn_sched_group_barrier(0x008, NB - 27, 0);
        } else if constexpr (BY && BITS) {
#pragma unroll
          for (int m = 0; m < 8; ++m) ha[m] = bits_to_bf16x8<1>(bw[m]);
          pair_mfma<MODE>(acc, na, na);
#pragma unroll
          for (int i = 0; i < 32; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
          }
          __builtin_amdgcn_sched_group_barrier(0x008, NB - 32, 0);
        } else if constexpr (BY && !TRI) {
#pragma unroll
          for (int m = 0; m < 8; ++m) ha[m] = frag(As, arow0 + m * 16 + (lane & 15), c1);
#pragma unroll
          for (int n = 0; n < 4; ++n) nb[n] = bytes_to_bf16x8(make_uint2(raw[n].x, raw[n].y));
#pragma unroll
          for (int n = 0; n < 4; ++n) hb[n] = bytes_to_bf16x8(make_uint2(raw[n].z, raw[n].w));
          pair_mfma<MODE>(acc, na, nb);
          __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);      // B fragment 0 of half 0
#pragma unroll
          for (int i = 0; i < 3; ++i) {                           // fragments 1-3 beside the
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // first MFMAs
            __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
          }
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          }
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
          }
          __builtin_amdgcn_sched_group_barrier(0x008, NB - 27, 0);
        } else if constexpr (BY) {
#pragma unroll
          for (int m = 0; m < 8; ++m) ha[m] = bytes_to_bf16x8(make_uint2(raw[m].z, raw[m].w));
          pair_mfma<MODE>(acc, na, na);
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
          }
          __builtin_amdgcn_sched_group_barrier(0x008, NB - 16, 0);
        } else if constexpr (!TRI) {
#pragma unroll
          for (int m = 0; m < 8; ++m) ha[m] = frag(As, arow0 + m * 16 + (lane & 15), c1);
#pragma unroll
          for (int n = 0; n < 4; ++n) hb[n] = frag(Bs, bcol0 + n * 16 + (lane & 15), c1);
          pair_mfma<MODE>(acc, na, nb);
#pragma unroll
          for (int i = 0; i < 12; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          }
          __builtin_amdgcn_sched_group_barrier(0x008, NB - 12, 0);
        } else {
#pragma unroll
          for (int m = 0; m < 8; ++m) ha[m] = frag(As, arow0 + m * 16 + (lane & 15), c1);
          pair_mfma<MODE>(acc, na, na);
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          }
          __builtin_amdgcn_sched_group_barrier(0x008, NB - 8, 0);
        }
      }
    } else {
      if (s + 1 < nsteps) stage(cur ^ 1, ch.row0 + (s + 1) * GK);
      // every fragment of the stage (both 32-row halves) read from LDS up front, then the
      // MFMAs: the waits on LDS leave the MFMA chains of the stage
      if (!idle) {
        if constexpr (BY && BITS && !TRI) {
          // bit B fragments: one 8-byte read holds both halves' rows of the wave's 64 columns;
          // half 0 widened ahead of its MFMAs (while the A reads are in flight), half 1 beside
          // half 0's MFMAs
          bf16x8 af[2][8];
          uint32_t w4[4];
          bits4(Bs, bcol0, w4);
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            const int cc = kk * 4 + (lane >> 4);
#pragma unroll
            for (int m = 0; m < 8; ++m) af[kk][m] = frag(As, arow0 + m * 16 + (lane & 15), cc);
          }
          bf16x8 b0v[4], b1v[4];
#pragma unroll
          for (int n = 0; n < 4; ++n) b0v[n] = bits_to_bf16x8<0>(w4[n]);
#pragma unroll
          for (int n = 0; n < 4; ++n) b1v[n] = bits_to_bf16x8<1>(w4[n]);
          pair_mfma<MODE>(acc, af[0], b0v);
          pair_mfma<MODE>(acc, af[1], b1v);
          __builtin_amdgcn_sched_group_barrier(0x100, 9, 0);      // bits + A half 0
          __builtin_amdgcn_sched_group_barrier(0x002, 36, 0);     // bits_rep + half 0
#pragma unroll
          for (int i = 0; i < 8; ++i) {                           // A half 1 reads beside
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // half 0's MFMAs
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          }
#pragma unroll
          for (int i = 0; i < 16; ++i) {                          // half 1 widened beside
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // the next MFMAs
            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
          }
          __builtin_amdgcn_sched_group_barrier(0x008, 2 * NB - 24, 0);
        } else if constexpr (BY && BITS) {
          // bit triangle: block column n of a half needs fragments 0..n, so fragment n + 1 is
          // widened beside column n's MFMAs and half 1's fragment 0 beside half 0's last column
          uint32_t w8[8];
          bits4(As, arow0, w8);
          bits4(As, arow0 + 64, w8 + 4);
          bf16x8 f0[8], f1[8];
#pragma unroll
          for (int m = 0; m < 8; ++m) f0[m] = bits_to_bf16x8<0>(w8[m]);
#pragma unroll
          for (int m = 0; m < 8; ++m) f1[m] = bits_to_bf16x8<1>(w8[m]);
          pair_mfma<MODE, true>(acc, f0, f0);
          pair_mfma<MODE, true>(acc, f1, f1);
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, 16, 0);     // bits_rep + fragment 0
#define TRI_COL(C) sched_group<0x008, 1>(); sched_group<0x002, 8>(); sched_group<0x008, C>();
          TRI_COL(0) TRI_COL(1) TRI_COL(2) TRI_COL(3) TRI_COL(4) TRI_COL(5) TRI_COL(6) TRI_COL(7)
          TRI_COL(0) TRI_COL(1) TRI_COL(2) TRI_COL(3) TRI_COL(4) TRI_COL(5) TRI_COL(6)
#undef TRI_COL
          __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
        } else if constexpr (BY && !TRI) {
          // byte B fragments: one 16-byte read per column holds both halves' rows, converted
          // per half just ahead of its MFMAs; the second half's conversion interleaved with the
          // first half's MFMAs (mask 0x002 VALU)
          bf16x8 af[2][8];
          uint4 braw[4];
#pragma unroll
          for (int n = 0; n < 4; ++n) braw[n] = raw16(Bs, bcol0 + n * 16 + (lane & 15));
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            const int cc = kk * 4 + (lane >> 4);
#pragma unroll
            for (int m = 0; m < 8; ++m) af[kk][m] = frag(As, arow0 + m * 16 + (lane & 15), cc);
          }
          bf16x8 b0v[4], b1v[4];
#pragma unroll
          for (int n = 0; n < 4; ++n) b0v[n] = bytes_to_bf16x8(make_uint2(braw[n].x, braw[n].y));
#pragma unroll
          for (int n = 0; n < 4; ++n) b1v[n] = bytes_to_bf16x8(make_uint2(braw[n].z, braw[n].w));
          pair_mfma<MODE>(acc, af[0], b0v);
          pair_mfma<MODE>(acc, af[1], b1v);
          __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);     // B (both halves) + A half 0
          __builtin_amdgcn_sched_group_barrier(0x002, 16, 0);     // half 0 conversion
#pragma unroll
          for (int i = 0; i < 8; ++i) {                           // A half 1 reads beside
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // half 0's MFMAs
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          }
#pragma unroll
          for (int i = 0; i < 16; ++i) {                          // half 1 conversion beside
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // the next MFMAs
            __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
          }
          __builtin_amdgcn_sched_group_barrier(0x008, 2 * NB - 24, 0);
        } else if constexpr (BY) {
          uint4 fraw[8];
#pragma unroll
          for (int m = 0; m < 8; ++m) fraw[m] = raw16(As, arow0 + m * 16 + (lane & 15));
          bf16x8 f0[8], f1[8];
#pragma unroll
          for (int m = 0; m < 8; ++m) f0[m] = bytes_to_bf16x8(make_uint2(fraw[m].x, fraw[m].y));
#pragma unroll
          for (int m = 0; m < 8; ++m) f1[m] = bytes_to_bf16x8(make_uint2(fraw[m].z, fraw[m].w));
          pair_mfma<MODE>(acc, f0, f0);
          pair_mfma<MODE>(acc, f1, f1);
          __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);      // both halves' reads
          __builtin_amdgcn_sched_group_barrier(0x002, 32, 0);     // half 0 conversion
#pragma unroll
          for (int i = 0; i < 16; ++i) {                          // half 1 conversion beside
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // half 0's MFMAs
            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
          }
          __builtin_amdgcn_sched_group_barrier(0x008, 2 * NB - 16, 0);
        } else if constexpr (!TRI) {
          bf16x8 af[2][8], bfr[2][4];
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            const int cc = kk * 4 + (lane >> 4);
#pragma unroll
            for (int m = 0; m < 8; ++m) af[kk][m] = frag(As, arow0 + m * 16 + (lane & 15), cc);
#pragma unroll
            for (int n = 0; n < 4; ++n) bfr[kk][n] = frag(Bs, bcol0 + n * 16 + (lane & 15), cc);
          }
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) pair_mfma<MODE>(acc, af[kk], bfr[kk]);
          // schedule: the first half's 12 reads, then the second half's 12 reads one per
          // MFMA of the first half, then the remaining MFMAs (mask 0x100 DS read, 0x008 MFMA)
          __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);
#pragma unroll
          for (int i = 0; i < 12; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          }
          __builtin_amdgcn_sched_group_barrier(0x008, 2 * NB - 12, 0);
        } else {
          bf16x8 fr[2][8];
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            const int cc = kk * 4 + (lane >> 4);
#pragma unroll
            for (int m = 0; m < 8; ++m) fr[kk][m] = frag(As, arow0 + m * 16 + (lane & 15), cc);
          }
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) pair_mfma<MODE>(acc, fr[kk], fr[kk]);
          __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          }
          __builtin_amdgcn_sched_group_barrier(0x008, 2 * NB - 8, 0);
        }
      }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): next stage landed
    __syncthreads();
  }
  if constexpr (LATE) {
    if (!idle) pair_mfma<MODE>(acc, ha, TRI ? ha : hb);      // half 1 of the last stage
  }
  if (idle) return;
  // Slab block image is lane-major: float4 `lane` holds acc regs r = 0..3 = (row (l>>4)*4+r,
  // col l&15) of the 16x16 block, so each block is ONE 1-KB dwordx4 store per wave (4x fewer
  // store instructions than a row-major image; the epilogue is store-issue bound).
#pragma unroll
  for (int i = 0; i < NB; ++i)
    *reinterpret_cast<f32x4*>(out + i * 256 + lane * 4) = acc[i];
}

#ifdef GRAM_CLOCK
// profiling build (tools/enet_profile.py --build): per-workgroup shader clock cycles [0] and
// 100 MHz wall ticks [1] of the tile kernel, workgroups [2] (tools/enet_clock.py: the Gram's
// clock alone and beside the CV path kernel)
__device__ unsigned long long gram_clock[3];
extern "C" __attribute__((visibility("default"))) int ate_gram_clock_read(void* host) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(gram_clock), sizeof(gram_clock));
}
extern "C" __attribute__((visibility("default"))) int ate_gram_clock_reset() {
  static unsigned long long z[3];
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(gram_clock), z, sizeof(z));
}
#endif

// CM: the column mode (COL_*; X8 = the byte copy or the bit image of columns 384..511).
// SCHED: the K-loop schedule (SCHED_*). prio: s_setprio 1 for waves 4-7 (0 = none, 1 = every
// workgroup, 2 = diagonal-pair workgroups only; GRAM_PRIO).
template <int CM, int SCHED>
__global__ __launch_bounds__(512) void gram_bf16_pair_kernel(
    const bf16_t* __restrict__ X, int64_t cs, int64_t bs, const int4* __restrict__ tiles, int ntiles,
    const Chunk* __restrict__ chunks, int nchunks, float* __restrict__ slab,
    const uint8_t* __restrict__ X8, int prio) {
  __shared__ __attribute__((aligned(16))) bf16_t lds[PAIR_LDS];   // 128 KB
#ifdef GRAM_CLOCK
  const unsigned long long gc0 = clock64(), gw0 = wall_clock64();
#endif
  const int L = xcd_remap(blockIdx.x, gridDim.x);
  const int c = L / ntiles, t = L % ntiles;
  ATE_DASSERT(c < nchunks && t < ntiles);
  const Chunk ch = chunks[c];
  const int4 tl = tiles[t];
  const int type = tl.z;
  // row chunks are whole K-steps of one segment; tiles name 256-column blocks a <= b
  ATE_DASSERT(ch.row0 >= 0 && ch.row0 <= ch.row1 && ch.row0 % GK == 0 && ch.row1 % GK == 0);
  ATE_DASSERT(tl.x >= 0 && tl.y >= tl.x && type >= 0 && type <= 2);
  const bool haveB = type != 2;
  const int a0 = tl.x * GT, b0 = tl.y * GT;
  const int wid = threadIdx.x >> 6;
  const bool tri = type != 0 && wid >= 4;
  const int region = type == 0 ? 0 : (tri ? (wid - 4) >> 1 : wid >> 1);   // 0: tile a, 1: tile b
  const int half = type == 0 ? 0 : (wid & 1);
  const bool idle = type == 2 && region == 1;
  int arow0, bcol0;
  if (type == 0) { arow0 = (wid >> 2) * 128; bcol0 = (wid & 3) * 64; }
  else if (!tri) { arow0 = 0; bcol0 = 128 + half * 64; }
  else { arow0 = half * 128; bcol0 = half * 128; }
  const int abuf = type == 0 ? 0 : region;
  const int bbuf = type == 0 ? 1 : region;
  constexpr int RS = PairRole<PAIR_RECT_D0>::NB, TS = PairRole<PAIR_TRI>::NB;  // 32 / 36
  const int base = type == 0 ? wid * 32 : tri ? 4 * RS + (wid - 4) * TS : wid * RS;
  float* out = slab + ((int64_t)c * ntiles + t) * (PAIR_SLOTS * 256) + (int64_t)base * 256;
  // the second-dispatched half (waves 4-7: the triangle waves of a diagonal pair, the
  // heavier role) loses VALU / LDS issue arbitration to the older half on every stage;
  // one static priority raise for it (uniform branches: readfirstlane, type, prio)
  if ((prio == 1 || (prio == 2 && type != 0)) &&
      __builtin_amdgcn_readfirstlane(threadIdx.x) >= 256)
    __builtin_amdgcn_s_setprio(1);
  // byte fragments: tile b's columns 128..255 (type 0: the waves of B columns 128..255;
  // type 1, tile b: the rectangle waves' B and the second triangle)
  constexpr bool BYTES = CM != COL_BF16;
  const bool by = BYTES && (type == 0 ? (wid & 3) >= 2 : region == 1 && (!tri || half == 1));
  ATE_DASSERT(!BYTES || (X8 != nullptr && ntiles == 2 && b0 == 256));
  // waves 4-7 (the triangle waves of a diagonal pair, half of the rectangle waves of an
  // off-diagonal tile) are the late ones of the stagger schedule
  constexpr bool STAG = (SCHED & SCHED_STAGGER) != 0;
#define PAIR_WAVE(M, B, L) pair_wave<M, CM, B, L, SCHED != SCHED_LOCKSTEP>(                         \
      X, cs, bs, a0, b0, haveB, idle, abuf, bbuf, arow0, bcol0, ch, lds, out, X8)
#define PAIR_WAVE_BY(M, L) do { if (by) PAIR_WAVE(M, BYTES, L); else PAIR_WAVE(M, false, L); } while (0)
  if (tri) PAIR_WAVE_BY(PAIR_TRI, STAG);
  else if (type == 0) {
    if (STAG && __builtin_amdgcn_readfirstlane(wid) >= 4) PAIR_WAVE_BY(PAIR_RECT, STAG);
    else PAIR_WAVE_BY(PAIR_RECT, false);
  }
  else if (half == 0) PAIR_WAVE_BY(PAIR_RECT_D0, false);
  else PAIR_WAVE_BY(PAIR_RECT_D1, false);
#undef PAIR_WAVE_BY
#undef PAIR_WAVE
#ifdef GRAM_CLOCK
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(&gram_clock[0], (unsigned long long)(clock64() - gc0));
    atomicAdd(&gram_clock[1], (unsigned long long)(wall_clock64() - gw0));
    atomicAdd(&gram_clock[2], 1ull);
  }
#endif
}

// Exact (world-size-invariant) reduction: a chunk partial v is split into two int64 limbs
// of fixed scale, hi = floor(v 2^24), lo = rint((v 2^24 - hi) 2^32) (both exact in fp64),
// and the limbs of all chunks are summed as integers -- associative, so the rank that
// reduces a chunk and the all-reduce order cannot change a bit (ops/exact.py from_limbs).
__device__ __forceinline__ void gram_limbs(double v, long long& hi, long long& lo) {
  const double x = v * 16777216.0;                      // 2^24
  const double h = floor(x);
  hi = (long long)h;
  lo = (long long)rint((x - h) * 4294967296.0);         // 2^32
}

// blocks: [ntiles][PAIR_SLOTS] int2 (I, J) = 16-column block coordinates of the Gram (I: A
// side = row), (-1, -1) = unused slot. Blocks with I == J are full 16x16 diagonal blocks: only
// their r <= c entries are written (plus mirror), so every Gram entry has ONE writer.
// byte0: first one-byte or bit column, P when there are none. Their slab partials are exact
// power-of-two multiples (a one was 0.5 as a byte, 2.0 as a bit): scaled back by bsc = 2 or
// 0.5 per such column, exactly.
__global__ void gram_pair_reduce_kernel(const float* __restrict__ slab, const int2* __restrict__ blocks,
                                        int ntiles, int slots, const int* __restrict__ seg_chunk0,
                                        int nseg, int P, double* __restrict__ G,
                                        long long* __restrict__ Gx, int byte0, double bsc) {
  const int64_t per = (int64_t)ntiles * slots * 256;
  const int64_t total = (int64_t)nseg * per;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int s = (int)(e / per);
    const int64_t rem = e % per;
    const int tb = (int)(rem >> 8);                 // tile * slots + slot
    const int ln = (int)(rem & 255) >> 2;           // lane-major image (pair_wave epilogue)
    const int r = ((ln >> 4) << 2) | (int)(rem & 3), cl = ln & 15;
    const int2 bl = blocks[tb];
    if (bl.x < 0) continue;
    if (bl.x == bl.y && r > cl) continue;
    // fixed chunk order; 8 independent loads in flight per batch
    const int c0 = seg_chunk0[s], c1 = seg_chunk0[s + 1];
    const float* src = slab + rem;
    const int a = bl.x * 16 + r, b = bl.y * 16 + cl;
    ATE_DASSERT(s < nseg && c0 >= 0 && c0 <= c1 && a >= 0 && a < P && b >= 0 && b < P);
    const double sc = (a >= byte0 ? bsc : 1.0) * (b >= byte0 ? bsc : 1.0);
    if (Gx) {                                       // exact mode: int64 limbs
      long long hs = 0, ls = 0;
      int ci = c0;
      for (; ci + 8 <= c1; ci += 8) {               // 8 independent loads in flight
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(int64_t)(ci + u) * per];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          long long h, l;
          gram_limbs((double)v[u] * sc, h, l);
          hs += h;
          ls += l;
        }
      }
      for (; ci < c1; ++ci) {
        long long h, l;
        gram_limbs((double)src[(int64_t)ci * per] * sc, h, l);
        hs += h;
        ls += l;
      }
      const int64_t PP = (int64_t)nseg * P * P;
      long long* Xs = Gx + (int64_t)s * P * P;
      Xs[(int64_t)a * P + b] = hs;
      Xs[(int64_t)b * P + a] = hs;
      Xs[PP + (int64_t)a * P + b] = ls;
      Xs[PP + (int64_t)b * P + a] = ls;
      continue;
    }
    double acc = 0.0;
    int ci = c0;
    for (; ci + 8 <= c1; ci += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = src[(int64_t)(ci + u) * per];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += (double)v[u];
    }
    for (; ci < c1; ++ci) acc += (double)src[(int64_t)ci * per];
    acc *= sc;
    double* Gs = G + (int64_t)s * P * P;
    Gs[(int64_t)a * P + b] = acc;
    Gs[(int64_t)b * P + a] = acc;
  }
}

// the schedules built into the library (X-macro: registration and launch below)
#define PAIR_SCHEDS(F) F(0) F(1)
#define PAIR_SHAPE(S)                                                                     \
  static ate::KernelShapeReg ate_kshape_pair_##S(                                         \
      (const void*)(gram_bf16_pair_kernel<COL_BF16, S>), "gram_bf16_pair_kernel<sched " #S ">", 512, 0); \
  static ate::KernelShapeReg ate_kshape_pair8_##S(                                        \
      (const void*)(gram_bf16_pair_kernel<COL_BYTES, S>), "gram_bf16_pair_kernel<bytes, sched " #S ">", 512, 0); \
  static ate::KernelShapeReg ate_kshape_pair1_##S(                                        \
      (const void*)(gram_bf16_pair_kernel<COL_BITS, S>), "gram_bf16_pair_kernel<bits, sched " #S ">", 512, 0);
PAIR_SCHEDS(PAIR_SHAPE)
#undef PAIR_SHAPE
ATE_KERNEL_SHAPE("gram_bf16_256_kernel", 512, 0, gram_bf16_256_kernel)
ATE_KERNEL_SHAPE("gram_bf16_kernel", 256, 0, gram_bf16_kernel)

// cm: COL_*; X8: the one-byte copies (COL_BYTES) or the bit image (COL_BITS) of columns
// 384..511, null for COL_BF16
static int gram_pair(int cm, const void* X, int64_t cs, int64_t bs, int P, const void* tiles,
                     int ntiles, const void* blocks, const void* chunks, int nchunks,
                     const void* seg_chunk0, int nseg, void* slab, void* G, int what, void* Gx,
                     const void* X8, int sched, int prio, void* stream) {
  if (P % (2 * GT) || what < 1 || what > 3) return -1;
  if ((cm != COL_BF16) != (X8 != nullptr)) return -1;
  if (X8 != nullptr && (P != 512 || ntiles != 2)) return -1;
  // the other schedules address a piece's 8 columns with a 32-bit per-lane byte offset
  if (sched != SCHED_LOCKSTEP && cs >= ((int64_t)1 << 28)) return -1;
  // the priority raise was tuned for lockstep; with the stagger it measures as no gain
  // (profiles/gram_handoff: none 4.446, diagonal pairs 4.465, everywhere 4.476 ms per call)
  if (prio < 0) prio = sched == SCHED_STAGGER ? 0 : GRAM_PRIO;
  if (prio > 2) return -1;
  hipStream_t s = (hipStream_t)stream;
  if (what & 1) {
#define PAIR_LAUNCH_CM(C, S)                                                                  \
  ATE_LAUNCH((gram_bf16_pair_kernel<C, S>), dim3(nchunks * ntiles), dim3(512), 0, s,          \
             (const bf16_t*)X, cs, bs, (const int4*)tiles, ntiles, (const Chunk*)chunks,      \
             nchunks, (float*)slab, (const uint8_t*)X8, prio)
    switch (sched) {
#define PAIR_LAUNCH(S)                                                                        \
  case S:                                                                                     \
    if (cm == COL_BITS) PAIR_LAUNCH_CM(COL_BITS, S);                                          \
    else if (cm == COL_BYTES) PAIR_LAUNCH_CM(COL_BYTES, S);                                   \
    else PAIR_LAUNCH_CM(COL_BF16, S);                                                         \
    break;
      PAIR_SCHEDS(PAIR_LAUNCH)
#undef PAIR_LAUNCH
#undef PAIR_LAUNCH_CM
      default: return -1;   // a schedule this library was not built with
    }
    ATE_CHECK_LAUNCH();
  }
  if (what & 2) {
    const int64_t total = (int64_t)nseg * ntiles * PAIR_SLOTS * 256;
    ATE_LAUNCH(gram_pair_reduce_kernel, dim3(grid_for(total, 256, 4096)), dim3(256), 0, s,
                       (const float*)slab, (const int2*)blocks, ntiles, PAIR_SLOTS,
                       (const int*)seg_chunk0, nseg, P, (double*)G, (long long*)Gx,
                       X8 != nullptr ? PAIR_BYTE0 : P, cm == COL_BITS ? 0.5 : 2.0);
    ATE_CHECK_LAUNCH();
  }
  return 0;
}

// what: 1 = tile kernel (slab partials), 2 = fixed-order slab reduce into G, 3 = both.
// Split so a caller can run the reduce on another stream than the next tile kernel.
// X8: the one-byte copies of columns 384..511 (P == 512 only), or null.
ATE_API int ate_gram_bf16_pair(const void* X, int64_t cs, int64_t bs, int P, const void* tiles, int ntiles,
                               const void* blocks, const void* chunks, int nchunks,
                               const void* seg_chunk0, int nseg, void* slab, void* G, int what,
                               void* Gx, const void* X8, int sched, int prio, void* stream) {
  return gram_pair(X8 != nullptr ? COL_BYTES : COL_BF16, X, cs, bs, P, tiles, ntiles, blocks,
                   chunks, nchunks, seg_chunk0, nseg, slab, G, what, Gx, X8, sched, prio, stream);
}

// The same with columns 384..511 streamed from the panel's bit image X1 ([ld / 64][1024]
// bytes, csrc/dgp.hip ate_dgp_pack_bits): P == 512 only, X1 not null.
ATE_API int ate_gram_bf16_pair_bits(const void* X, int64_t cs, int64_t bs, int P, const void* tiles,
                                    int ntiles, const void* blocks, const void* chunks, int nchunks,
                                    const void* seg_chunk0, int nseg, void* slab, void* G, int what,
                                    void* Gx, const void* X1, int sched, int prio, void* stream) {
  if (X1 == nullptr) return -1;
  return gram_pair(COL_BITS, X, cs, bs, P, tiles, ntiles, blocks, chunks, nchunks, seg_chunk0,
                   nseg, slab, G, what, Gx, X1, sched, prio, stream);
}

// ------------------------------------------------------------------ fp32 / fp64 64x64
constexpr int FT = 64;
constexpr int FK = 16;

typedef __attribute__((ext_vector_type(4))) double f64x4;
template <typename T> struct AccT;
template <> struct AccT<float> { typedef f32x4 type; };
template <> struct AccT<double> { typedef f64x4 type; };

__device__ __forceinline__ f32x4 mfma_16x16x4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f64x4 mfma_16x16x4(double a, double b, f64x4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
// C/D row of accumulator register r: f32 16x16x4 -> (l>>4)*4+r ; f64 16x16x4 -> (l>>4)+4r
__device__ __forceinline__ int acc_row(float, int lane, int r) { return (lane >> 4) * 4 + r; }
__device__ __forceinline__ int acc_row(double, int lane, int r) { return (lane >> 4) + 4 * r; }

template <typename T>
__global__ __launch_bounds__(256) void gram_small_kernel(
    const T* __restrict__ X, int64_t ld, const T* __restrict__ w,
    const int2* __restrict__ tiles, int ntiles, const Chunk* __restrict__ chunks, int nchunks,
    T* __restrict__ slab, const int* __restrict__ done) {
  if (done && *done) return;
  typedef typename AccT<T>::type acc_t;
  __shared__ T lds[2][FT * (FK + 1)];   // [A/B][col*(FK+1)+row], +1 pad vs bank conflicts
  const int L = xcd_remap(blockIdx.x, gridDim.x);
  const int c = L / ntiles, t = L % ntiles;
  const Chunk ch = chunks[c];
  const int2 tl = tiles[t];
  const int a0 = tl.x * FT, b0 = tl.y * FT;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  acc_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = acc_t{0, 0, 0, 0};

  for (int64_t i0 = ch.row0; i0 < ch.row1; i0 += FK) {
    // stage 64 cols x 16 rows for A (row-weighted) and B: 1024 values each, 4 per thread
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int idx = r * 256 + tid, col = idx >> 4, row = idx & 15;
      int64_t gi = i0 + row;
      T wv = w ? w[gi] : T(1);
      lds[0][col * (FK + 1) + row] = X[(int64_t)(a0 + col) * ld + gi] * wv;
      lds[1][col * (FK + 1) + row] = X[(int64_t)(b0 + col) * ld + gi];
    }
    __syncthreads();
#pragma unroll
    for (int k4 = 0; k4 < FK; k4 += 4) {
      T af[2], bfv[2];
#pragma unroll
      for (int m = 0; m < 2; ++m)
        af[m] = lds[0][(wr * 32 + m * 16 + (lane & 15)) * (FK + 1) + k4 + (lane >> 4)];
#pragma unroll
      for (int n = 0; n < 2; ++n)
        bfv[n] = lds[1][(wc * 32 + n * 16 + (lane & 15)) * (FK + 1) + k4 + (lane >> 4)];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = mfma_16x16x4(af[m], bfv[n], acc[m][n]);
    }
    __syncthreads();
  }
  T* out = slab + ((int64_t)c * ntiles + t) * (FT * FT);
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = wr * 32 + m * 16 + acc_row(T(0), lane, r);
        int col = wc * 32 + n * 16 + (lane & 15);
        out[row * FT + col] = acc[m][n][r];
      }
}

// ------------------------------------------------------------------ slab reduce (fp64, fixed order)
template <typename S>
__global__ void gram_reduce_kernel(const S* __restrict__ slab, int T, const int2* __restrict__ tiles,
                                   int ntiles, const int* __restrict__ seg_chunk0, int nseg, int P,
                                   double* __restrict__ G, const int* __restrict__ done,
                                   long long* __restrict__ Gx) {
  if (done && *done) return;
  const int tt = T * T;
  const int64_t total = (int64_t)nseg * ntiles * tt;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    int s = (int)(e / ((int64_t)ntiles * tt));
    int rem = (int)(e % ((int64_t)ntiles * tt));
    int t = rem / tt, ij = rem % tt;
    // diagonal tiles: only the upper entry of each (i, j) / (j, i) pair is reduced and it
    // writes both G[a][b] and G[b][a] -- ONE writer per Gram entry. (With row weights the
    // tile's (i, j) and (j, i) partials round differently, (x_i w) x_j vs (x_j w) x_i, and
    // two writers made the weighted Gram differ run to run at rounding level.)
    if (tiles[t].x == tiles[t].y && ij / T > ij % T) continue;
    if (Gx) {                                       // exact mode: int64 limbs
      long long hs = 0, ls = 0;
      for (int c = seg_chunk0[s]; c < seg_chunk0[s + 1]; ++c) {
        long long h, l;
        gram_limbs((double)slab[((int64_t)c * ntiles + t) * tt + ij], h, l);
        hs += h;
        ls += l;
      }
      const int a = tiles[t].x * T + ij / T, b = tiles[t].y * T + ij % T;
      const int64_t PP = (int64_t)nseg * P * P;
      long long* Xs = Gx + (int64_t)s * P * P;
      Xs[(int64_t)a * P + b] = hs;
      Xs[(int64_t)b * P + a] = hs;
      Xs[PP + (int64_t)a * P + b] = ls;
      Xs[PP + (int64_t)b * P + a] = ls;
      continue;
    }
    double acc = 0.0;
    for (int c = seg_chunk0[s]; c < seg_chunk0[s + 1]; ++c)
      acc += (double)slab[((int64_t)c * ntiles + t) * tt + ij];
    int a = tiles[t].x * T + ij / T, b = tiles[t].y * T + ij % T;
    double* Gs = G + (int64_t)s * P * P;
    Gs[(int64_t)a * P + b] = acc;
    Gs[(int64_t)b * P + a] = acc;
  }
}

// ------------------------------------------------------------------ host API
// chunks/tiles/seg_chunk0 are device arrays prepared by the caller (ops/gram.py).
// tile = 128 (4 waves, register-staged) or 256 (8 waves, LDS-DMA staged); the caller's
// tile table and chunk plan must use the same tile size.
ATE_API int ate_gram_bf16(const void* X, int64_t ld, int P, int tile,
                          const void* tiles, int ntiles, const void* chunks, int nchunks,
                          const void* seg_chunk0, int nseg, void* slab, void* G, void* Gx,
                          void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int nwg = nchunks * ntiles;
  if (tile == GT) {
    if (P % GT) return -1;
    ATE_LAUNCH(gram_bf16_256_kernel, dim3(nwg), dim3(512), 0, s, (const bf16_t*)X, ld,
                       (const int2*)tiles, ntiles, (const Chunk*)chunks, nchunks, (float*)slab);
  } else if (tile == BT) {
    if (P % BT) return -1;
    ATE_LAUNCH(gram_bf16_kernel, dim3(nwg), dim3(256), 0, s, (const bf16_t*)X, ld,
                       (const int2*)tiles, ntiles, (const Chunk*)chunks, nchunks, (float*)slab);
  } else {
    return -1;
  }
  ATE_CHECK_LAUNCH();
  int64_t total = (int64_t)nseg * ntiles * tile * tile;
  ATE_LAUNCH(gram_reduce_kernel<float>, dim3(grid_for(total, 256, 4096)), dim3(256), 0, s,
                     (const float*)slab, tile, (const int2*)tiles, ntiles, (const int*)seg_chunk0,
                     nseg, P, (double*)G, (const int*)nullptr, (long long*)Gx);
  ATE_CHECK_LAUNCH();
  return 0;
}

template <typename T>
static int gram_small(const void* X, int64_t ld, int P, const void* w, const void* tiles,
                      int ntiles, const void* chunks, int nchunks, const void* seg_chunk0,
                      int nseg, void* slab, void* G, const void* done, void* Gx, void* stream) {
  if (P % FT) return -1;
  hipStream_t s = (hipStream_t)stream;
  int nwg = nchunks * ntiles;
  ATE_LAUNCH(gram_small_kernel<T>, dim3(nwg), dim3(256), 0, s, (const T*)X, ld,
                     (const T*)w, (const int2*)tiles, ntiles, (const Chunk*)chunks, nchunks,
                     (T*)slab, (const int*)done);
  ATE_CHECK_LAUNCH();
  int64_t total = (int64_t)nseg * ntiles * FT * FT;
  ATE_LAUNCH(gram_reduce_kernel<T>, dim3(grid_for(total, 256, 4096)), dim3(256), 0, s,
                     (const T*)slab, FT, (const int2*)tiles, ntiles, (const int*)seg_chunk0,
                     nseg, P, (double*)G, (const int*)done, (long long*)Gx);
  ATE_CHECK_LAUNCH();
  return 0;
}

ATE_API int ate_gram_f32(const void* X, int64_t ld, int P, const void* w, const void* tiles,
                         int ntiles, const void* chunks, int nchunks, const void* seg_chunk0,
                         int nseg, void* slab, void* G, const void* done, void* Gx, void* stream) {
  return gram_small<float>(X, ld, P, w, tiles, ntiles, chunks, nchunks, seg_chunk0, nseg, slab, G,
                        done, Gx, stream);
}

ATE_API int ate_gram_f64(const void* X, int64_t ld, int P, const void* w, const void* tiles,
                         int ntiles, const void* chunks, int nchunks, const void* seg_chunk0,
                         int nseg, void* slab, void* G, const void* done, void* Gx, void* stream) {
  return gram_small<double>(X, ld, P, w, tiles, ntiles, chunks, nchunks, seg_chunk0, nseg, slab, G,
                        done, Gx, stream);
}

ATE_API int ate_gram_tile_sizes(int* bf16_tile, int* bf16_kstep, int* f32_tile, int* f32_kstep) {
  *bf16_tile = BT; *bf16_kstep = BK; *f32_tile = FT; *f32_kstep = FK;
  return 0;
}
