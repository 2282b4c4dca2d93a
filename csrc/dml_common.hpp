// DML score arithmetic shared by the stand-alone kernels (csrc/stats.hip) and the fused
// residual pass (csrc/dml.hip): one definition, so both chains give the same bits.
#pragma once
#include "common.hpp"

namespace ate {

// m[7] = {S_wy, S_ww, S_yyww, S_yw3, S_w4, n, S_yy} -> res = {theta, se}.
// mode 0 (PLR, Neyman score): theta = S_wy/S_ww, psi = (yr - theta wr) wr,
//   se = sqrt(mean(psi^2)/J^2/n), J = S_ww/n.
// mode 1 (reference lm(Y_resid ~ 0 + W_resid), ate_functions.R:363-366):
//   se = sqrt(RSS/(n-1)/S_ww).
__device__ __forceinline__ void dml_finalize_formula(const double* m, int mode, double* res) {
  double n = m[5];
  double theta = m[0] / m[1];
  double se;
  if (mode == 0) {
    double j = m[1] / n;
    double psi2 = (m[2] - 2.0 * theta * m[3] + theta * theta * m[4]) / n;
    se = sqrt(fmax(psi2, 0.0) / (j * j) / n);
  } else {
    double rss = m[6] - 2.0 * theta * m[0] + theta * theta * m[1];
    se = sqrt(fmax(rss, 0.0) / (n - 1.0) / m[1]);
  }
  res[0] = theta;
  res[1] = se;
}

// 256 threads: thread i sums partials i, i+256, ... (fixed order), then a fixed-shape block
// reduction -> deterministic for a given launch geometry. Result valid in thread 0.
__device__ __forceinline__ void sum7_block(const double* partial, int nb, double (&v)[7],
                                           double* red /* >= 16*7 */) {
  for (int b = threadIdx.x; b < nb; b += 256)
#pragma unroll
    for (int q = 0; q < 7; ++q) v[q] += partial[(int64_t)b * 7 + q];
  block_sum<7>(v, red);
}

}  // namespace ate
