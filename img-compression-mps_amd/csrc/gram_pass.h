// One Gram orthonormalisation pass of a sketched bond, shared by the sketch of the elementwise product (hadamard.hip)
// and the sketch of a sum (sumsketch.hip): the only definition of the pass and of its floor.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"

namespace ndmps {

constexpr double kSketchFloor = 1e-7;  // SKETCH_FLOOR of core/hadamard.py

// what a pass needs of the caller's workspace: G, V (l x l each), w (l) and the eigen-solver's workspace of `eig` bytes
struct GramPassWs {
  double *G = nullptr, *V = nullptr, *w = nullptr;
  char* ev = nullptr;
  int64_t eig = 0;
};

// Q (rows x r, row-major) columns divided by sqrt(w), in place
static __global__ void __launch_bounds__(256) cols_over_sqrt_kernel(double* __restrict__ Q, int64_t rows, int64_t r,
                                                                    const double* __restrict__ w) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < rows * r; e += (int64_t)gridDim.x * 256)
    Q[e] /= sqrt(w[e % r]);
}

// One Gram orthonormalisation pass of S (rows x l, row-major): G = S^T S = V diag(w) V^T, kept r = #{sqrt(w_j) >
// kSketchFloor sqrt(w_0)} (0 when w_0 <= 0), Q (rows x r) = S V_r diag(1 / sqrt(w)).  hw: at least l host doubles.
// Synchronises the stream.
static inline int gram_pass(const GramPassWs& b, const double* S, int64_t rows, int64_t l, double* Q, int64_t* r_out,
                            std::vector<double>& hw, hipStream_t s) {
  NDMPS_TRY(ndmps_dgemm(1, 0, l, l, rows, S, l, S, l, b.G, l, s));
  NDMPS_TRY(ndmps_syevj_f64(b.G, l, b.V, b.w, b.ev, b.eig, nullptr, s));
  NDMPS_CHECK_HIP(hipMemcpyAsync(hw.data(), b.w, l * sizeof(double), hipMemcpyDeviceToHost, s));
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));
  *r_out = 0;
  if (!(hw[0] > 0.0)) return NDMPS_OK;
  const double s0 = std::sqrt(hw[0]);
  int64_t r = 0;
  while (r < l && hw[r] > 0.0 && std::sqrt(hw[r]) > kSketchFloor * s0) ++r;
  r = std::min(r, rows);
  NDMPS_TRY(ndmps_dgemm(0, 0, rows, r, l, S, l, b.V, l, Q, r, s));
  hipLaunchKernelGGL(cols_over_sqrt_kernel, dim3(grid1d(rows * r)), dim3(256), 0, s, Q, rows, r, b.w);
  NDMPS_LAUNCH_CHECK();
  *r_out = r;
  return NDMPS_OK;
}

}  // namespace ndmps
