// What the sketch of the elementwise product (hadamard.hip) and the sketch of a sum (sumsketch.hip) share on the host:
// the only definition of the layout of a sketched chain, of one Gram orthonormalisation pass of a sketched bond, of
// its floor and of its pieces of the workspace.
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
// its carve for passes of order <= lmax, in the order G, V, w, ev
static inline GramPassWs carve_gram_pass(Arena& ar, int64_t lmax, int64_t eig) {
  GramPassWs g;
  g.G = ar.take<double>(lmax * lmax);
  g.V = ar.take<double>(lmax * lmax);
  g.w = ar.take<double>(lmax);
  g.ev = ar.take<char>(std::max<int64_t>(eig, 1));
  g.eig = eig;
  return g;
}

// The layout of a sketched chain: site k of the output holds at most ell[k] dims[k] ell[k+1] doubles at out_off[k], and
// the random cores R have the same layout.
struct SketchLayout {
  std::vector<int64_t> dims, ell, out_off;  // dims and ell: assigned and checked by the caller
  int64_t lmax = 1, sq = 1, r_elems = 0, eig = 0;  // largest sketch bond, largest site, all sites, the eigen-solver's bytes
};
static inline int fill_sketch_layout(SketchLayout& s) {
  const int L = (int)s.dims.size();
  s.lmax = *std::max_element(s.ell.begin(), s.ell.end());
  s.out_off.assign(L + 1, 0);
  for (int k = 0; k < L; ++k) {
    const int64_t cap = s.ell[k] * s.dims[k] * s.ell[k + 1];
    s.out_off[k + 1] = s.out_off[k] + cap;
    s.sq = std::max(s.sq, cap);
  }
  s.r_elems = s.out_off[L];
  s.eig = ndmps_syevj_workspace_bytes(s.lmax);
  NDMPS_REQUIRE(s.eig >= 0, "internal: eigen-solver workspace");
  return NDMPS_OK;
}
// the caller's random cores: as many as the layout says (they are copied once the workspace is known to fit)
static inline int check_sketch_cores(const SketchLayout& s, int64_t r_len) {
  NDMPS_REQUIRE(r_len == s.r_elems, "the sketch cores have %lld elements, expected %lld", (long long)r_len, (long long)s.r_elems);
  return NDMPS_OK;
}

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
