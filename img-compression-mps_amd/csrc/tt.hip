// MPS composites: the SVD sweep and bond truncation.
//
//   ndmps_tt_sweep_f32        <- quimb MatrixProductState.from_dense   (core/ndmps.py:74)
//   ndmps_compress_bond_f32   <- quimb tensor_compress_bond            (core/ndmps.py:104-106)
//
// SVD strategy (per site, unfolding A of m rows x n cols, fp32 in HBM):
//   n <= m : G = A^T A in fp64 (exact products), G = V diag(w) V^T by Jacobi; sigma = sqrt(w);
//            site core = V_k^T (k x n), carry = A V_k (m x k, fp32 MFMA GEMM).
//   n >  m : G = A A^T in fp64, G = U diag(w) U^T; carry = U_k diag(sigma_k),
//            core = diag(1/sigma_k) U_k^T A (fp64 GEMM, then fp32).
// The carried matrix is exact whatever the accuracy of sigma (it is an orthogonal projection
// of the data); sigma is accurate to ~1e-8 sigma_0 (fp64 Gram of fp32 data).  Singular values
// below kCutoffFloor * sigma_0 are representation noise of fp32 input and are dropped even
// when the caller's cutoff is smaller (the reference's 1e-10 presumes fp64 data).
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "trunc.h"
#include "typed.h"

namespace {

constexpr double kCutoffFloor = 1e-6;
// fp64 storage: the Gram route resolves singular values down to ~sqrt(eps) s_0
constexpr double kCutoffFloorF64 = 1e-8;
template <typename T>
constexpr double cutoff_floor() { return sizeof(T) == 8 ? kCutoffFloorF64 : kCutoffFloor; }
// Jacobi convergence threshold of the sweep's eigenproblems, relative to the largest eigenvalue.
// The data is fp32: off-diagonal couplings below 1e-13 lambda_0 move the kept subspace by less than
// fp32 rounding even inside a noise-floor cluster (gaps ~1e-9 lambda_0); override for experiments with
// NDMPS_SWEEP_EIG_TOL.
constexpr double kSweepEigTol = 1e-13;

inline double sweep_eig_tol(bool f64_storage = false) {
  const char* e = getenv("NDMPS_SWEEP_EIG_TOL");
  if (e) {
    const double v = atof(e);
    if (v >= 1e-16 && v <= 1e-6) return v;
  }
  return f64_storage ? 1e-15 : kSweepEigTol;  // fp64 data: iterate down to the rounding of the Gram matrix
}

using ndmps::Arena;
using ndmps::ceil_div;
using ndmps::gram_ws_bound;

// ----------------------------------------------------------------------------- small kernels
// |A v_j|^2 for the eigenvectors v_j = V[:, i0 + j], j < t, of a Gram matrix of A: the singular values behind the SMALLEST
// eigenvalues, which the eigenvalues themselves resolve only to ~1e-15 |G| (3e-8 of the largest singular value).
// A(r, c) = A[r rs + c cs] (rs = n, cs = 1 for G = A^T A; the transposed strides for G = A A^T).  Thread (row, j):
// 4 rows x 64 columns per workgroup, row blocks strided by the grid (one row per thread when gridDim.x covers the
// rows); partial[blockIdx.x][j] = sum over the workgroup's rows; tail_norm_reduce_kernel adds the row blocks in fixed
// order.
template <typename T>
__global__ void __launch_bounds__(256)
tail_norm_partial_kernel(const T* __restrict__ A, int64_t rs, int64_t cs, int rows, int cols, const double* __restrict__ V,
                         int ldv, int i0, int t, double* __restrict__ partial) {
  __shared__ double red[4][64];
  const int jl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int j = blockIdx.y * 64 + jl;
  double acc = 0.0;
  for (int r = blockIdx.x * 4 + rl; r < rows && j < t; r += gridDim.x * 4) {
    const T* a = A + (int64_t)r * rs;
    const double* v = V + i0 + j;
    double y = 0.0;
    for (int c = 0; c < cols; ++c) y = fma(ndmps::to_f64(a[(int64_t)c * cs]), v[(int64_t)c * ldv], y);
    acc += y * y;
  }
  red[rl][jl] = acc;
  __syncthreads();
  if (rl == 0 && j < t) partial[(int64_t)blockIdx.x * t + j] = (red[0][jl] + red[1][jl]) + (red[2][jl] + red[3][jl]);
}
__global__ void tail_norm_reduce_kernel(const double* __restrict__ partial, int nblk, int t, double* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= t) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += partial[(int64_t)b * t + j];
  out[j] = s;
}
// Both launches: *sums <- the device pointer of the t values |A v_j|^2.  Partials (nblk x t) and sums (t) live in `scratch`
// (scratch_elems doubles): nblk = ceil(rows / 4) row blocks where they fit, else fewer blocks of more rows each (a tall
// unfolding, e.g. 4096 rows of order 8 in an order-64 layout).
template <typename T>
int tail_norms(const T* A, int64_t rs, int64_t cs, int64_t rows, int64_t cols, const double* V, int64_t ldv, int64_t i0,
               int64_t t, double* scratch, int64_t scratch_elems, double** sums, hipStream_t s) {
  int nblk = (int)ceil_div(rows, 4);
  if ((int64_t)nblk * t + t > scratch_elems) nblk = (int)((scratch_elems - t) / t);
  NDMPS_REQUIRE(nblk >= 1 && (int64_t)nblk * t + t <= scratch_elems, "internal: no room for the tail norms (%lld x %lld)",
                (long long)nblk, (long long)t);
  *sums = scratch + (int64_t)nblk * t;
  hipLaunchKernelGGL(tail_norm_partial_kernel<T>, dim3((unsigned)nblk, (unsigned)ceil_div(t, 64)), dim3(256), 0, s, A, rs, cs,
                     (int)rows, (int)cols, V, (int)ldv, (int)i0, (int)t, scratch);
  hipLaunchKernelGGL(tail_norm_reduce_kernel, dim3((unsigned)ceil_div(t, 256)), dim3(256), 0, s, scratch, nblk, (int)t, *sums);
  NDMPS_LAUNCH_CHECK();
  return NDMPS_OK;
}

// ---- elementwise bodies: each is shared by a per-volume kernel and by its `_batched` twin, which resolves the volume's
//      pointers from blockIdx.y first (f32_to_f64_body and its per-volume kernel: typed.h)
// core (k x n) <- first k columns of V (n x n fp64), transposed.  rank_r (device, may be null): the rank of the right
// bond where the sweep decides its ranks on the device and n = d x cap_r is laid out for the cap; the columns behind
// that rank are rows and columns of zeros in the Gram matrix, where the solver's vectors carry rounding noise: the
// padded core gets the exact zeros it is documented to hold.
template <typename T>
__device__ __forceinline__ void core_from_vectors_body(const double* __restrict__ V, int64_t n, int64_t k, T* __restrict__ core,
                                                       const int* __restrict__ rank_r, int64_t cap_r) {
  const int64_t total = k * n;
  const int64_t kr = rank_r ? (int64_t)*rank_r : cap_r;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / n, c = e % n;
    core[e] = ndmps::from_f64<T>(c % cap_r < kr ? V[c * n + i] : 0.0);
  }
}
// s <- sqrt(max(w, 0))
__device__ __forceinline__ void sqrt_clamp_body(const double* __restrict__ w, int64_t n, double* __restrict__ s) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) s[i] = sqrt(fmax(w[i], 0.0));
}
// out (rows x k) <- M (rows x ldm fp64)[:, :k] * sigma[col]^power
template <typename T>
__device__ __forceinline__ void scale_cols_body(const double* __restrict__ M, int64_t rows, int64_t ldm, int64_t k,
                                                const double* __restrict__ sigma, double power, T* __restrict__ out) {
  const int64_t total = rows * k;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / k, c = e % k;
    const double sg = sigma[c];
    out[e] = ndmps::from_f64<T>(sg > 0.0 ? M[r * ldm + c] * pow(sg, power) : 0.0);
  }
}
// out (k x n) <- M (k x n fp64) with row i scaled by sigma[i]^power
template <typename T>
__device__ __forceinline__ void scale_rows_body(const double* __restrict__ M, int64_t k, int64_t n,
                                                const double* __restrict__ sigma, double power, T* __restrict__ out) {
  const int64_t total = k * n;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const double sg = sigma[e / n];
    out[e] = ndmps::from_f64<T>(sg > 0.0 ? M[e] * pow(sg, power) : 0.0);
  }
}

template <typename T>
__global__ void __launch_bounds__(256)
core_from_vectors_kernel(const double* __restrict__ V, int64_t n, int64_t k, T* __restrict__ core,
                         const int* __restrict__ rank_r, int64_t cap_r) {
  core_from_vectors_body(V, n, k, core, rank_r, cap_r);
}
template <typename T>
__global__ void __launch_bounds__(256)
scale_cols_to_f32_kernel(const double* __restrict__ M, int64_t rows, int64_t ldm, int64_t k,
                         const double* __restrict__ sigma, double power, T* __restrict__ out) {
  scale_cols_body(M, rows, ldm, k, sigma, power, out);
}
template <typename T>
__global__ void __launch_bounds__(256)
scale_rows_to_f32_kernel(const double* __restrict__ M, int64_t k, int64_t n, const double* __restrict__ sigma,
                         double power, T* __restrict__ out) {
  scale_rows_body(M, k, n, sigma, power, out);
}
__global__ void __launch_bounds__(256) sqrt_clamp_kernel(const double* __restrict__ w, int64_t n, double* s) {
  sqrt_clamp_body(w, n, s);
}

// in-place: M (rows x cols fp64), column c scaled by sqrt(max(w[c], 0))
__global__ void __launch_bounds__(256)
scale_cols_sqrt_kernel(double* __restrict__ M, int64_t rows, int64_t cols, const double* __restrict__ w,
                       double rel_zero = 0.0) {
  // eigenvalues at or below rel_zero * max(w) (sorted either way) are solver noise of a zero: a zero column
  const double zero = rel_zero * fmax(fmax(w[0], w[cols - 1]), 0.0);
  const int64_t total = rows * cols;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const double we = w[e % cols];
    M[e] *= we > zero ? sqrt(we) : 0.0;
  }
}

// ---- the same for a whole lockstep group (blockIdx.y = volume): fp64 side arrays are strided in the workspace,
//      volumes / carried matrices / cores come as pointers in the kernel arguments
constexpr int kSmallBatch = 64;
struct BatchOps {
  const void* in[kSmallBatch];
  void* out[kSmallBatch];
};
template <typename T>
__global__ void __launch_bounds__(256) f32_to_f64_batched_kernel(BatchOps ops, int64_t n, double* __restrict__ y, int64_t y_stride) {
  f32_to_f64_body(static_cast<const T*>(ops.in[blockIdx.y]), n, y + (int64_t)blockIdx.y * y_stride);
}
template <typename T>
__global__ void __launch_bounds__(256)
core_from_vectors_batched_kernel(const double* __restrict__ V, int64_t v_stride, int64_t n, int64_t k, BatchOps ops,
                                 const int* __restrict__ rank_r, int64_t cap_r) {
  core_from_vectors_body(V + (int64_t)blockIdx.y * v_stride, n, k, static_cast<T*>(ops.out[blockIdx.y]),
                         rank_r ? rank_r + blockIdx.y : nullptr, cap_r);
}
__global__ void __launch_bounds__(256)
sqrt_clamp_batched_kernel(const double* __restrict__ w, int64_t stride, int64_t n, double* __restrict__ sg) {
  sqrt_clamp_body(w + (int64_t)blockIdx.y * stride, n, sg + (int64_t)blockIdx.y * stride);
}
template <typename T>
__global__ void __launch_bounds__(256)
scale_cols_to_f32_batched_kernel(const double* __restrict__ M, int64_t m_stride, int64_t rows, int64_t ldm, int64_t k,
                                 const double* __restrict__ sigma, int64_t s_stride, double power, BatchOps ops) {
  scale_cols_body(M + (int64_t)blockIdx.y * m_stride, rows, ldm, k, sigma + (int64_t)blockIdx.y * s_stride, power,
                  static_cast<T*>(ops.out[blockIdx.y]));
}
template <typename T>
__global__ void __launch_bounds__(256)
scale_rows_to_f32_batched_kernel(const double* __restrict__ M, int64_t m_stride, int64_t k, int64_t n,
                                 const double* __restrict__ sigma, int64_t s_stride, double power, BatchOps ops) {
  scale_rows_body(M + (int64_t)blockIdx.y * m_stride, k, n, sigma + (int64_t)blockIdx.y * s_stride, power,
                  static_cast<T*>(ops.out[blockIdx.y]));
}

// ------------------------------------------------------------ merged trailing sites (bond-capped sweep)
// While a bond is exact (the product N_{i+1} of the site dims to its right does not exceed the cap) site i's
// unfolding is the RAW unfolding A_i (M_i x N_i) times a block-diagonal basis:  A_i (I_{d_i} (x) W_{i+1}),
// W_{i+1} (N_{i+1} x k_{i+1}) the accumulated right bases.  Its Gram matrix is therefore a congruence of the
// raw one, and the raw Gram matrices of all those sites are block sums of the largest:
//     G_i = B^T Graw_i B,  B = I (x) W_{i+1},   Graw_{i+1} = sum of the d_i diagonal blocks of Graw_i.
// One Gram pass over the raw tensor (order N_{i0}) thus serves every site i >= i0, and one projection
// A_{i0} W_{i0} replaces the per-site projections: the tensor is read twice instead of once per Gram and
// once per projection of every site, and the cores are the same SVD cores (same arithmetic, fewer roundings).
struct MergeRanks {  // per-volume ranks of one launch (kernel argument)
  int k_right[64];   // k_{i+1}
  int k_here[64];    // k_i (w_update only)
};

// T (N_i x n_i) = Graw_i B:  T[r][(b, q)] = sum_c' Graw_i[r][b N' + c'] W[c'][q],
// Graw_i[r][c] = sum_t Graw[(t N_i + r)][(t N_i + c)]  (t over the N_top / N_i diagonal blocks of the top Gram)
__global__ void __launch_bounds__(256)
merge_stage1_kernel(const double* __restrict__ Gtop, int64_t stride_top, int n_top, const double* __restrict__ W,
                    int64_t stride_w, int ldw, double* __restrict__ T, int64_t stride_t, int n_i, int n_right,
                    int d_i, MergeRanks rk) {
  const int b = blockIdx.y;
  const int k = rk.k_right[b];
  const int cols = d_i * k;  // n_i of this volume
  const double* G = Gtop + (int64_t)b * stride_top;
  const double* Wb = W + (int64_t)b * stride_w;
  double* Tb = T + (int64_t)b * stride_t;
  const int reps = n_top / n_i;
  const int64_t total = (int64_t)n_i * cols;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int r = (int)(e / cols), col = (int)(e % cols);
    const int bb = col / k, q = col % k;
    double acc = 0.0;
    for (int t = 0; t < reps; ++t) {
      const double* grow = G + (int64_t)(t * n_i + r) * n_top + t * n_i + bb * n_right;
      for (int c = 0; c < n_right; ++c) acc = fma(grow[c], Wb[(int64_t)c * ldw + q], acc);
    }
    Tb[e] = acc;
  }
}

// G_i (n_i x n_i, ld n_i) = B^T T:  G[(a, p)][j] = sum_c' W[c'][p] T[(a N' + c')][j]
__global__ void __launch_bounds__(256)
merge_stage2_kernel(const double* __restrict__ T, int64_t stride_t, const double* __restrict__ W, int64_t stride_w,
                    int ldw, double* __restrict__ Gout, int64_t stride_g, int n_right, int d_i, MergeRanks rk) {
  const int b = blockIdx.y;
  const int k = rk.k_right[b];
  const int n = d_i * k;
  const double* Tb = T + (int64_t)b * stride_t;
  const double* Wb = W + (int64_t)b * stride_w;
  double* Gb = Gout + (int64_t)b * stride_g;
  const int64_t total = (int64_t)n * n;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int row = (int)(e / n), j = (int)(e % n);
    const int a = row / k, pp = row % k;
    double acc = 0.0;
    for (int c = 0; c < n_right; ++c) acc = fma(Wb[(int64_t)c * ldw + pp], Tb[(int64_t)(a * n_right + c) * n + j], acc);
    Gb[e] = acc;
  }
}

// W_i (N_i x k_i, ld ldw) = B V_i:  W_i[(a, c')][p] = sum_q W_{i+1}[c'][q] V[(a k_{i+1} + q)][p]   (V: n_i x n_i, ld n_i)
// optionally also as fp32 (ld = k_i, compact) for the projection GEMM
template <typename T>
__global__ void __launch_bounds__(256)
merge_basis_kernel(const double* __restrict__ Wr, int64_t stride_w, int ldw, const double* __restrict__ V,
                   int64_t stride_v, double* __restrict__ Wout, T* __restrict__ W32, int64_t stride_w32,
                   int n_right, int d_i, MergeRanks rk) {
  const int b = blockIdx.y;
  const int kr = rk.k_right[b], kh = rk.k_here[b];
  const int n = d_i * kr;
  const double* Wb = Wr + (int64_t)b * stride_w;
  const double* Vb = V + (int64_t)b * stride_v;
  double* Ob = Wout + (int64_t)b * stride_w;
  T* O32 = W32 ? W32 + (int64_t)b * stride_w32 : nullptr;
  const int64_t total = (int64_t)d_i * n_right * kh;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int row = (int)(e / kh), pp = (int)(e % kh);
    const int a = row / n_right, c = row % n_right;
    double acc = 0.0;
    for (int q = 0; q < kr; ++q) acc = fma(Wb[(int64_t)c * ldw + q], Vb[(int64_t)(a * kr + q) * n + pp], acc);
    Ob[(int64_t)row * ldw + pp] = acc;
    if (O32) O32[(int64_t)row * kh + pp] = ndmps::from_f64<T>(acc);
  }
}

__global__ void merge_basis_init_kernel(double* __restrict__ W, int64_t stride_w) {
  W[(int64_t)blockIdx.x * stride_w] = 1.0;  // W_L = [1]
}

// Fused reshape stage: the raw Gram pass reads the volume with its columns in MEMORY order (perm[c'] = site-order
// column of the c'-th smallest offset) and its slab reduction stores G'[a][b] at G[perm[a]][perm[b]]
// (ndmps_gram_indexed_f32) ...
// ... and the projection multiplies by the basis with its rows in memory order: out[c'] = W[perm[c']]
__global__ void __launch_bounds__(256)
gather_rows_kernel(const float* __restrict__ W, int64_t rows, int64_t cols, const int32_t* __restrict__ perm,
                   float* __restrict__ out, int64_t w_stride = 0, int64_t out_stride = 0) {  // volume blockIdx.y
  W += (int64_t)blockIdx.y * w_stride;
  out += (int64_t)blockIdx.y * out_stride;
  const int64_t total = rows * cols;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256)
    out[e] = W[(int64_t)perm[e / cols] * cols + e % cols];
}

struct SweepSource {           // the volume read through the index permutation (fp32, merged run only)
  const int64_t* row_off;      // [numel / n_cols]
  const int64_t* row_sorted;   // the same offsets in ascending order: the Gram kernels -- a sum over rows -- read the volume
                               // front to back (16-byte pieces of adjacent rows are neighbours in memory); may equal row_off
  const int32_t* row_order;    // row_sorted[s] = row_off[row_order[s]] (NULL: not given); the streamed projection
  const int64_t* col_off;      // [n_cols], ascending, aligned runs of four consecutive offsets
  const int32_t* col_perm;     // [n_cols]
  int64_t n_cols;
};

constexpr int64_t kMergeMax = 512;  // largest raw Gram order of the merged sites

// first site of the merged run, or L when nothing is merged (see the comment above)
int merge_start(int L, const int64_t* dims, int64_t numel, int64_t max_bond) {
  if (max_bond <= 0 || getenv("NDMPS_SWEEP_NO_MERGE")) return L;
  int best = L;
  int64_t right = 1;  // N_{i+1}
  for (int i = L - 1; i >= 1; --i) {
    const int64_t n_i = right * dims[i];
    if (right > max_bond || n_i > kMergeMax || numel / n_i < n_i) break;
    best = i;
    right = n_i;
  }
  return best >= L - 1 ? L : best;  // a run of one site is the ordinary path
}

// keep s_k > cutoff * s_0 (at least one), at most max_bond
int64_t kept_rank(const std::vector<double>& sigma, double cutoff, int64_t max_bond, double floor = kCutoffFloor) {
  const int64_t n = (int64_t)sigma.size();
  const double c = std::max(cutoff, floor);
  int64_t k = 0;
  for (int64_t i = 0; i < n; ++i) k += sigma[i] > c * sigma[0];
  k = std::max<int64_t>(k, 1);
  if (max_bond > 0) k = std::min(k, max_bond);
  return std::min(k, n);
}

// The bond-capped sweep wants chi <= 128 of the n eigenpairs of every site: the direct solver
// (eig_tridiag.hip).  Exact sweeps (all eigenpairs above the cutoff) and orders beyond its limit stay on
// the block Jacobi.
inline bool use_topk(int64_t n_max, int64_t max_bond) {
  if (getenv("NDMPS_SWEEP_JACOBI")) return false;  // A/B timing
  return max_bond > 0 && max_bond <= ndmps_syevd_topk_max_k() && n_max <= ndmps_syevd_topk_max_n();
}
// Sweeps that want every eigenpair above a cutoff (no bond cap, or one beyond the direct solver's 128) take the direct
// solver too, with the eigenvectors orthonormalised across the chip (eig_wide.inc), while its workspace -- four
// n x n planes of LU factors per matrix -- stays below kDirectFullBytes; orders beyond its limit stay on the block Jacobi.
constexpr int64_t kDirectFullBytes = (int64_t)48 << 30;
inline bool use_direct_full(int64_t n_max, int batch, int64_t max_bond) {
  if (getenv("NDMPS_SWEEP_JACOBI") || getenv("NDMPS_EXACT_JACOBI")) return false;  // A/B timing
  if (max_bond > 0 && max_bond <= ndmps_syevd_topk_max_k()) return false;            // the bond-capped path
  if (n_max > ndmps_syevd_topk_max_n()) return false;
  const int64_t need = ndmps_syevd_topk_workspace_bytes(n_max, batch, n_max);
  return need > 0 && need <= kDirectFullBytes;
}
inline int64_t eig_workspace_bytes(int64_t n_max, int batch, int64_t max_bond) {
  const int64_t jac = ndmps_syevj_batched_workspace_bytes(n_max, batch);
  if (max_bond > 0 && max_bond <= ndmps_syevd_topk_max_k() && n_max <= ndmps_syevd_topk_max_n())
    return std::max(jac, ndmps_syevd_topk_workspace_bytes(n_max, batch, std::min(max_bond, n_max)));
  if (use_direct_full(n_max, batch, max_bond)) return std::max(jac, ndmps_syevd_topk_workspace_bytes(n_max, batch, n_max));
  return jac;
}
// The direct solver leaves eigenvalue errors of up to ~1e-14 |G| (measured 6e-16 at order 4096, tools/full_probe.py):
// eigenvalues within kDirectDoubt |G| of the threshold c^2 w_0 cannot decide a rank -- under the tiny cutoffs of exact
// sweeps that is the whole lower end of the spectrum of a square noisy unfolding (its smallest singular values reach
// zero) and every numerically zero eigenvalue of a rank-deficient matrix.  First index (descending order) from which
// the eigenvalues are in doubt; n: none.
constexpr double kDirectDoubt = 1e-13;
inline int64_t direct_doubt_from(const double* w_desc, int64_t n, double c) {
  if (n < 1) return n;
  const double hi = c * c * w_desc[0] + kDirectDoubt * fabs(w_desc[0]);
  int64_t i = n;
  while (i > 0 && w_desc[i - 1] <= hi) --i;
  return i;
}
inline bool direct_rank_is_safe(const double* w_desc, int64_t n, double c) {  // nothing in doubt around the threshold
  if (n < 1) return true;
  const double thr = c * c * w_desc[0], delta = kDirectDoubt * fabs(w_desc[0]);
  for (int64_t i = 0; i < n; ++i)
    if (fabs(w_desc[i] - thr) <= delta) return false;
  return true;
}

// ------------------------------------------------------------------ sweep layout (worst case)
struct SweepLayout {
  std::vector<int64_t> max_bonds, core_off, spec_off;
  int64_t numel = 1;
  int64_t small_max = 1;      // largest eigenproblem
  int64_t gram_ws = 0;        // largest Gram workspace
  int64_t wide_elems = 0;     // largest wide unfolding (m < n), elements
  int merge_from = 0;         // first site of the merged trailing run (== L: none)
  int64_t merge_n = 0;        // order of its raw Gram matrix
  int64_t merge_w = 0;        // leading dimension of the accumulated bases
  int64_t transpose_bytes = 0;  // bf16 path: transposed copy of the merged basis
  bool device_rank = false;   // every site on the direct solver: ranks decided on the device, padded cores
  int64_t spec_stride = 0;    // singular values kept per site and volume on the device
  int L = 0, batch = 0;       // what it was computed for
  int elem_bytes = 4;         // storage element as the workspace counts it: 4 (fp32 and bf16) or 8 (fp64)
  int64_t eig_bytes = 0;      // workspace of the eigen-solvers
  int64_t workspace = 0;      // sum of the pieces carve_sweep() takes
};

// The sweep's workspace, piece by piece.  This is the only description of it: the size query carves an arena without
// memory (sweep_layout), the sweep carves the caller's.  Storage-type buffers are taken at lay.elem_bytes per element.
struct SweepBuffers {
  void* other;           // second carry buffer per volume (storage type)
  double *G, *V;         // Gram matrices; eigenvectors V / U (small_max^2 per volume)
  double *w, *sig;       // eigenvalues, singular values (small_max per volume)
  char *ev_ws, *gram_ws; // eigen-solver and Gram workspaces (the latter shared, stream-ordered)
  double *A64, *UtA;     // wide unfoldings in fp64 and U_k^T A64, per volume
  double *Graw, *Tm;     // merged run: raw Gram, T = Graw B
  double* Wm[2];         // merged run: accumulated basis W, ping and pong
  void* W32;             // ... and its copy in the storage type for the projection
  char* tws;             // bf16 products: transposed copy of the merged basis
  int *d_ranks, *d_status;  // device ranks and solver status, [site][volume] each
  double* d_spec;        // device spectra per site
};
void carve_sweep(Arena& ar, const SweepLayout& lay, SweepBuffers& b) {
  const int64_t batch = lay.batch, sq = lay.small_max * lay.small_max, raw = lay.merge_n * lay.merge_n,
                basis = lay.merge_n * lay.merge_w;
  b.other = ar.take<char>(lay.elem_bytes * batch * lay.numel);
  b.G = ar.take<double>(batch * sq);
  b.V = ar.take<double>(batch * sq);
  b.w = ar.take<double>(batch * lay.small_max);
  b.sig = ar.take<double>(batch * lay.small_max);
  b.ev_ws = ar.take<char>(lay.eig_bytes);
  b.gram_ws = ar.take<char>(lay.gram_ws);
  b.A64 = ar.take<double>(batch * lay.wide_elems);
  b.UtA = ar.take<double>(batch * lay.wide_elems);
  b.Graw = ar.take<double>(batch * raw);
  b.Tm = ar.take<double>(batch * raw);
  b.Wm[0] = ar.take<double>(batch * basis);
  b.Wm[1] = ar.take<double>(batch * basis);
  b.W32 = ar.take<char>(lay.elem_bytes * batch * basis);
  b.tws = ar.take<char>(lay.transpose_bytes);
  b.d_ranks = ar.take<int>((int64_t)2 * lay.L * batch);
  b.d_status = b.d_ranks ? b.d_ranks + (int64_t)lay.L * batch : nullptr;
  b.d_spec = ar.take<double>((int64_t)lay.L * batch * lay.spec_stride);
}

int sweep_layout(int L, const int64_t* dims, int64_t max_bond, int batch, SweepLayout& out, int elem_bytes = 4) {
  NDMPS_REQUIRE(L >= 1 && L <= 64, "L=%d outside [1, 64]", L);
  NDMPS_REQUIRE(batch >= 1 && batch <= 4096, "batch=%d outside [1, 4096]", batch);
  out.numel = 1;
  for (int i = 0; i < L; ++i) {
    NDMPS_REQUIRE(dims[i] >= 1, "dims[%d]=%lld must be positive", i, (long long)dims[i]);
    out.numel *= dims[i];
  }
  out.max_bonds.assign(L + 1, 1);
  std::vector<int64_t> left(L + 1, 1), right(L + 1, 1);
  for (int i = 0; i < L; ++i) left[i + 1] = left[i] * dims[i];
  for (int i = L - 1; i >= 0; --i) right[i] = right[i + 1] * dims[i];
  for (int i = 1; i < L; ++i) {
    int64_t b = std::min(left[i], right[i]);
    if (max_bond > 0) b = std::min(b, max_bond);
    out.max_bonds[i] = b;
  }
  out.core_off.assign(L + 1, 0);
  out.spec_off.assign(L + 1, 0);
  for (int i = 0; i < L; ++i) {
    out.core_off[i + 1] = out.core_off[i] + ndmps::round_up(out.max_bonds[i] * dims[i] * out.max_bonds[i + 1], 64);
    const int64_t m = left[i], n = dims[i] * out.max_bonds[i + 1];
    out.spec_off[i + 1] = out.spec_off[i] + (i == 0 ? 0 : std::min(m, n));
    if (i >= 1) {
      const int64_t small = std::min(m, n);
      out.small_max = std::max(out.small_max, small);
      if (n <= m) out.gram_ws = std::max(out.gram_ws, gram_ws_bound(n, batch));
      else out.wide_elems = std::max(out.wide_elems, m * n);
    }
  }
  out.merge_from = merge_start(L, dims, out.numel, max_bond);
  out.merge_n = out.merge_from < L ? right[out.merge_from] : 0;
  out.merge_w = out.merge_from < L ? std::min(out.merge_n, max_bond) : 0;
  if (out.merge_from < L) {
    out.small_max = std::max(out.small_max, out.merge_n);
    out.gram_ws = std::max(out.gram_ws, gram_ws_bound(out.merge_n, batch));
  }
  // Rank decision on the device: possible when every site's eigenproblem (order min(rows, d_i cap_{i+1}) with
  // the bonds at their caps) goes to the direct top-k solver.  The sweep then sizes everything by the caps,
  // zero-fills the columns beyond a volume's rank and never waits for the host between sites.
  out.device_rank = max_bond > 0 && max_bond <= ndmps_syevd_topk_max_k() && !getenv("NDMPS_SWEEP_HOST_RANK") &&
                    !getenv("NDMPS_SWEEP_JACOBI");
  for (int i = 1; i < L && out.device_rank; ++i)
    if (std::min(left[i], dims[i] * out.max_bonds[i + 1]) > ndmps_syevd_topk_max_n()) out.device_rank = false;
  out.spec_stride = max_bond > 0 ? std::min<int64_t>(max_bond, out.small_max) : 0;
  out.L = L;
  out.batch = batch;
  out.elem_bytes = elem_bytes;
  out.eig_bytes = eig_workspace_bytes(out.small_max, batch, max_bond);
  out.transpose_bytes = ndmps_gemm_bf16_workspace_bytes(0, std::max<int64_t>(out.merge_w, 1), std::max<int64_t>(out.merge_n, 1));
  Arena sizing(nullptr, 0);  // a carve on no memory: only `used` advances
  SweepBuffers unused;
  carve_sweep(sizing, out, unused);
  out.workspace = ndmps::round_up(sizing.used, 256) + 256;
  return NDMPS_OK;
}

}  // namespace

extern "C" int ndmps_tt_layout(int L, const int64_t* h_dims, int64_t max_bond, int64_t* h_max_bonds,
                               int64_t* h_core_offsets, int64_t* h_spec_offsets,
                               int64_t* h_workspace_bytes) {
  NDMPS_REQUIRE(h_dims, "NULL dims");
  SweepLayout lay;
  NDMPS_TRY(sweep_layout(L, h_dims, max_bond, 1, lay));
  for (int i = 0; i <= L; ++i) {
    if (h_max_bonds) h_max_bonds[i] = lay.max_bonds[i];
    if (h_core_offsets) h_core_offsets[i] = lay.core_off[i];
    if (h_spec_offsets) h_spec_offsets[i] = lay.spec_off[i];
  }
  if (h_workspace_bytes) *h_workspace_bytes = lay.workspace;
  return NDMPS_OK;
}

extern "C" int64_t ndmps_tt_sweep_batched_workspace_bytes(int batch, int L, const int64_t* h_dims,
                                                          int64_t max_bond) {
  SweepLayout lay;
  if (!h_dims || sweep_layout(L, h_dims, max_bond, batch, lay) != NDMPS_OK) return -1;
  return lay.workspace;
}
// the same for fp64 storage (ndmps_tt_sweep_batched_f64): carried matrices of 8-byte elements
extern "C" int64_t ndmps_tt_sweep_batched_workspace_bytes_f64(int batch, int L, const int64_t* h_dims,
                                                              int64_t max_bond) {
  SweepLayout lay;
  if (!h_dims || sweep_layout(L, h_dims, max_bond, batch, lay, 8) != NDMPS_OK) return -1;
  return lay.workspace;
}

// All volumes of the batch have the same site dims; they advance through the sites in lockstep so that every site's
// eigenproblems are solved by ONE batched solve (its sequential depth is the cost of the path).  While the volumes
// of a group stay in the same state their Gram matrices, cores and projections are one launch per step as well
// (Sweep::uniform); a group whose ranks have diverged goes volume by volume.
namespace {
// element-type dispatch of the two streaming products of the sweep
inline int gram_T(const float* A, int64_t m, int64_t n, int64_t lda, double* G, void* ws, int64_t wsb, hipStream_t s) {
  return ndmps_gram_f32(A, m, n, lda, G, ws, wsb, s);
}
inline int gram_T(const __bf16* A, int64_t m, int64_t n, int64_t lda, double* G, void* ws, int64_t wsb, hipStream_t s) {
  return ndmps_gram_bf16(A, m, n, lda, G, ws, wsb, s);
}
inline int gram_T(const double* A, int64_t m, int64_t n, int64_t lda, double* G, void* ws, int64_t wsb, hipStream_t s) {
  return ndmps_gram_f64(A, m, n, lda, G, ws, wsb, s);
}
inline int64_t gram_need(const float*, int64_t m, int64_t n) { return ndmps_gram_workspace_bytes(m, n); }
inline int64_t gram_need(const __bf16*, int64_t m, int64_t n) { return ndmps_gram_workspace_bytes(m, n); }
inline int64_t gram_need(const double*, int64_t m, int64_t n) { return ndmps_gram_f64_workspace_bytes(m, n); }
// the group-wide Gram launch (LDS-staged fp32 panels) exists for fp32 / bf16 storage only
template <typename T>
inline int64_t gram_batched_need(int batch, int64_t m, int64_t n) {
  return sizeof(T) == 8 ? 0 : ndmps_gram_batched_workspace_bytes(batch, m, n);
}
// one launch for the Gram matrices of a lockstep group (same shape; n >= 128, m >= 256)
inline int gram_batched_T(int batch, const float* const* A, int64_t m, int64_t n, double* G, int64_t stride, void* ws,
                          int64_t wsb, hipStream_t s) {
  return ndmps_gram_batched_f32(batch, A, m, n, n, G, stride, ws, wsb, s);
}
inline int gram_batched_T(int batch, const __bf16* const* A, int64_t m, int64_t n, double* G, int64_t stride, void* ws,
                          int64_t wsb, hipStream_t s) {
  return ndmps_gram_batched_bf16(batch, (const void* const*)A, m, n, n, G, stride, ws, wsb, s);
}
inline int gram_batched_T(int, const double* const*, int64_t, int64_t, double*, int64_t, void*, int64_t, hipStream_t) {
  ndmps::set_error("internal: no group-wide Gram launch for fp64 storage");
  return NDMPS_EINVAL;
}
inline int gram_batched_src(int, const double* const*, int64_t, int64_t, const SweepSource&, double*, int64_t, void*,
                            int64_t, hipStream_t) {
  ndmps::set_error("the fused reshape stage is fp32 only");
  return NDMPS_EINVAL;
}
inline int gram_batched_src(int batch, const float* const* vol, int64_t m, int64_t n, const SweepSource& src, double* G,
                            int64_t stride, void* ws, int64_t wsb, hipStream_t s) {
  return ndmps_gram_batched_indexed_f32(batch, vol, m, n, src.row_sorted, src.col_off, src.col_perm, G, stride, ws, wsb, s);
}
inline int gram_batched_src(int, const __bf16* const*, int64_t, int64_t, const SweepSource&, double*, int64_t, void*,
                            int64_t, hipStream_t) {
  ndmps::set_error("the fused reshape stage is fp32 only");
  return NDMPS_EINVAL;
}
// gemm_T, gemm_any, gemm_batched_T: typed.h
// fp32 only: Gram and projection of the merged run through the permutation tables
inline int gram_src(const float* vol, int64_t m, int64_t n, const SweepSource& src, double* G, void* ws, int64_t wsb,
                    hipStream_t s) {
  return ndmps_gram_indexed_f32(vol, m, n, src.row_sorted, src.col_off, src.col_perm, G, ws, wsb, s);
}
inline int gram_src(const __bf16*, int64_t, int64_t, const SweepSource&, double*, void*, int64_t, hipStream_t) {
  ndmps::set_error("the fused reshape stage is fp32 only");
  return NDMPS_EINVAL;
}
inline int gram_src(const double*, int64_t, int64_t, const SweepSource&, double*, void*, int64_t, hipStream_t) {
  ndmps::set_error("the fused reshape stage is fp32 only");
  return NDMPS_EINVAL;
}
inline int project_src(const double*, int64_t, int64_t, int64_t, const SweepSource&, const double*, double*, double*,
                       hipStream_t) {
  return NDMPS_EINVAL;
}
inline int project_src(const float* vol, int64_t m, int64_t k, int64_t n, const SweepSource& src, const float* W,
                       float* scratch, float* out, hipStream_t s) {
  hipLaunchKernelGGL(gather_rows_kernel, dim3(grid1d(n * k)), dim3(256), 0, s, W, n, k, src.col_perm, scratch);
  NDMPS_LAUNCH_CHECK();
  return ndmps_sgemm_indexed(m, k, n, vol, 0, src.row_off, src.col_off, 1, scratch, k, out, k, nullptr, nullptr, s);
}
inline int project_src(const __bf16*, int64_t, int64_t, int64_t, const SweepSource&, const __bf16*, __bf16*, __bf16*,
                       hipStream_t) {
  return NDMPS_EINVAL;
}

// status of the direct solver for one matrix (eig_tridiag.hip): 1 = Cholesky breakdown, 2 = a team gave up waiting
inline int solver_failed(int site, int volume, int status) {
  if (status == 2) {
    ndmps::set_error("site %d, volume %d: the resident tridiagonalisation gave up waiting for its workgroups (3 s; is the "
                     "GPU shared with another process?); repeat the sweep after ndmps_syevd_topk_set_team(0)", site, volume);
    return NDMPS_ETEAM;
  }
  ndmps::set_error("site %d, volume %d: eigenvector block lost rank in the orthonormalisation", site, volume);
  return NDMPS_ENOCONV;
}

// The two halves of a sweep whose ranks are decided on the device: everything such a sweep needs from the host is known
// before it starts, so it can be ENQUEUED as a whole (SweepAsync: ranks, status words and kept singular values travel to
// pinned host memory behind the last kernel, nobody waits) and READ later, once the caller has synchronised with the
// stream (sweep_collect: bonds, spectra, a solver's failure).  The caller's host thread is free in between -- the objects
// of the previous batch are built while this one runs (core/batch.py).
struct SweepAsync {
  int* h_ranks;    // pinned, 2 L batch ints: [site][volume] ranks, then [site][volume] solver status
  double* h_spec;  // pinned, L batch spec_stride doubles (may be NULL when the layout keeps no spectra)
};
int sweep_collect(int batch, int L, int64_t spec_stride, const int* host_i, const double* host_s, int64_t* h_bonds_out,
                  double* h_spectra, const int64_t* h_spec_offsets) {
  const int64_t spec_total = h_spec_offsets ? h_spec_offsets[L] : 0;
  for (int b = 0; b < batch; ++b) {
    h_bonds_out[(int64_t)b * (L + 1)] = 1;
    h_bonds_out[(int64_t)b * (L + 1) + L] = 1;
  }
  for (int i = 1; i < L; ++i)
    for (int b = 0; b < batch; ++b) {
      if (host_i[(size_t)L * batch + (size_t)i * batch + b] != 0)
        return solver_failed(i, b, host_i[(size_t)L * batch + (size_t)i * batch + b]);
      h_bonds_out[(int64_t)b * (L + 1) + i] = host_i[(size_t)i * batch + b];
      if (h_spectra && h_spec_offsets) {
        const int64_t room = h_spec_offsets[i + 1] - h_spec_offsets[i];
        double* dst = h_spectra + (int64_t)b * spec_total + h_spec_offsets[i];
        const int64_t have = std::min(room, spec_stride);
        for (int64_t t = 0; t < room; ++t)
          dst[t] = (t < have && host_s) ? host_s[((size_t)i * batch + b) * spec_stride + t] : 0.0;
      }
    }
  return NDMPS_OK;
}

// A sweep whose input is still intact (the fused one reads the volumes in place) repeats itself on the column
// launches when a resident tridiagonalisation gave up (NDMPS_ETEAM); the others hand the code to the caller, who
// owns the site-order copy the sweep has overwritten.
template <typename F>
int retry_without_team(F&& sweep) {
  int rc = sweep();
  if (rc != NDMPS_ETEAM) return rc;
  (void)ndmps_syevd_topk_note_team_fallback();
  const int was = ndmps_syevd_topk_set_team(0);
  rc = sweep();
  (void)ndmps_syevd_topk_set_team(was);
  return rc;
}

// One TT-SVD sweep over a lockstep group of `batch` volumes: the arguments, the layout, the carved workspace and the
// per-volume state, with one member function per stage.  sweep_impl() below drives them:
//
//   prepare()                   argument checks, layout, workspace carve, initial state
//   merged_run()                sites merge_from .. L-1 from ONE Gram pass and ONE projection pass:
//     merged_raw_gram()           the raw Gram of the group
//     merged_site_gram(i)         G_i = B^T G_raw B (batched fp64 products, or merge_stage1 / merge_stage2)
//     merged_basis_and_core(i)    W_i = B V_i and the core of site i
//     merged_project()            carry = A_raw W
//   then for every remaining site i, right to left:
//     site_gram(i)                small-side Gram matrices: one launch for the group, the wide pair, or per volume
//     solve_site(i, have_a)       the eigenproblems of the site and the rank of every volume:
//       solve_on_device()           ranks decided on the device (no host round trip)
//       solve_direct()              eigenvalues to the host, rank decision, kept vectors (direct solver)
//       measure_doubt()             singular values the eigenvalues cannot resolve, measured as |A v|
//       solve_jacobi()              the block Jacobi, also as the redo of a direct solve that lost rank
//     site_core_and_carry(i)      core and carried matrix: core_and_carry_uniform() or core_and_carry_volume()
//   finish()                    the site-0 copy; ranks and spectra back from the device, or their async enqueue
//
// Every stage enqueues on `s` in program order; the host waits only where eigenvalues or tail norms are fetched and in
// finish().
template <typename T>
struct Sweep {
  // ---- arguments
  int batch;
  T* const* h_dense;
  int L;
  const int64_t* h_dims;
  double cutoff;
  int64_t max_bond;
  T* const* h_cores;
  const int64_t* h_core_offsets;
  int64_t* h_bonds_out;
  double* h_spectra;
  const int64_t* h_spec_offsets;
  void* d_ws;
  int64_t ws_bytes;
  hipStream_t s;
  const SweepSource* src;
  const SweepAsync* async;
  // ---- layout and workspace
  SweepLayout lay;
  SweepBuffers ws;
  int64_t sq = 0;          // small_max^2: doubles per volume in G and V
  int64_t spec_total = 0;  // spectrum values per volume in h_spectra
  // ---- per-volume state
  std::vector<T*> cur, nxt;                 // carried matrix and the buffer the next one goes to
  std::vector<int64_t> chi_r, cur_elems;    // bond to the right of the current site; elements of cur
  std::vector<int64_t> eig_n, kept, doubt;  // order of the site's eigenproblem, kept rank, first eigenvalue in doubt
  std::vector<double> host_w;               // eigenvalues on the host, small_max per volume

  double rel_cutoff() const { return std::max(cutoff, cutoff_floor<T>()); }
  T* core(int b, int i) const { return h_cores[b] + h_core_offsets[i]; }
  double* Gb(int b) const { return ws.G + (int64_t)b * sq; }
  double* Vb(int b) const { return ws.V + (int64_t)b * sq; }

  // every volume in the same state (always so when the ranks are decided on the device): the per-volume launches of
  // a site become one launch each
  bool uniform() const {
    if (batch < 2) return false;
    for (int b = 1; b < batch; ++b)
      if (chi_r[b] != chi_r[0] || cur_elems[b] != cur_elems[0]) return false;
    return true;
  }
  bool uniform_kept() const {
    for (int b = 1; b < batch; ++b)
      if (kept[b] != kept[0] || eig_n[b] != eig_n[0]) return false;
    return true;
  }
  // base + b stride for every volume: the pointer table of a batched product
  std::vector<double*> strided(double* base, int64_t stride) const {
    std::vector<double*> p(batch);
    for (int b = 0; b < batch; ++b) p[b] = base + (int64_t)b * stride;
    return p;
  }
  // ... and small enough for the pointer tables of the group kernels and of the batched products
  bool uniform_small() const { return uniform() && batch <= std::min(kSmallBatch, ndmps_gemm_batched_max()); }

  int prepare() {
    NDMPS_REQUIRE(h_dense && h_dims && h_cores && h_core_offsets && h_bonds_out, "NULL sweep argument");
    NDMPS_REQUIRE(cutoff >= 0.0, "cutoff must be non-negative");
    NDMPS_TRY(sweep_layout(L, h_dims, max_bond, batch, lay, sizeof(T) == 8 ? 8 : 4));
    if (d_ws == nullptr || ws_bytes < lay.workspace) {
      ndmps::set_error("sweep workspace too small: %lld < %lld", (long long)ws_bytes, (long long)lay.workspace);
      return NDMPS_EWORKSPACE;
    }
    for (int b = 0; b < batch; ++b) NDMPS_REQUIRE(h_dense[b] && h_cores[b], "NULL volume or core arena %d", b);
    Arena ar(d_ws, ws_bytes);
    carve_sweep(ar, lay, ws);
    NDMPS_REQUIRE(ar.fits(), "workspace carve failed");
    if (src) {
      // h_dense[b] is the C-order volume and stays untouched: the carried matrices ping-pong between the halves
      // of the workspace buffer (the first one is already <= half the tensor)
      NDMPS_REQUIRE(lay.merge_from < L && src->n_cols == lay.merge_n &&
                        (lay.numel / lay.merge_n) * lay.merge_w <= lay.numel / 2,
                    "the fused reshape stage needs a merged run of %lld columns (see ndmps_tt_merge_columns)",
                    (long long)src->n_cols);
    }
    sq = lay.small_max * lay.small_max;
    spec_total = h_spec_offsets ? h_spec_offsets[L] : 0;
    cur.assign(h_dense, h_dense + batch);
    nxt.resize(batch);
    chi_r.assign(batch, 1);
    cur_elems.assign(batch, lay.numel);
    eig_n.assign(batch, 0);
    kept.assign(batch, 0);
    host_w.assign((size_t)batch * lay.small_max, 0.0);
    for (int b = 0; b < batch; ++b) {
      nxt[b] = static_cast<T*>(ws.other) + (int64_t)b * lay.numel;
      h_bonds_out[(int64_t)b * (L + 1)] = 1;
      h_bonds_out[(int64_t)b * (L + 1) + L] = 1;
    }
    return NDMPS_OK;
  }

  // ------------------------------------------------------------------------------------------------ eigenproblems
  // One batched eigen-solve for site i on the matrices G[b] (order eig_n[b], ld eig_n[b]): the rank of every volume
  // (kept[b]) and the kept eigenvectors in the columns of V[b].  have_a: the unfolding itself is at hand in cur[b].
  int solve_site(int i, bool have_a) {
    const int64_t site_n = *std::max_element(eig_n.begin(), eig_n.end());
    const int64_t k_cap = std::min<int64_t>(max_bond, site_n);
    if (lay.device_rank) return solve_on_device(i, k_cap);
    const bool topk = use_topk(site_n, max_bond);
    // every eigenpair above the cutoff, direct solver
    bool full = !topk && use_direct_full(lay.small_max, batch, max_bond);
    const int64_t k_solver = topk ? k_cap : lay.small_max;
    if (topk || full) {
      NDMPS_TRY(ndmps_syevd_topk_values_f64(batch, ws.G, sq, eig_n.data(), ws.V, sq, ws.w, lay.small_max, k_solver,
                                            ws.ev_ws, lay.eig_bytes, s));
      // the host waits for the eigenvalues anyway: a resident launch that gave up is redone on the column launches
      NDMPS_TRY(ndmps_syevd_topk_recover_f64(batch, eig_n.data(), k_solver, ws.ev_ws, lay.eig_bytes, nullptr, s));
      NDMPS_TRY(fetch_eigenvalues());
    }
    if (full) {
      // eigenvalues in doubt (direct_doubt_from): with the unfolding at hand their singular values are measured
      // as |A v| behind the solve (measure_doubt); without it (merged run) the Jacobi decides (G is untouched)
      doubt.assign(batch, 0);
      for (int b = 0; b < batch; ++b) {
        doubt[b] = direct_doubt_from(host_w.data() + (int64_t)b * lay.small_max, eig_n[b], rel_cutoff());
        if (doubt[b] < eig_n[b] && !have_a) full = false;
      }
    }
    if (!topk && !full) return solve_jacobi(i, true);
    return solve_direct(i, topk, k_solver);
  }

  // no host round trip: eigenvalues -> rank (device) -> k_b eigenvectors, the other columns up to the cap zero
  int solve_on_device(int i, int64_t k_cap) {
    NDMPS_TRY(ndmps_syevd_topk_values_f64(batch, ws.G, sq, eig_n.data(), ws.V, sq, ws.w, lay.small_max, k_cap, ws.ev_ws,
                                          lay.eig_bytes, s));
    NDMPS_TRY(ndmps_syevd_topk_vectors_auto_f64(batch, eig_n.data(), k_cap, rel_cutoff(), ws.d_ranks + (int64_t)i * batch,
                                                ws.d_spec + (int64_t)i * batch * lay.spec_stride, lay.spec_stride,
                                                ws.d_status + (int64_t)i * batch, ws.ev_ws, lay.eig_bytes, s));
    for (int b = 0; b < batch; ++b) kept[b] = k_cap;
    return NDMPS_OK;
  }

  int fetch_eigenvalues() {
    NDMPS_CHECK_HIP(hipMemcpyAsync(host_w.data(), ws.w, sizeof(double) * batch * lay.small_max, hipMemcpyDeviceToHost, s));
    NDMPS_CHECK_HIP(hipStreamSynchronize(s));
    return NDMPS_OK;
  }

  // kept[b] from the eigenvalues on the host: singular values = sqrt, the rank rule of kept_rank; record: the singular
  // values also go to the caller's spectra
  void ranks_from_eigenvalues(int i, bool record) {
    for (int b = 0; b < batch; ++b) {
      const int64_t small = eig_n[b];
      std::vector<double> sv(host_w.begin() + (int64_t)b * lay.small_max, host_w.begin() + (int64_t)b * lay.small_max + small);
      for (auto& x : sv) x = sqrt(std::max(x, 0.0));
      kept[b] = kept_rank(sv, cutoff, max_bond, cutoff_floor<T>());
      if (record && h_spectra && h_spec_offsets) {
        // the layout reserves min(m, d_i max_bond_{i+1}) values for the bond; a merged site may be larger
        const int64_t room = h_spec_offsets[i + 1] - h_spec_offsets[i];
        memcpy(h_spectra + (int64_t)b * spec_total + h_spec_offsets[i], sv.data(), std::min(small, room) * sizeof(double));
      }
    }
  }

  // the block Jacobi: eigenvalues, rank decision on the host, kept vectors
  int solve_jacobi(int i, bool record) {
    int sweeps = 0;
    NDMPS_TRY(ndmps_syevj_batched_values_f64(batch, ws.G, sq, eig_n.data(), ws.V, sq, ws.w, lay.small_max,
                                             sweep_eig_tol(sizeof(T) == 8), ws.ev_ws, lay.eig_bytes, &sweeps, s));
    NDMPS_TRY(fetch_eigenvalues());
    ranks_from_eigenvalues(i, record);
    return ndmps_syevj_batched_vectors_f64(batch, ws.G, sq, eig_n.data(), ws.V, sq, ws.w, lay.small_max, kept.data(), ws.ev_ws,
                                           lay.eig_bytes, s);
  }

  // the direct solver behind its eigenvalues (already in host_w): ranks, then the kept vectors.  topk: at most k_solver of
  // them; else every eigenpair above the cutoff, with the eigenvalues in doubt measured afterwards.
  int solve_direct(int i, bool topk, int64_t k_solver) {
    ranks_from_eigenvalues(i, true);
    for (int b = 0; b < batch; ++b)
      if (!topk && doubt[b] < eig_n[b]) kept[b] = eig_n[b];  // every vector first; the rank follows from |A v| (measure_doubt)
    std::vector<int> status(batch, 0);
    NDMPS_TRY(ndmps_syevd_topk_vectors_f64(batch, eig_n.data(), kept.data(), k_solver, ws.ev_ws, lay.eig_bytes, status.data(), s));
    bool redo = false;
    for (int b = 0; b < batch; ++b)
      if (status[b] != 0) {
        if (topk) return solver_failed(i, b, status[b]);
        redo = true;  // the wide block lost rank (a cluster tighter than the shifts resolve): the Jacobi has no such case
      }
    if (redo) return solve_jacobi(i, false);
    return topk ? NDMPS_OK : measure_doubt(i);
  }

  // Singular values in doubt, measured: s_j = |A v_j| (or |A^T u_j|) for the eigenvectors from doubt[b] on; G (free
  // now) is the scratch.  The kept rank = the vectors in front + those whose s_j passes the cutoff.
  int measure_doubt(int i) {
    for (int b = 0; b < batch; ++b) {
      const int64_t small = eig_n[b], i0 = doubt[b], t = small - i0;
      if (t <= 0) continue;
      const int64_t n = h_dims[i] * chi_r[b], m = cur_elems[b] / n;
      const bool right = n <= m;  // G = A^T A: vectors in R^n, |A v|; else G = A A^T: |A^T u|
      double* out = nullptr;
      NDMPS_TRY(tail_norms((const T*)cur[b], right ? n : (int64_t)1, right ? (int64_t)1 : n, right ? m : n, right ? n : m,
                           Vb(b), small, i0, t, Gb(b), sq, &out, s));
      std::vector<double> s2((size_t)t);
      NDMPS_CHECK_HIP(hipMemcpyAsync(s2.data(), out, sizeof(double) * t, hipMemcpyDeviceToHost, s));
      NDMPS_CHECK_HIP(hipStreamSynchronize(s));
      const double s0 = sqrt(std::max(host_w[(int64_t)b * lay.small_max], 0.0));
      int64_t k = i0;
      for (int64_t j = 0; j < t; ++j) k += sqrt(std::max(s2[(size_t)j], 0.0)) > rel_cutoff() * s0;
      k = std::max<int64_t>(k, 1);
      if (max_bond > 0) k = std::min(k, max_bond);
      kept[b] = std::min(k, small);
      if (h_spectra && h_spec_offsets) {
        const int64_t room = h_spec_offsets[i + 1] - h_spec_offsets[i];
        for (int64_t j = 0; j < t && i0 + j < room; ++j)
          h_spectra[(int64_t)b * spec_total + h_spec_offsets[i] + i0 + j] = sqrt(std::max(s2[(size_t)j], 0.0));
      }
    }
    return NDMPS_OK;
  }

  // --------------------------------------------------------------------------------------- merged trailing run
  // sites merge_from .. L-1 from ONE Gram pass and ONE projection pass (see the comment above MergeRanks)
  int merged_run() {
    NDMPS_TRY(merged_raw_gram());
    hipLaunchKernelGGL(merge_basis_init_kernel, dim3(batch), dim3(1), 0, s, ws.Wm[0], lay.merge_n * lay.merge_w);
    NDMPS_LAUNCH_CHECK();
    int wcur = 0;         // which of Wm holds W_{i+1}
    int64_t n_right = 1;  // N_{i+1}
    for (int i = L - 1; i >= lay.merge_from; --i) {
      NDMPS_TRY(merged_site_gram(i, n_right, ws.Wm[wcur]));
      NDMPS_TRY(solve_site(i, false));
      NDMPS_TRY(merged_basis_and_core(i, n_right, ws.Wm[wcur], ws.Wm[wcur ^ 1]));
      wcur ^= 1;
      n_right *= h_dims[i];
    }
    return merged_project();
  }

  int merged_raw_gram() {
    const int64_t n0 = lay.merge_n, m0 = lay.numel / n0, stride_top = n0 * n0;
    const int64_t raw_batched = gram_batched_need<T>(batch, m0, n0);
    if (batch > 1 && raw_batched > 0 && raw_batched <= lay.gram_ws) {
      // the whole group in one launch (long slabs: a fraction of the partial tiles, no launch gaps); with src the columns
      // are visited in memory order and the slab reduction stores the result in site order
      return src ? gram_batched_src(batch, cur.data(), m0, n0, *src, ws.Graw, stride_top, ws.gram_ws, lay.gram_ws, s)
                 : gram_batched_T(batch, cur.data(), m0, n0, ws.Graw, stride_top, ws.gram_ws, lay.gram_ws, s);
    }
    for (int b = 0; b < batch; ++b) {
      double* Gr = ws.Graw + (int64_t)b * stride_top;
      NDMPS_TRY(src ? gram_src(cur[b], m0, n0, *src, Gr, ws.gram_ws, lay.gram_ws, s)
                    : gram_T(cur[b], m0, n0, n0, Gr, ws.gram_ws, lay.gram_ws, s));
    }
    return NDMPS_OK;
  }

  // ranks of the volumes base .. base + count - 1 for one merge launch; here == nullptr: k_here = 0
  MergeRanks merge_ranks(int base, int count, const int64_t* here) const {
    MergeRanks rk;
    for (int t = 0; t < count; ++t) {
      rk.k_right[t] = (int)chi_r[base + t];
      rk.k_here[t] = here ? (int)here[base + t] : 0;
    }
    return rk;
  }

  // G_i = B^T Graw_i B into G, B = I (x) W (the accumulated basis W_{i+1}); eig_n[b] = its order
  int merged_site_gram(int i, int64_t n_right, double* W) {
    const int64_t n0 = lay.merge_n, ldw = lay.merge_w, stride_top = n0 * n0, stride_w = n0 * ldw;
    const int64_t d_i = h_dims[i], n_i = n_right * d_i;
    for (int b = 0; b < batch; ++b) eig_n[b] = d_i * chi_r[b];
    // the top site of the run (its raw Gram IS the one computed: no block sums) of a uniform group: both
    // congruence stages as batched fp64 products on the MFMA (0.3 + 0.3 ms of scalar loops per group otherwise,
    // right behind the Gram pass on the critical path)
    if (n_i == n0 && uniform() && batch <= ndmps_gemm_batched_max() && n_i * chi_r[0] >= 4096) {
      const int64_t kr = chi_r[0], n = d_i * kr;
      const auto pa = strided(ws.Graw, stride_top), pb = strided(W, stride_w), pc = strided(ws.Tm, stride_top);
      std::vector<double*> qa, qb, qc;
      for (int b = 0; b < batch; ++b)
        for (int64_t a = 0; a < d_i; ++a) {
          qa.push_back(pb[b]);
          qb.push_back(pc[b] + a * n_right * n);
          qc.push_back(Gb(b) + a * kr * n);
        }
      // T[(r, blk)][q] = sum_c Graw[(r, blk)][c] W[c][q]: rows (r, blk) of n_right contiguous elements
      NDMPS_TRY(ndmps_dgemm_batched(batch, 0, 0, n_i * d_i, kr, n_right, pa.data(), n_right, pb.data(), ldw, pc.data(), kr, s));
      // G[(a, p)][j] = sum_c W[c][p] T[(a n_right + c)][j]: one product per (volume, a)
      const size_t per = (size_t)ndmps_gemm_batched_max();
      for (size_t base = 0; base < qa.size(); base += per) {
        const int count = (int)std::min(per, qa.size() - base);
        NDMPS_TRY(ndmps_dgemm_batched(count, 1, 0, kr, n, n_right, qa.data() + base, ldw, qb.data() + base, n,
                                      qc.data() + base, n, s));
      }
      return NDMPS_OK;
    }
    for (int base = 0; base < batch; base += 64) {
      const int count = std::min(64, batch - base);
      const int64_t biggest = std::max<int64_t>(1, *std::max_element(eig_n.begin() + base, eig_n.begin() + base + count));
      const MergeRanks rk = merge_ranks(base, count, nullptr);
      const int g1 = (int)std::min<int64_t>(ceil_div(n_i * biggest, 256), 1024);
      const int g2 = (int)std::min<int64_t>(ceil_div(biggest * biggest, 256), 1024);
      hipLaunchKernelGGL(merge_stage1_kernel, dim3(g1, count), dim3(256), 0, s, ws.Graw + base * stride_top, stride_top,
                         (int)n0, W + base * stride_w, stride_w, (int)ldw, ws.Tm + base * stride_top, stride_top,
                         (int)n_i, (int)n_right, (int)d_i, rk);
      hipLaunchKernelGGL(merge_stage2_kernel, dim3(g2, count), dim3(256), 0, s, ws.Tm + base * stride_top, stride_top,
                         W + base * stride_w, stride_w, (int)ldw, ws.G + base * sq, sq, (int)n_right, (int)d_i, rk);
    }
    NDMPS_LAUNCH_CHECK();
    return NDMPS_OK;
  }

  // W_i = B V_i into Wnext (at the first site of the run also in the storage type, for the projection), the core of
  // site i from the kept vectors, and the bond
  int merged_basis_and_core(int i, int64_t n_right, double* W, double* Wnext) {
    const int64_t stride_w = lay.merge_n * lay.merge_w, d_i = h_dims[i], n_i = n_right * d_i;
    T* W32 = static_cast<T*>(ws.W32);
    for (int base = 0; base < batch; base += 64) {
      const int count = std::min(64, batch - base);
      const int64_t biggest = std::max<int64_t>(1, *std::max_element(kept.begin() + base, kept.begin() + base + count));
      const MergeRanks rk = merge_ranks(base, count, kept.data());
      const int g3 = (int)std::min<int64_t>(ceil_div(n_i * biggest, 256), 1024);
      hipLaunchKernelGGL(merge_basis_kernel<T>, dim3(g3, count), dim3(256), 0, s, W + base * stride_w, stride_w,
                         (int)lay.merge_w, ws.V + base * sq, sq, Wnext + base * stride_w,
                         i == lay.merge_from ? W32 + base * stride_w : (T*)nullptr, stride_w, (int)n_right, (int)d_i, rk);
    }
    NDMPS_LAUNCH_CHECK();
    if (batch > 1 && uniform_kept()) {
      for (int base = 0; base < batch; base += kSmallBatch) {
        const int count = std::min(kSmallBatch, batch - base);
        BatchOps ops;
        for (int t = 0; t < count; ++t) ops.out[t] = core(base + t, i);
        hipLaunchKernelGGL(core_from_vectors_batched_kernel<T>, dim3(grid1d(kept[0] * eig_n[0]), count), dim3(256), 0, s,
                           Vb(base), sq, eig_n[0], kept[0], ops, right_ranks(i, base), chi_r[base]);
      }
    } else {
      for (int b = 0; b < batch; ++b)
        hipLaunchKernelGGL(core_from_vectors_kernel<T>, dim3(grid1d(kept[b] * eig_n[b])), dim3(256), 0, s,
                           Vb(b), eig_n[b], kept[b], core(b, i), right_ranks(i, b), chi_r[b]);
    }
    NDMPS_LAUNCH_CHECK();
    for (int b = 0; b < batch; ++b) {
      chi_r[b] = kept[b];
      h_bonds_out[(int64_t)b * (L + 1) + i] = kept[b];
    }
    return NDMPS_OK;
  }

  // carry = A_raw W (m0 x k): the one projection of the run
  int merged_project() {
    const int64_t n0 = lay.merge_n, m0 = lay.numel / n0, stride_top = n0 * n0, stride_w = n0 * lay.merge_w;
    T* W32 = static_cast<T*>(ws.W32);
    if (src && uniform() && batch <= ndmps_gemm_batched_max()) {
      // the whole group: the basis rows into memory order (one launch, into the fp64 slots of T, free now), then one
      // batched product that reads the volumes through the permutation tables
      const int64_t k = chi_r[0];
      float* wperm0 = reinterpret_cast<float*>(ws.Tm);
      const int64_t wperm_stride = stride_top * 2;  // in floats
      hipLaunchKernelGGL(gather_rows_kernel, dim3(grid1d(n0 * k), batch), dim3(256), 0, s, (const float*)W32, n0, k,
                         src->col_perm, wperm0, stride_w, wperm_stride);
      NDMPS_LAUNCH_CHECK();
      std::vector<const float*> pa(batch), pb(batch);
      std::vector<float*> pc(batch);
      for (int b = 0; b < batch; ++b) {
        pa[b] = (const float*)cur[b];
        pb[b] = wperm0 + (int64_t)b * wperm_stride;
        pc[b] = (float*)nxt[b];
      }
      // 64 gathered columns (a bond cap of 32): the stream over the rows in memory order; anything else: the tile kernel
      if (n0 == 64 && (k == 32 || k == 64) && src->row_order && src->row_sorted != src->row_off && !getenv("NDMPS_PROJ64_TILES"))
        NDMPS_TRY(ndmps_sgemm_gathered64_stream_batched(batch, m0, k, pa.data(), src->row_sorted, src->row_order, src->col_off,
                                                        pb.data(), k, pc.data(), k, s));
      else
        NDMPS_TRY(ndmps_sgemm_indexed_batched(batch, m0, k, n0, pa.data(), 0, src->row_off, src->col_off, 1, pb.data(), k,
                                              pc.data(), k, nullptr, nullptr, s));
    } else {
      for (int b = 0; b < batch; ++b) {
        // with src, T (fp64 scratch of the congruences, free now) holds the basis with its rows in memory order
        T* wperm = reinterpret_cast<T*>(ws.Tm + (int64_t)b * stride_top);
        const T* Wb = W32 + (int64_t)b * stride_w;
        NDMPS_TRY(src ? project_src(cur[b], m0, chi_r[b], n0, *src, Wb, wperm, nxt[b], s)
                      : gemm_T(0, m0, chi_r[b], n0, cur[b], Wb, chi_r[b], nxt[b], ws.tws, lay.transpose_bytes, s));
      }
    }
    for (int b = 0; b < batch; ++b) {
      std::swap(cur[b], nxt[b]);
      if (src) nxt[b] = cur[b] + lay.numel / 2;  // the volume stays untouched: the other half of the workspace buffer
      cur_elems[b] = m0 * chi_r[b];
    }
    return NDMPS_OK;
  }

  // ------------------------------------------------------------------------------------------- one site at a time
  // small-side Gram matrix of every volume's unfolding (m x n, n = d_i chi_r) into G; eig_n[b] = min(m, n)
  int site_gram(int i) {
    if (uniform()) {
      const int64_t n = h_dims[i] * chi_r[0], m = cur_elems[0] / n;
      // tall: one launch for the group
      const int64_t need = n <= m ? gram_batched_need<T>(batch, m, n) : 0;
      if (need > 0 && need <= lay.gram_ws && n * n <= sq) {
        eig_n.assign(batch, n);
        return gram_batched_T(batch, cur.data(), m, n, ws.G, sq, ws.gram_ws, lay.gram_ws, s);
      }
      // wide (n > m, the last sites): A A^T of every volume from two launches
      if (n > m && uniform_small()) {
        BatchOps ops;
        for (int b = 0; b < batch; ++b) ops.in[b] = cur[b];
        const auto pa = strided(ws.A64, lay.wide_elems), pc = strided(ws.G, sq);
        eig_n.assign(batch, m);
        hipLaunchKernelGGL(f32_to_f64_batched_kernel<T>, dim3(grid1d(m * n), batch), dim3(256), 0, s, ops, m * n, ws.A64,
                           lay.wide_elems);
        NDMPS_LAUNCH_CHECK();
        return ndmps_dgemm_batched(batch, 0, 1, m, m, n, pa.data(), n, pa.data(), n, pc.data(), m, s);
      }
    }
    for (int b = 0; b < batch; ++b) {
      const int64_t n = h_dims[i] * chi_r[b], m = cur_elems[b] / n;
      eig_n[b] = std::min(m, n);
      if (n <= m) {
        const int64_t need = gram_need(cur[b], m, n);
        NDMPS_REQUIRE(need <= lay.gram_ws, "internal: Gram workspace bound violated (%lld > %lld)", (long long)need,
                      (long long)lay.gram_ws);
        NDMPS_TRY(gram_T(cur[b], m, n, n, Gb(b), ws.gram_ws, lay.gram_ws, s));
      } else {
        double* Ab = ws.A64 + (int64_t)b * lay.wide_elems;
        hipLaunchKernelGGL(f32_to_f64_kernel<T>, dim3(grid1d(m * n)), dim3(256), 0, s, (const T*)cur[b], m * n, Ab);
        NDMPS_LAUNCH_CHECK();
        NDMPS_TRY(ndmps_dgemm(0, 1, m, m, n, Ab, n, Ab, n, Gb(b), m, s));
      }
    }
    return NDMPS_OK;
  }

  // device ranks of the bond right of site i for the volumes from `base` on, where the cores are cap-shaped and that
  // bond exists; null otherwise (compact cores: every column of the unfolding is inside the rank)
  const int* right_ranks(int i, int base) const {
    return lay.device_rank && ws.d_ranks && i + 1 < L ? ws.d_ranks + (int64_t)(i + 1) * batch + base : nullptr;
  }

  // core of site i and the carried matrix of site i - 1: one launch per step for a uniform group, else volume by volume
  int site_core_and_carry(int i) {
    if (uniform_small() && uniform_kept()) {
      NDMPS_TRY(core_and_carry_uniform(i));
    } else {
      for (int b = 0; b < batch; ++b) NDMPS_TRY(core_and_carry_volume(i, b));
    }
    for (int b = 0; b < batch; ++b) {
      const int64_t m = cur_elems[b] / (h_dims[i] * chi_r[b]);
      std::swap(cur[b], nxt[b]);
      cur_elems[b] = m * kept[b];
      chi_r[b] = kept[b];
      h_bonds_out[(int64_t)b * (L + 1) + i] = kept[b];
    }
    return NDMPS_OK;
  }

  int core_and_carry_uniform(int i) {
    const int64_t n = h_dims[i] * chi_r[0], m = cur_elems[0] / n, small = eig_n[0], k = kept[0];
    BatchOps cores_out, carry_out;
    std::vector<T*> pcore(batch);
    for (int b = 0; b < batch; ++b) {
      pcore[b] = core(b, i);
      cores_out.out[b] = pcore[b];
      carry_out.out[b] = nxt[b];
    }
    if (n <= m) {  // core = V_k^T, carry = A V_k
      hipLaunchKernelGGL(core_from_vectors_batched_kernel<T>, dim3(grid1d(k * n), batch), dim3(256), 0, s,
                         ws.V, sq, n, k, cores_out, right_ranks(i, 0), chi_r[0]);
      NDMPS_LAUNCH_CHECK();
      int rc = NDMPS_OK;
      const bool grouped = gemm_batched_T(batch, 1, m, k, n, cur.data(), pcore.data(), n, nxt.data(), s, &rc);
      NDMPS_TRY(rc);
      for (int b = 0; b < batch && !grouped; ++b)  // bf16 storage: the products go volume by volume
        NDMPS_TRY(gemm_T(1, m, k, n, cur[b], pcore[b], n, nxt[b], ws.tws, lay.transpose_bytes, s));
      return NDMPS_OK;
    }
    const auto pv = strided(ws.V, sq), pa = strided(ws.A64, lay.wide_elems), pu = strided(ws.UtA, lay.wide_elems);
    hipLaunchKernelGGL(sqrt_clamp_batched_kernel, dim3(grid1d(small), batch), dim3(256), 0, s, ws.w,
                       lay.small_max, small, ws.sig);
    hipLaunchKernelGGL(scale_cols_to_f32_batched_kernel<T>, dim3(grid1d(m * k), batch), dim3(256), 0, s, ws.V,
                       sq, m, m, k, ws.sig, lay.small_max, 1.0, carry_out);  // carry = U_k diag(sigma_k)
    NDMPS_LAUNCH_CHECK();
    NDMPS_TRY(ndmps_dgemm_batched(batch, 1, 0, k, n, m, pv.data(), m, pa.data(), n, pu.data(), n, s));
    hipLaunchKernelGGL(scale_rows_to_f32_batched_kernel<T>, dim3(grid1d(k * n), batch), dim3(256), 0, s,
                       ws.UtA, lay.wide_elems, k, n, ws.sig, lay.small_max, -1.0,
                       cores_out);  // core = diag(1/sigma_k) U_k^T A
    NDMPS_LAUNCH_CHECK();
    return NDMPS_OK;
  }

  int core_and_carry_volume(int i, int b) {
    const int64_t n = h_dims[i] * chi_r[b], m = cur_elems[b] / n, small = eig_n[b], k = kept[b];
    const double* sigb = ws.sig + (int64_t)b * lay.small_max;
    if (n <= m) {  // core = V_k^T, carry = A V_k
      hipLaunchKernelGGL(core_from_vectors_kernel<T>, dim3(grid1d(k * n)), dim3(256), 0, s, Vb(b), n, k,
                         core(b, i), right_ranks(i, b), chi_r[b]);
      NDMPS_LAUNCH_CHECK();
      return gemm_T(1, m, k, n, cur[b], core(b, i), n, nxt[b], ws.tws, lay.transpose_bytes, s);
    }
    hipLaunchKernelGGL(sqrt_clamp_kernel, dim3(grid1d(small)), dim3(256), 0, s, ws.w + (int64_t)b * lay.small_max,
                       small, ws.sig + (int64_t)b * lay.small_max);
    hipLaunchKernelGGL(scale_cols_to_f32_kernel<T>, dim3(grid1d(m * k)), dim3(256), 0, s, Vb(b), m, m, k, sigb,
                       1.0, nxt[b]);  // carry = U_k diag(sigma_k)
    NDMPS_LAUNCH_CHECK();
    NDMPS_TRY(ndmps_dgemm(1, 0, k, n, m, Vb(b), m, ws.A64 + (int64_t)b * lay.wide_elems, n, ws.UtA, n, s));
    hipLaunchKernelGGL(scale_rows_to_f32_kernel<T>, dim3(grid1d(k * n)), dim3(256), 0, s, ws.UtA, k, n, sigb,
                       -1.0, core(b, i));  // core = diag(1/sigma_k) U_k^T A
    NDMPS_LAUNCH_CHECK();
    return NDMPS_OK;
  }

  // site 0 carries the norm: (1, d_0, chi_1).  Then the ranks, status words and spectra a device-rank sweep left on the
  // device: read here, or (async) only enqueued towards the caller's pinned buffers (sweep_collect reads them later).
  int finish() {
    for (int b = 0; b < batch; ++b)
      NDMPS_CHECK_HIP(hipMemcpyAsync(core(b, 0), cur[b], cur_elems[b] * sizeof(T), hipMemcpyDeviceToDevice, s));
    if (!lay.device_rank || L <= 1) {
      if (async) {
        ndmps::set_error("an asynchronous sweep needs ranks decided on the device (ndmps_tt_sweep_pads_cores) and more than one site");
        return NDMPS_EINVAL;
      }
      NDMPS_CHECK_HIP(hipStreamSynchronize(s));
      return NDMPS_OK;
    }
    const size_t n_i = (size_t)2 * L * batch, n_s = (size_t)L * batch * lay.spec_stride;
    std::vector<int> host_i(async ? 0 : n_i);
    std::vector<double> host_s(async ? 0 : n_s);
    if (async) NDMPS_REQUIRE(async->h_ranks && (async->h_spec || n_s == 0), "asynchronous sweep without its host buffers");
    int* dst_i = async ? async->h_ranks : host_i.data();
    double* dst_s = async ? async->h_spec : host_s.data();
    NDMPS_CHECK_HIP(hipMemcpyAsync(dst_i, ws.d_ranks, n_i * sizeof(int), hipMemcpyDeviceToHost, s));
    if (n_s) NDMPS_CHECK_HIP(hipMemcpyAsync(dst_s, ws.d_spec, n_s * sizeof(double), hipMemcpyDeviceToHost, s));
    if (async) return NDMPS_OK;  // the caller reads the pinned buffers behind its own synchronisation
    NDMPS_CHECK_HIP(hipStreamSynchronize(s));
    return sweep_collect(batch, L, lay.spec_stride, dst_i, n_s ? dst_s : nullptr, h_bonds_out, h_spectra, h_spec_offsets);
  }
};

template <typename T>
int sweep_impl(int batch, T* const* h_dense, int L, const int64_t* h_dims, double cutoff, int64_t max_bond,
               T* const* h_cores, const int64_t* h_core_offsets, int64_t* h_bonds_out, double* h_spectra,
               const int64_t* h_spec_offsets, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream,
               const SweepSource* src = nullptr, const SweepAsync* async = nullptr) {
  Sweep<T> sw{batch, h_dense, L, h_dims, cutoff, max_bond, h_cores, h_core_offsets, h_bonds_out, h_spectra,
              h_spec_offsets, d_ws, ws_bytes, (hipStream_t)stream, src, async};
  NDMPS_TRY(sw.prepare());
  int i = L - 1;
  if (sw.lay.merge_from < L) {
    NDMPS_TRY(sw.merged_run());
    i = sw.lay.merge_from - 1;
  }
  for (; i >= 1; --i) {
    NDMPS_TRY(sw.site_gram(i));
    NDMPS_TRY(sw.solve_site(i, true));
    NDMPS_TRY(sw.site_core_and_carry(i));
  }
  return sw.finish();
}
}  // namespace

// 1 when the sweep for these site dims and this bond cap decides ranks on the device: cores are then written at
// the layout's offsets in PADDED shape (max_bonds[i], d_i, max_bonds[i+1]) with zeros beyond the actual bonds
// (h_bonds_out), and the caller slices them; 0: cores are compact (bonds[i], d_i, bonds[i+1]).
extern "C" int ndmps_tt_sweep_pads_cores(int L, const int64_t* h_dims, int64_t max_bond) {
  SweepLayout lay;
  if (!h_dims || sweep_layout(L, h_dims, max_bond, 1, lay) != NDMPS_OK) return 0;
  return lay.device_rank ? 1 : 0;
}

extern "C" int ndmps_tt_sweep_batched_f32(int batch, float* const* h_dense, int L, const int64_t* h_dims,
                                          double cutoff, int64_t max_bond, float* const* h_cores,
                                          const int64_t* h_core_offsets, int64_t* h_bonds_out,
                                          double* h_spectra, const int64_t* h_spec_offsets, void* d_ws,
                                          int64_t ws_bytes, ndmps_stream_t stream) {
  return sweep_impl<float>(batch, h_dense, L, h_dims, cutoff, max_bond, h_cores, h_core_offsets, h_bonds_out, h_spectra,
                           h_spec_offsets, d_ws, ws_bytes, stream);
}

// Order of the raw Gram matrix of the merged trailing run when the reshape stage can ride on it (0 otherwise):
// the caller passes ndmps_plan_split_offsets tables for that many columns to the fused sweep.
extern "C" int64_t ndmps_tt_merge_columns(int L, const int64_t* h_dims, int64_t max_bond) {
  SweepLayout lay;
  if (!h_dims || sweep_layout(L, h_dims, max_bond, 1, lay) != NDMPS_OK) return 0;
  if (lay.merge_from >= L || (lay.numel / lay.merge_n) * lay.merge_w > lay.numel / 2) return 0;
  if (lay.merge_n < 64 || lay.numel / lay.merge_n < 256 || lay.merge_n % 4 != 0) return 0;  // wide Gram path only
  return lay.merge_n;
}

// The fp32 sweep reading the C-order VOLUMES through the index permutation (core/ndmps.py:66-71 fused into the
// first Gram pass and the first projection): h_volume[b] are left untouched, no site-order tensor is formed.
// Tables: ndmps_plan_split_offsets for n_cols = ndmps_tt_merge_columns(...), columns sorted by offset
// (d_col_off ascending, in aligned runs of four consecutive offsets; d_col_perm[c] = site-order column).
extern "C" int ndmps_tt_sweep_batched_fused_f32(int batch, const float* const* h_volume, int L, const int64_t* h_dims,
                                                double cutoff, int64_t max_bond, float* const* h_cores,
                                                const int64_t* h_core_offsets, int64_t* h_bonds_out,
                                                double* h_spectra, const int64_t* h_spec_offsets,
                                                const int64_t* d_row_off, const int64_t* d_row_off_sorted,
                                                const int32_t* d_row_order, const int64_t* d_col_off,
                                                const int32_t* d_col_perm, int64_t n_cols, void* d_ws, int64_t ws_bytes,
                                                ndmps_stream_t stream) {
  NDMPS_REQUIRE(d_row_off && d_col_off && d_col_perm && n_cols >= 1, "NULL permutation table");
  SweepSource src{d_row_off, d_row_off_sorted ? d_row_off_sorted : d_row_off, d_row_off_sorted ? d_row_order : nullptr, d_col_off,
                  d_col_perm, n_cols};
  return retry_without_team([&]() {
    return sweep_impl<float>(batch, (float* const*)h_volume, L, h_dims, cutoff, max_bond, h_cores, h_core_offsets,
                             h_bonds_out, h_spectra, h_spec_offsets, d_ws, ws_bytes, stream, &src);
  });
}

// The fused sweep in two halves (device-side ranks only: ndmps_tt_sweep_pads_cores; see SweepAsync above).
//   ..._begin   enqueues the whole sweep and the copies of ranks / status / spectra into the caller's PINNED host buffers
//               (ndmps_tt_sweep_async_ints / _doubles elements); returns without waiting.  h_bonds_scratch: batch (L + 1).
//   ndmps_tt_sweep_finish  once the caller has synchronised with the stream (an event behind _begin): bonds, spectra, or
//               the solver's error -- NDMPS_ETEAM when a resident tridiagonalisation gave up: nothing is repeated here,
//               the caller redoes the batch with ndmps_tt_sweep_batched_fused_f32 (which retries on the column launches).
// Reference: the same from_dense of core/ndmps.py:74; the reference has no counterpart of the split (NumPy is synchronous).
extern "C" int64_t ndmps_tt_sweep_async_ints(int batch, int L) { return (int64_t)2 * L * batch; }
extern "C" int64_t ndmps_tt_sweep_async_doubles(int batch, int L, const int64_t* h_dims, int64_t max_bond) {
  SweepLayout lay;
  if (!h_dims || sweep_layout(L, h_dims, max_bond, batch, lay) != NDMPS_OK) return -1;
  return (int64_t)L * batch * lay.spec_stride;
}
extern "C" int ndmps_tt_sweep_batched_fused_begin_f32(int batch, const float* const* h_volume, int L, const int64_t* h_dims,
                                                      double cutoff, int64_t max_bond, float* const* h_cores,
                                                      const int64_t* h_core_offsets, int64_t* h_bonds_scratch,
                                                      const int64_t* d_row_off, const int64_t* d_row_off_sorted,
                                                      const int32_t* d_row_order, const int64_t* d_col_off,
                                                      const int32_t* d_col_perm, int64_t n_cols, void* d_ws, int64_t ws_bytes,
                                                      int* h_pinned_ranks, double* h_pinned_spec, ndmps_stream_t stream) {
  NDMPS_REQUIRE(d_row_off && d_col_off && d_col_perm && n_cols >= 1, "NULL permutation table");
  NDMPS_REQUIRE(h_pinned_ranks != nullptr, "NULL host buffer");
  SweepSource src{d_row_off, d_row_off_sorted ? d_row_off_sorted : d_row_off, d_row_off_sorted ? d_row_order : nullptr, d_col_off,
                  d_col_perm, n_cols};
  const SweepAsync as{h_pinned_ranks, h_pinned_spec};
  return sweep_impl<float>(batch, (float* const*)h_volume, L, h_dims, cutoff, max_bond, h_cores, h_core_offsets,
                           h_bonds_scratch, nullptr, nullptr, d_ws, ws_bytes, stream, &src, &as);
}
extern "C" int ndmps_tt_sweep_finish(int batch, int L, const int64_t* h_dims, int64_t max_bond, const int* h_pinned_ranks,
                                     const double* h_pinned_spec, int64_t* h_bonds_out, double* h_spectra,
                                     const int64_t* h_spec_offsets) {
  NDMPS_REQUIRE(h_dims && h_pinned_ranks && h_bonds_out && batch >= 1 && L >= 2, "bad sweep_finish argument");
  SweepLayout lay;
  NDMPS_TRY(sweep_layout(L, h_dims, max_bond, batch, lay));
  NDMPS_REQUIRE(lay.device_rank, "this layout decides its ranks on the host: there is nothing to finish");
  return sweep_collect(batch, L, lay.spec_stride, h_pinned_ranks, lay.spec_stride ? h_pinned_spec : nullptr, h_bonds_out,
                       h_spectra, h_spec_offsets);
}

// bf16 storage: the site-order tensors, the carried matrices and the cores are bf16 in HBM; Gram matrices,
// eigen-decompositions and bases stay fp64, products accumulate in fp32 on the bf16 MFMA.  Same layout and
// workspace queries as the fp32 sweep (offsets in elements; the fp32 workspace size is an upper bound).
extern "C" int ndmps_tt_sweep_batched_bf16(int batch, void* const* h_dense, int L, const int64_t* h_dims,
                                           double cutoff, int64_t max_bond, void* const* h_cores,
                                           const int64_t* h_core_offsets, int64_t* h_bonds_out,
                                           double* h_spectra, const int64_t* h_spec_offsets, void* d_ws,
                                           int64_t ws_bytes, ndmps_stream_t stream) {
  return sweep_impl<__bf16>(batch, (__bf16* const*)h_dense, L, h_dims, cutoff, max_bond, (__bf16* const*)h_cores,
                            h_core_offsets, h_bonds_out, h_spectra, h_spec_offsets, d_ws, ws_bytes, stream);
}

// fp64 storage, the reference's own element type (core/ndmps.py:56): volume / site-order tensor, carried matrices and
// cores are fp64 in HBM, every product runs on the fp64 MFMA (ndmps_dgemm), Gram matrices and eigen-decompositions
// are fp64 as in the other storage types.  Workspace: ndmps_tt_sweep_batched_workspace_bytes_f64; layout offsets
// (ndmps_tt_layout) are in elements and shared with the other storage types.  The relative cutoff is clamped below
// at 1e-8 (singular values come from fp64 Gram matrices: sqrt(eps) s_0 is what they resolve).
extern "C" int ndmps_tt_sweep_batched_f64(int batch, double* const* h_dense, int L, const int64_t* h_dims,
                                          double cutoff, int64_t max_bond, double* const* h_cores,
                                          const int64_t* h_core_offsets, int64_t* h_bonds_out,
                                          double* h_spectra, const int64_t* h_spec_offsets, void* d_ws,
                                          int64_t ws_bytes, ndmps_stream_t stream) {
  return sweep_impl<double>(batch, h_dense, L, h_dims, cutoff, max_bond, h_cores, h_core_offsets, h_bonds_out, h_spectra,
                            h_spec_offsets, d_ws, ws_bytes, stream);
}

extern "C" int ndmps_tt_sweep_f32(float* d_dense, int L, const int64_t* h_dims, double cutoff,
                                  int64_t max_bond, float* d_cores, const int64_t* h_core_offsets,
                                  int64_t* h_bonds_out, double* h_spectra, const int64_t* h_spec_offsets,
                                  void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  NDMPS_REQUIRE(d_dense && d_cores, "NULL sweep argument");
  float* dense[1] = {d_dense};
  float* cores[1] = {d_cores};
  return ndmps_tt_sweep_batched_f32(1, dense, L, h_dims, cutoff, max_bond, cores, h_core_offsets, h_bonds_out,
                                    h_spectra, h_spec_offsets, d_ws, ws_bytes, stream);
}

// =================================================================== bond truncation
namespace {
// eigen workspace of compress_bond: the block Jacobi's, and the direct solver's for every eigenpair where it applies
inline int64_t bond_eig_bytes(int64_t chi) {
  const int64_t jac = ndmps_syevj_workspace_bytes(chi);
  return use_direct_full(chi, 1, 0) ? std::max(jac, ndmps_syevd_topk_workspace_bytes(chi, 1, chi)) : jac;
}

// The workspace of compress_bond for cores (m1, chi) and (chi, n2), piece by piece: the size query carves an arena
// without memory, compress_bond_impl the caller's.
struct BondBuffers {
  double *G1, *G2;       // T1^T T1; T2 T2^T (destroyed)
  ndmps::GramTrunc g;    // the buffers of the truncation itself: Lt, tmp, H, V, P1, w2, wh, sig and the eigen workspace
  double* P2;            // tmp V
  double *A1, *B2;       // the two factors in the storage type (chi^2 doubles each, whatever the type)
  double* t2d;           // T2 in fp64
  char* gram_ws;
  int64_t gram_bytes;
};
void carve_bond(Arena& ar, int64_t m1, int64_t chi, int64_t n2, BondBuffers& b) {
  const int64_t c2 = chi * chi;
  ndmps::GramTrunc& g = b.g;
  g.chi = chi;
  b.G1 = ar.take<double>(c2);
  b.G2 = ar.take<double>(c2);
  g.Lt = ar.take<double>(c2);
  g.tmp = ar.take<double>(c2);
  g.H = ar.take<double>(c2);
  g.V = ar.take<double>(c2);
  g.P1 = ar.take<double>(c2);
  b.P2 = ar.take<double>(c2);
  g.w2 = ar.take<double>(chi);
  g.wh = ar.take<double>(chi);
  g.sig = ar.take<double>(chi);
  b.A1 = ar.take<double>(c2);
  b.B2 = ar.take<double>(c2);
  b.t2d = ar.take<double>(chi * n2);
  g.ev_bytes = bond_eig_bytes(chi);
  g.ev_ws = ar.take<char>(g.ev_bytes);
  b.gram_bytes = std::max(ndmps_gram_workspace_bytes(m1, chi), ndmps_gram_f64_workspace_bytes(m1, chi));
  b.gram_ws = ar.take<char>(b.gram_bytes);
}
}  // namespace

// ------------------------------------------------------------- truncation from two Gram matrices (trunc.h)
int64_t ndmps::gram_trunc_eig_bytes(int64_t chi) { return bond_eig_bytes(chi); }

template <typename T>
int ndmps::gram_truncate(const GramTrunc& g, double* Gf, const double* Gd, const T* data, int64_t rows, int64_t rs,
                         int64_t cs, double cutoff, double floor, double abs_thr, int64_t max_bond, bool f64_tails,
                         bool cap_decides, int64_t* k_out, double* h_s, hipStream_t s) {
  const int64_t chi = g.chi, c2 = chi * chi;
  double *Lt = g.Lt, *tmp = g.tmp, *H = g.H, *V = g.V, *P1 = g.P1, *w2 = g.w2, *wh = g.wh;
  char* ev_ws = g.ev_ws;
  const int64_t ev_bytes = g.ev_bytes;
  int sweeps = 0;
  // Both decompositions on the direct solver where it applies (every eigenpair of Gf for its square root; of H the
  // eigenvalues, then only the kept vectors), the block Jacobi otherwise -- and for H whenever the solver's own noise
  // could move the rank (direct_rank_is_safe).
  const bool direct = use_direct_full(chi, 1, 0);
  const int64_t n1[1] = {chi};
  auto direct_values = [&](const double* M, double* vecs, double* vals) -> int {
    NDMPS_TRY(ndmps_syevd_topk_values_f64(1, M, c2, n1, vecs, c2, vals, chi, chi, ev_ws, ev_bytes, s));
    return ndmps_syevd_topk_recover_f64(1, n1, chi, ev_ws, ev_bytes, nullptr, s);
  };
  auto direct_vectors = [&](int64_t kv, bool& ok) -> int {  // ok = false: the block lost rank, the caller takes the Jacobi
    const int64_t k1[1] = {kv};
    int status = 0;
    NDMPS_TRY(ndmps_syevd_topk_vectors_f64(1, n1, k1, chi, ev_ws, ev_bytes, &status, s));
    if (status == 2) return solver_failed(-1, 0, status);
    ok = status == 0;
    return NDMPS_OK;
  };
  // Square root of Gf: any Lt with Lt Lt^T = Gf serves (H = Lt^T Gd Lt has the singular values squared whatever the
  // factor, and Lt V_k, Gd Lt V_k do not depend on it).  The Cholesky factor where Gf is numerically positive definite
  // -- in compress_bond the cores to the right of the bond are isometries until compress() reaches them: Gf = I +
  // rounding, a chi-fold eigenvalue, the worst case of an eigen-solver and the best of a Cholesky --, else W D^(1/2)
  // from the eigen-decomposition (zero eigenvalues give zero columns).
  bool g2_chol = direct && !getenv("NDMPS_COMPRESS_EIG") && ndmps_potrf_scratch_elems(chi) <= 2 * c2;
  if (g2_chol) {
    NDMPS_CHECK_HIP(hipMemcpyAsync(Lt, Gf, sizeof(double) * c2, hipMemcpyDeviceToDevice, s));
    int bad = 0;
    NDMPS_TRY(ndmps_potrf_lower_f64(Lt, chi, tmp, &bad, s));  // tmp and H (adjacent, 2 c2 doubles) are free until Lt is known
    g2_chol = bad == 0;
  }
  if (!g2_chol) {
    bool g2_direct = direct;
    if (g2_direct) {
      NDMPS_TRY(direct_values(Gf, Lt, w2));
      NDMPS_TRY(direct_vectors(chi, g2_direct));
    }
    if (!g2_direct) NDMPS_TRY(ndmps_syevj_f64(Gf, chi, Lt, w2, ev_ws, ev_bytes, &sweeps, s));
    // a singular Gf (rank-deficient factor) has eigenvalues of ~kDirectDoubt |Gf| where it has zeros: their square
    // roots would be columns of ~3e-7 |F| pointing anywhere, spurious singular values
    hipLaunchKernelGGL(scale_cols_sqrt_kernel, dim3(grid1d(c2)), dim3(256), 0, s, Lt, chi, chi, w2, kDirectDoubt);
    NDMPS_LAUNCH_CHECK();
  }
  NDMPS_TRY(ndmps_dgemm(0, 0, chi, chi, chi, Gd, chi, Lt, chi, tmp, chi, s));
  NDMPS_TRY(ndmps_dgemm(1, 0, chi, chi, chi, Lt, chi, tmp, chi, H, chi, s));
  std::vector<double> sv(chi);
  auto fetch = [&]() -> int {
    NDMPS_CHECK_HIP(hipMemcpyAsync(sv.data(), wh, chi * sizeof(double), hipMemcpyDeviceToHost, s));
    NDMPS_CHECK_HIP(hipStreamSynchronize(s));
    return NDMPS_OK;
  };
  bool h_direct = direct;
  if (h_direct) NDMPS_TRY(direct_values(H, V, wh));  // the solver symmetrises its copy of H
  else NDMPS_TRY(ndmps_syevj_f64(H, chi, V, wh, ev_ws, ev_bytes, &sweeps, s));  // symmetrises H on entry
  NDMPS_TRY(fetch());
  // the relative threshold; an absolute one (abs_thr >= 0, 0 included) raises it, or leaves nothing to keep
  double c = std::max(cutoff, floor);
  if (abs_thr >= 0.0) {
    const double s0 = sqrt(std::max(sv[0], 0.0));
    if (!(s0 > abs_thr)) {
      for (auto& x : sv) x = sqrt(std::max(x, 0.0));
      if (h_s) memcpy(h_s, sv.data(), chi * sizeof(double));
      *k_out = 0;
      return NDMPS_OK;
    }
    c = std::max(c, abs_thr / s0);
  }
  const int64_t limit = max_bond > 0 ? std::min(max_bond, chi) : chi;
  // cap_decides: a rank fixed by the cap -- `limit` eigenvalues clearly above the threshold -- needs no decision there
  bool safe = direct_rank_is_safe(sv.data(), chi, c);
  if (!safe && cap_decides && limit < chi) {
    const double clear = c * c * sv[0] + kDirectDoubt * fabs(sv[0]);
    safe = sv[limit - 1] > clear;
  }
  if (h_direct && !safe) {
    h_direct = false;
    NDMPS_TRY(ndmps_syevj_f64(H, chi, V, wh, ev_ws, ev_bytes, &sweeps, s));
    NDMPS_TRY(fetch());
  }
  // fp64 cores: H carries s^2, so a zero comes back at ~sqrt(n u) s_0 -- on kCutoffFloorF64 itself -- and the eigenvalues
  // in doubt (direct_doubt_from) cannot decide the rank.  Those below the cap are measured directly, s_j = |data Lt v_j|
  // (H = (data Lt)^T (data Lt)), whose noise is ~u |data| |Lt|, as the sweep measures its tail norms (Sweep::measure_doubt); they replace the
  // squared values in the rank and in the caller's scalings.  fp32 and bf16 cores: the floor (1e-6) is far above the noise.
  // (k is 1 whatever the values when at most one may be kept; from chi = 2 on, one row block fits H: 2 t <= chi^2)
  if (f64_tails && limit > 1 && direct_doubt_from(sv.data(), chi, c) < limit) {
    if (h_direct) {  // every vector is needed: the Jacobi computes them all (same spectrum)
      NDMPS_TRY(ndmps_syevj_f64(H, chi, V, wh, ev_ws, ev_bytes, &sweeps, s));
      NDMPS_TRY(fetch());
      h_direct = false;
    }
    const int64_t i0 = direct_doubt_from(sv.data(), chi, c), t = chi - i0;
    if (i0 < limit) {
      NDMPS_TRY(ndmps_dgemm(0, 0, chi, chi, chi, Lt, chi, V, chi, P1, chi, s));  // Lt V
      double* out = nullptr;  // partials and sums in H, free now
      NDMPS_TRY(tail_norms(data, rs, cs, rows, chi, P1, chi, i0, t, H, c2, &out, s));
      NDMPS_CHECK_HIP(hipMemcpyAsync(wh + i0, out, t * sizeof(double), hipMemcpyDeviceToDevice, s));
      NDMPS_CHECK_HIP(hipMemcpyAsync(sv.data() + i0, out, t * sizeof(double), hipMemcpyDeviceToHost, s));
      NDMPS_CHECK_HIP(hipStreamSynchronize(s));
    }
  }
  for (auto& x : sv) x = sqrt(std::max(x, 0.0));  // eigenvalues of H are s^2 (measured |data Lt v_j|^2 in doubt)
  const int64_t k = kept_rank(sv, c, max_bond, floor);
  if (h_direct) {
    NDMPS_TRY(direct_vectors(k, h_direct));
    if (!h_direct) NDMPS_TRY(ndmps_syevj_f64(H, chi, V, wh, ev_ws, ev_bytes, &sweeps, s));  // same spectrum, same k
  }
  if (h_s) memcpy(h_s, sv.data(), chi * sizeof(double));
  *k_out = k;
  hipLaunchKernelGGL(sqrt_clamp_kernel, dim3(grid1d(chi)), dim3(256), 0, s, wh, chi, g.sig);
  NDMPS_LAUNCH_CHECK();
  return NDMPS_OK;
}
template int ndmps::gram_truncate<float>(const GramTrunc&, double*, const double*, const float*, int64_t, int64_t,
                                         int64_t, double, double, double, int64_t, bool, bool, int64_t*, double*, hipStream_t);
template int ndmps::gram_truncate<double>(const GramTrunc&, double*, const double*, const double*, int64_t, int64_t,
                                          int64_t, double, double, double, int64_t, bool, bool, int64_t*, double*, hipStream_t);


extern "C" int64_t ndmps_compress_bond_workspace_bytes(int64_t chi_l, int64_t d1, int64_t chi, int64_t d2,
                                                       int64_t chi_r) {
  if (chi_l <= 0 || d1 <= 0 || chi <= 0 || d2 <= 0 || chi_r <= 0) return 0;
  Arena sizing(nullptr, 0);
  BondBuffers unused;
  carve_bond(sizing, chi_l * d1, chi, d2 * chi_r, unused);
  return ndmps::round_up(sizing.used, 256) + 256;
}

// Truncated SVD of the two-site product P = T1 T2 through the bond, without forming P or
// Q factors: with G1 = T1^T T1, G2 = T2 T2^T = W D W^T, Lt = W D^(1/2) and H = Lt^T G1 Lt
// = V diag(s^2) V^T (the s are the singular values of P), the absorb-"both" cores are
//   T1' = T1 (Lt V_k) s_k^(-1/2),   T2' = s_k^(-3/2) (G1 Lt V_k)^T T2 .
namespace {
template <typename T>
int compress_bond_impl(const T* d_t1, const T* d_t2, int64_t chi_l, int64_t d1, int64_t chi, int64_t d2, int64_t chi_r,
                       double cutoff, int64_t max_bond, T* d_new1, T* d_new2, int64_t* h_new_chi, double* h_s, void* d_ws,
                       int64_t ws_bytes, ndmps_stream_t stream) {
  NDMPS_REQUIRE(d_t1 && d_t2 && d_new1 && d_new2 && h_new_chi, "NULL compress_bond argument");
  NDMPS_REQUIRE(chi_l > 0 && d1 > 0 && chi > 0 && d2 > 0 && chi_r > 0, "bad core shape");
  NDMPS_REQUIRE(cutoff >= 0.0, "cutoff must be non-negative");
  const int64_t need = ndmps_compress_bond_workspace_bytes(chi_l, d1, chi, d2, chi_r);
  if (!d_ws || ws_bytes < need) {
    ndmps::set_error("compress_bond workspace too small: %lld < %lld", (long long)ws_bytes, (long long)need);
    return NDMPS_EWORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const int64_t m1 = chi_l * d1, n2 = d2 * chi_r;
  Arena ar(d_ws, ws_bytes);
  BondBuffers w;
  carve_bond(ar, m1, chi, n2, w);
  NDMPS_REQUIRE(ar.fits(), "workspace carve failed");
  T *A1 = reinterpret_cast<T*>(w.A1), *B2 = reinterpret_cast<T*>(w.B2);
  double *Lt = w.g.Lt, *tmp = w.g.tmp, *V = w.g.V, *P1 = w.g.P1, *P2 = w.P2, *sig = w.g.sig;

  NDMPS_TRY(gram_T(d_t1, m1, chi, chi, w.G1, w.gram_ws, w.gram_bytes, s));
  hipLaunchKernelGGL(f32_to_f64_kernel<T>, dim3(grid1d(chi * n2)), dim3(256), 0, s, d_t2, chi * n2, w.t2d);
  NDMPS_LAUNCH_CHECK();
  NDMPS_TRY(ndmps_dgemm(0, 1, chi, chi, n2, w.t2d, n2, w.t2d, n2, w.G2, chi, s));
  // G2 = T2 T2^T is the square-rooted metric, G1 = T1^T T1 the data Gram; tail norms measured on the rows of T1
  int64_t k = 0;
  NDMPS_TRY(ndmps::gram_truncate<T>(w.g, w.G2, w.G1, d_t1, m1, chi, 1, cutoff, cutoff_floor<T>(), -1.0, max_bond, sizeof(T) == 8,
                                    false, &k, h_s, s));
  *h_new_chi = k;
  NDMPS_TRY(ndmps_dgemm(0, 0, chi, k, chi, Lt, chi, V, chi, P1, k, s));
  NDMPS_TRY(ndmps_dgemm(0, 0, chi, k, chi, tmp, chi, V, chi, P2, k, s));
  hipLaunchKernelGGL(scale_cols_to_f32_kernel<T>, dim3(grid1d(chi * k)), dim3(256), 0, s, P1, chi, k, k, sig, -0.5, A1);
  hipLaunchKernelGGL(scale_cols_to_f32_kernel<T>, dim3(grid1d(chi * k)), dim3(256), 0, s, P2, chi, k, k, sig, -1.5, B2);
  NDMPS_LAUNCH_CHECK();
  NDMPS_TRY(gemm_any(0, 0, m1, k, chi, d_t1, chi, A1, k, d_new1, k, s));      // (chi_l d1, k)
  NDMPS_TRY(gemm_any(1, 0, k, n2, chi, B2, k, d_t2, n2, d_new2, n2, s));      // (k, d2 chi_r)
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));
  return NDMPS_OK;
}
}  // namespace

extern "C" int ndmps_compress_bond_f32(const float* d_t1, const float* d_t2, int64_t chi_l, int64_t d1,
                                       int64_t chi, int64_t d2, int64_t chi_r, double cutoff,
                                       int64_t max_bond, float* d_new1, float* d_new2, int64_t* h_new_chi,
                                       double* h_s, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  return compress_bond_impl<float>(d_t1, d_t2, chi_l, d1, chi, d2, chi_r, cutoff, max_bond, d_new1, d_new2, h_new_chi, h_s,
                                   d_ws, ws_bytes, stream);
}
// fp64 cores (same workspace query)
extern "C" int ndmps_compress_bond_f64(const double* d_t1, const double* d_t2, int64_t chi_l, int64_t d1,
                                       int64_t chi, int64_t d2, int64_t chi_r, double cutoff,
                                       int64_t max_bond, double* d_new1, double* d_new2, int64_t* h_new_chi,
                                       double* h_s, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  return compress_bond_impl<double>(d_t1, d_t2, chi_l, d1, chi, d2, chi_r, cutoff, max_bond, d_new1, d_new2, h_new_chi, h_s,
                                    d_ws, ws_bytes, stream);
}
