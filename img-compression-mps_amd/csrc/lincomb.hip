// TT rounding of a weighted sum of MPS (core/lincomb.py, NDMPS.linear_combination / recompress): the TT-SVD
// truncation of  S = sum_a w_a X^a  computed on the cores, without the sum's block cores or a volume.
//
// The formal sum chain has S_0 = [w_1 X^1_0 | ... | w_K X^K_0], block-diagonal middle sites and the last sites
// stacked.  Sigma_k = sum_a chi_{a,k} is its bond k.
//   1. Left Grams.  GL_0 = w w^T (K x K, every chi_{a,0} = 1); for every pair a <= b and site j
//        GL_{j+1}[a, b] = sum_i X^a_j[:, i, :]^T GL_j[a, b] X^b_j[:, i, :]
//      in two ragged launches per site: Z_ab = GL_j[a, b] X^b_j, then GL_{j+1}[a, b] = (X^a_j)^T Z_ab with the
//      transposed block mirrored into [b, a].  The weights ride in GL_0, so every block comes out weighted.
//   2. Right-to-left sweep, k = L-1 .. 1, carried core C_k (Sigma_k x d_k r_{k+1}, fp64; C_{L-1} = the last sites):
//        G2 = C_k C_k^T,  GL_k = Lt Lt^T,  H = Lt^T G2 Lt = V diag(s^2) V^T          (gram_truncate, trunc.h)
//        site k = diag(1/s) (Lt V_r)^T C_k          (rows orthonormal: the result is right-isometric)
//        P = G2 Lt V_r diag(1/s)                    (Sigma_k x r_k)
//        C_{k-1}[block a] = X^a_{k-1} x_3 P_a       (one ragged launch; at k-1 = 0 the blocks are summed with w)
//      Kept: s_j > max(cutoff s_0, floor scale), floor 1e-6 (fp32 work) or 1e-8 (fp64 work), at most max_bond and
//      min(prod_{j<k} d_j, d_k r_{k+1}); nothing kept at some bond -> the zero MPS (every bond 1, zero cores).
// The ragged products are 64 x 64 fp64 tiles of FMA from LDS; the input cores are read in their storage type
// (fp32, bf16, fp64) through a task table built on the host and uploaded once with the weights and GL_0.
// Departure from the planned design: the pair transfer was to be one launch per site on v_mfma_f64_16x16x4_f64; it is
// two launches per site (Z, then GL) of this vector-FMA kernel.  Measured at 0.81 ms of 19.1 ms of device time for a
// mean of 8 x 256^3 chi=64, where the eigen-solves take 16.7 ms, so the MFMA kernel is not built.
#include <math.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "common.h"
#include "trunc.h"

namespace {

using ndmps::Arena;
using ndmps::ceil_div;
using ndmps::load_any;

constexpr int kTile = 64, kTk = 16;

// one ragged product C (M x N) = op(A) (M x K) B (K x N); A, B in a storage type (code 0 fp32, 1 bf16, 2 fp64)
struct Task {
  const void* A;
  const void* B;
  double* C;
  double* Cm;  // != nullptr: C^T is written there too (row stride ldc)
  int64_t M, N, K, lda, ldb, ldc;
  int64_t brow, crow;  // projection launches: B = Pbase + brow r, C = Cbase + crow r, N = ldb = ldc = r
  int32_t a_code, b_code, transA, pad;
};

// blockIdx.y = task, blockIdx.x = 64 x 64 output tile; 256 threads, 4 x 4 outputs each (rows ty + 16 i,
// columns tx + 16 j).  A task or tile outside its range does nothing.
template <bool kProj>
__global__ void __launch_bounds__(256)
ragged_gemm_kernel(const Task* __restrict__ tasks, int ntasks, const double* __restrict__ Pbase, double* __restrict__ Cbase,
                   int64_t r) {
  if ((int)blockIdx.y >= ntasks) return;
  const Task t = tasks[blockIdx.y];
  const int64_t M = t.M, K = t.K;
  const int64_t N = kProj ? r : t.N, ldb = kProj ? r : t.ldb, ldc = kProj ? r : t.ldc;
  const void* B = kProj ? (const void*)(Pbase + t.brow * r) : t.B;
  double* C = kProj ? Cbase + t.crow * r : t.C;
  const int bcode = kProj ? 2 : t.b_code;
  if (M <= 0 || N <= 0 || K < 0 || !t.A || !B || !C) return;
  const int64_t tiles_n = (N + kTile - 1) / kTile;
  if ((int64_t)blockIdx.x >= (M + kTile - 1) / kTile * tiles_n) return;
  const int64_t m0 = (blockIdx.x / tiles_n) * kTile, n0 = (blockIdx.x % tiles_n) * kTile;

  __shared__ double As[kTk][kTile + 1];
  __shared__ double Bs[kTk][kTile + 1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;

  for (int64_t k0 = 0; k0 < K; k0 += kTk) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = tid + 256 * q;
      int ml, kl;
      if (t.transA) { kl = e / kTile; ml = e % kTile; }  // A[k lda + m]: consecutive m
      else { ml = e / kTk; kl = e % kTk; }               // A[m lda + k]: consecutive k
      const int64_t m = m0 + ml, k = k0 + kl;
      double v = 0.0;
      if (m < M && k < K) v = load_any(t.A, t.a_code, t.transA ? k * t.lda + m : m * t.lda + k);
      As[kl][ml] = v;
      const int kb = e / kTile, nb = e % kTile;
      const int64_t kk = k0 + kb, n = n0 + nb;
      Bs[kb][nb] = (kk < K && n < N) ? load_any(B, bcode, kk * ldb + n) : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kTk; ++kk) {
      double a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = As[kk][ty + 16 * i];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = Bs[kk][tx + 16 * j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + ty + 16 * i;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t n = n0 + tx + 16 * j;
      if (n >= N) continue;
      C[m * ldc + n] = acc[i][j];
      if (!kProj && t.Cm) t.Cm[n * ldc + m] = acc[i][j];
    }
  }
}

// out (k x n, storage type) <- rows of Y (k x n fp64) divided by s
template <typename T>
__global__ void __launch_bounds__(256)
rows_over_s_kernel(const double* __restrict__ Y, int64_t k, int64_t n, const double* __restrict__ s, T* __restrict__ out) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < k * n; e += (int64_t)gridDim.x * 256)
    out[e] = ndmps::from_f64<T>(Y[e] / s[e / n]);
}
// M (rows x k fp64) columns divided by s, in place
__global__ void __launch_bounds__(256) cols_over_s_kernel(double* __restrict__ M, int64_t rows, int64_t k,
                                                          const double* __restrict__ s) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < rows * k; e += (int64_t)gridDim.x * 256)
    M[e] /= s[e % k];
}
// site 0: out (n) = sum_a w_a Cst[a n + i]  (the K stacked blocks of the last projection)
template <typename T>
__global__ void __launch_bounds__(256)
weighted_sum_kernel(const double* __restrict__ Cst, int K, int64_t n, const double* __restrict__ w, T* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    double acc = 0.0;
    for (int a = 0; a < K; ++a) acc = fma(w[a], Cst[(int64_t)a * n + i], acc);
    out[i] = ndmps::from_f64<T>(acc);
  }
}
template <typename T>
__global__ void __launch_bounds__(256) zero_kernel(T* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = T(0);
}

using ndmps::grid1d;

// Host plan: bond sums, block offsets, output bounds and the workspace carve (a null arena counts bytes).
struct Plan {
  int K = 0, L = 0;
  std::vector<int64_t> dims, bonds;      // bonds: K x (L + 1), row a = input a
  std::vector<int64_t> S, off;           // S[j] = sum_a chi_{a,j}; off[a (L + 1) + j] = block offset of a at bond j
  std::vector<int64_t> ub, out_off;      // ub[j]: output bond bound; out_off[j]: site j's offset in the output arena
  std::vector<int64_t> left;             // prod_{i<j} d_i (saturating)
  int64_t smax = 1, zmax = 1, cmax = 1, ymax = 1, eig = 0, ntransfer = 0;
  int64_t chi(int a, int j) const { return bonds[(size_t)a * (L + 1) + j]; }
};

int make_plan(int K, int L, const int64_t* h_dims, const int64_t* h_bonds, int64_t max_bond, Plan& p) {
  NDMPS_REQUIRE(K >= 1 && L >= 1 && h_dims && h_bonds, "bad lincomb argument (K = %d, L = %d)", K, L);
  p.K = K;
  p.L = L;
  p.dims.assign(h_dims, h_dims + L);
  p.bonds.assign(h_bonds, h_bonds + (size_t)K * (L + 1));
  for (int j = 0; j < L; ++j) NDMPS_REQUIRE(p.dims[j] >= 1, "site %d: bad physical dim %lld", j, (long long)p.dims[j]);
  p.S.assign(L + 1, 0);
  p.off.assign((size_t)K * (L + 1), 0);
  for (int a = 0; a < K; ++a) {
    NDMPS_REQUIRE(p.chi(a, 0) == 1 && p.chi(a, L) == 1, "input %d: the outer bonds must be 1", a);
    for (int j = 0; j <= L; ++j) {
      NDMPS_REQUIRE(p.chi(a, j) >= 1 && p.chi(a, j) <= ndmps_syevd_topk_max_n(), "input %d, bond %d: bad bond %lld", a, j,
                    (long long)p.chi(a, j));
      p.off[(size_t)a * (L + 1) + j] = p.S[j];
      p.S[j] += p.chi(a, j);
    }
  }
  for (int j = 1; j < L; ++j)
    NDMPS_REQUIRE(p.S[j] <= ndmps_syevd_topk_max_n(),
                  "bond %d: the summed bond %lld exceeds %lld; recompress the inputs first", j, (long long)p.S[j],
                  (long long)ndmps_syevd_topk_max_n());
  p.left.assign(L + 1, 1);
  const int64_t big = std::numeric_limits<int64_t>::max() / 4;
  for (int j = 1; j <= L; ++j) p.left[j] = std::min(big, p.left[j - 1] * p.dims[j - 1]);
  p.ub.assign(L + 1, 1);
  for (int j = L - 1; j >= 1; --j) {
    int64_t u = std::min({p.S[j], p.left[j], p.dims[j] * p.ub[j + 1]});
    if (max_bond > 0) u = std::min(u, max_bond);
    p.ub[j] = std::max<int64_t>(u, 1);
  }
  p.out_off.assign(L + 1, 0);
  for (int j = 0; j < L; ++j) p.out_off[j + 1] = p.out_off[j] + p.ub[j] * p.dims[j] * p.ub[j + 1];
  p.smax = 1;
  p.eig = 0;
  for (int j = 1; j < L; ++j) {
    p.smax = std::max(p.smax, p.S[j]);
    p.eig = std::max(p.eig, ndmps::gram_trunc_eig_bytes(p.S[j]));
  }
  p.zmax = 1;
  p.ntransfer = 0;
  for (int j = 0; j + 1 < L; ++j) {
    int64_t z = 0;
    for (int a = 0; a < K; ++a)
      for (int b = a; b < K; ++b) z += p.chi(a, j) * p.dims[j] * p.chi(b, j + 1);
    p.zmax = std::max(p.zmax, z);
    p.ntransfer += (int64_t)K * (K + 1);  // two tasks per pair
  }
  // carried cores: C_j is S_j x d_j r_{j+1} (S_0 = K: site 0's blocks are stacked before the weighted sum)
  p.cmax = 1;
  p.ymax = 1;
  for (int j = 0; j < L; ++j) {
    p.cmax = std::max(p.cmax, (j == 0 ? (int64_t)K : p.S[j]) * p.dims[j] * p.ub[j + 1]);
    p.ymax = std::max(p.ymax, p.ub[j] * p.dims[j] * p.ub[j + 1]);
  }
  return NDMPS_OK;
}

struct Buffers {
  std::vector<double*> GL;  // GL[j], S_j^2 (GL[0] = w w^T, K^2)
  double *Z, *C[2], *G2, *P2, *Y, *wts, *ones;
  ndmps::GramTrunc g;
  Task* tasks;
};

// carve in a fixed order; with a null arena only the byte count (ar.used) is meaningful
void carve(const Plan& p, Arena& ar, Buffers& b) {
  const int64_t s2 = p.smax * p.smax;
  b.GL.assign(p.L, nullptr);
  b.GL[0] = ar.take<double>((int64_t)p.K * p.K);
  for (int j = 1; j < p.L; ++j) b.GL[j] = ar.take<double>(p.S[j] * p.S[j]);
  b.Z = ar.take<double>(p.zmax);
  b.C[0] = ar.take<double>(p.cmax);
  b.C[1] = ar.take<double>(p.cmax);
  b.G2 = ar.take<double>(s2);
  b.g.Lt = ar.take<double>(s2);
  b.g.tmp = ar.take<double>(s2);  // tmp then H: the Cholesky scratch
  b.g.H = ar.take<double>(s2);
  b.g.V = ar.take<double>(s2);
  b.g.P1 = ar.take<double>(s2);
  b.P2 = ar.take<double>(s2);
  b.Y = ar.take<double>(p.ymax);
  b.g.w2 = ar.take<double>(p.smax);
  b.g.wh = ar.take<double>(p.smax);
  b.g.sig = ar.take<double>(p.smax);
  b.wts = ar.take<double>(p.K);
  b.ones = ar.take<double>(p.K);
  b.tasks = ar.take<Task>(p.ntransfer + (int64_t)p.K * p.L);
  b.g.ev_bytes = std::max<int64_t>(p.eig, 1);
  b.g.ev_ws = ar.take<char>(b.g.ev_bytes);
}

// tasks [first, first + count) of the table, one per blockIdx.y, in launches of at most kMaxTasksPerLaunch tasks
// (gridDim.y <= 65535): K inputs give K (K + 1) / 2 pair tasks, above 65535 from K = 362 on
constexpr int64_t kMaxTasksPerLaunch = 65535;

int launch_tasks(const Task* d_tasks, const std::vector<Task>& h, int64_t first, int64_t count, bool proj,
                 const double* Pbase, double* Cbase, int64_t r, hipStream_t s) {
  for (int64_t c0 = first; c0 < first + count; c0 += kMaxTasksPerLaunch) {
    const int64_t n_tasks = std::min(kMaxTasksPerLaunch, first + count - c0);
    int64_t tiles = 1;
    for (int64_t i = c0; i < c0 + n_tasks; ++i) {
      const int64_t n = proj ? r : h[i].N;
      tiles = std::max(tiles, ceil_div(h[i].M, kTile) * ceil_div(n, kTile));
    }
    NDMPS_REQUIRE(tiles <= INT32_MAX, "internal: ragged launch too large");
    if (proj)
      hipLaunchKernelGGL(ragged_gemm_kernel<true>, dim3((unsigned)tiles, (unsigned)n_tasks), dim3(256), 0, s,
                         d_tasks + c0, (int)n_tasks, Pbase, Cbase, r);
    else
      hipLaunchKernelGGL(ragged_gemm_kernel<false>, dim3((unsigned)tiles, (unsigned)n_tasks), dim3(256), 0, s,
                         d_tasks + c0, (int)n_tasks, (const double*)nullptr, (double*)nullptr, (int64_t)0);
    NDMPS_LAUNCH_CHECK();
  }
  return NDMPS_OK;
}

template <typename TO>
int lincomb_impl(const Plan& p, const int* h_codes, const void* const* h_cores, const double* h_w, double cutoff,
                 int64_t max_bond, double scale, TO* d_out, int64_t out_elems, int64_t* h_out_bonds, double* h_spectra,
                 int64_t spec_stride, void* d_ws, int64_t ws_bytes, hipStream_t s) {
  const int K = p.K, L = p.L;
  NDMPS_REQUIRE(d_out && out_elems >= p.out_off[L], "output arena too small: %lld < %lld", (long long)out_elems,
                (long long)p.out_off[L]);
  NDMPS_REQUIRE(h_out_bonds && (L == 1 || (h_spectra && spec_stride >= p.smax)), "bad lincomb output argument");
  for (int a = 0; a < K; ++a) {
    NDMPS_REQUIRE(h_codes[a] >= 0 && h_codes[a] <= 2, "input %d: bad dtype code %d", a, h_codes[a]);
    NDMPS_REQUIRE(std::isfinite(h_w[a]), "input %d: non-finite weight", a);
    for (int j = 0; j < L; ++j) NDMPS_REQUIRE(h_cores[(size_t)a * L + j], "input %d, site %d: NULL core", a, j);
  }
  NDMPS_REQUIRE(cutoff >= 0.0 && std::isfinite(scale) && scale >= 0.0, "bad cutoff or scale");
  Arena ar(d_ws, ws_bytes);
  Buffers b;
  carve(p, ar, b);
  if (!ar.fits()) {
    ndmps::set_error("lincomb workspace too small: %lld < %lld", (long long)ws_bytes, (long long)ar.used);
    return NDMPS_EWORKSPACE;
  }
  auto core = [&](int a, int j) { return h_cores[(size_t)a * L + j]; };
  auto offs = [&](int a, int j) { return p.off[(size_t)a * (L + 1) + j]; };
  const bool f64 = sizeof(TO) == 8;
  const double floor = f64 ? 1e-8 : 1e-6;

  // ---- tasks: every site's transfer products, then every site's projections; one upload with w, 1 and GL_0
  std::vector<Task> tasks;
  tasks.reserve(p.ntransfer + (size_t)K * L);
  for (int j = 0; j + 1 < L; ++j) {  // site j: the pairs' Z products, then their GL products
    std::vector<Task> second;
    const int64_t d = p.dims[j], Sj = j == 0 ? K : p.S[j], Sn = p.S[j + 1];
    int64_t z = 0;
    for (int a = 0; a < K; ++a)
      for (int c = a; c < K; ++c) {
        const int64_t ca = p.chi(a, j), cb = p.chi(c, j), ca2 = p.chi(a, j + 1), cb2 = p.chi(c, j + 1);
        const int64_t ra = j == 0 ? a : offs(a, j), rc = j == 0 ? c : offs(c, j);
        Task t1{};  // Z (ca x d cb2) = GL_j[a, c] (ca x cb) X^c_j (cb x d cb2)
        t1.A = b.GL[j] + ra * Sj + rc;
        t1.a_code = 2;
        t1.lda = Sj;
        t1.B = core(c, j);
        t1.b_code = h_codes[c];
        t1.ldb = d * cb2;
        t1.C = b.Z + z;
        t1.ldc = d * cb2;
        t1.M = ca;
        t1.N = d * cb2;
        t1.K = cb;
        Task t2{};  // GL_{j+1}[a, c] (ca2 x cb2) = (X^a_j viewed ca d x ca2)^T Z (ca d x cb2)
        t2.A = core(a, j);
        t2.a_code = h_codes[a];
        t2.transA = 1;
        t2.lda = ca2;
        t2.B = b.Z + z;
        t2.b_code = 2;
        t2.ldb = cb2;
        t2.C = b.GL[j + 1] + offs(a, j + 1) * Sn + offs(c, j + 1);
        t2.Cm = a == c ? nullptr : b.GL[j + 1] + offs(c, j + 1) * Sn + offs(a, j + 1);
        t2.ldc = Sn;
        t2.M = ca2;
        t2.N = cb2;
        t2.K = ca * d;
        tasks.push_back(t1);
        second.push_back(t2);
        z += ca * d * cb2;
      }
    NDMPS_REQUIRE(z <= p.zmax, "internal: transfer scratch");
    tasks.insert(tasks.end(), second.begin(), second.end());
  }
  const int64_t proj0 = (int64_t)tasks.size();
  for (int j = 0; j < L; ++j)
    for (int a = 0; a < K; ++a) {  // C_j[block a] (chi_{a,j} d_j x r) = X^a_j (chi_{a,j} d_j x chi_{a,j+1}) P_a
      Task t{};
      t.A = core(a, j);
      t.a_code = h_codes[a];
      t.lda = p.chi(a, j + 1);
      t.M = p.chi(a, j) * p.dims[j];
      t.K = p.chi(a, j + 1);
      t.brow = j + 1 == L ? a : offs(a, j + 1);
      t.crow = (j == 0 ? a : offs(a, j)) * p.dims[j];
      tasks.push_back(t);
    }
  {
    std::vector<double> host(2 * K + (size_t)K * K);
    for (int a = 0; a < K; ++a) {
      host[a] = h_w[a];
      host[K + a] = 1.0;
      for (int c = 0; c < K; ++c) host[2 * K + (size_t)a * K + c] = h_w[a] * h_w[c];
    }
    NDMPS_CHECK_HIP(hipMemcpyAsync(b.wts, host.data(), K * sizeof(double), hipMemcpyHostToDevice, s));
    NDMPS_CHECK_HIP(hipMemcpyAsync(b.ones, host.data() + K, K * sizeof(double), hipMemcpyHostToDevice, s));
    NDMPS_CHECK_HIP(hipMemcpyAsync(b.GL[0], host.data() + 2 * K, (size_t)K * K * sizeof(double), hipMemcpyHostToDevice, s));
    NDMPS_CHECK_HIP(hipMemcpyAsync(b.tasks, tasks.data(), tasks.size() * sizeof(Task), hipMemcpyHostToDevice, s));
    NDMPS_CHECK_HIP(hipStreamSynchronize(s));  // the host vectors go out of scope
  }

  // ---- 1. left Grams
  const int64_t np = (int64_t)K * (K + 1) / 2;
  for (int j = 0; j + 1 < L; ++j) {
    NDMPS_TRY(launch_tasks(b.tasks, tasks, 2 * np * j, np, false, nullptr, nullptr, 0, s));
    NDMPS_TRY(launch_tasks(b.tasks, tasks, 2 * np * j + np, np, false, nullptr, nullptr, 0, s));
  }

  // ---- 2. right-to-left sweep
  std::vector<int64_t> r(L + 1, 1);
  std::vector<double> hs(p.smax);
  // the zero MPS: every bond 1, zero cores, a kept value of 0 per bond
  auto zero_result = [&]() -> int {
    hipLaunchKernelGGL(zero_kernel<TO>, dim3(grid1d(p.out_off[L])), dim3(256), 0, s, d_out, p.out_off[L]);
    NDMPS_LAUNCH_CHECK();
    for (int j = 0; j <= L; ++j) h_out_bonds[j] = 1;
    for (int j = 1; j < L; ++j) h_spectra[(int64_t)j * spec_stride] = 0.0;
    NDMPS_CHECK_HIP(hipStreamSynchronize(s));
    return 1;  // > 0: the zero MPS
  };
  // scale = 0: every input is zero or weighted by zero, the sum is exactly zero (and no singular value can be divided by)
  if (L > 1 && !(scale > 0.0)) return zero_result();
  int cur = 0;
  // C_{L-1}: the last sites stacked (x_3 the 1 x 1 identity)
  NDMPS_TRY(launch_tasks(b.tasks, tasks, proj0 + (int64_t)(L - 1) * K, K, true, b.ones, b.C[cur], 1, s));
  for (int k = L - 1; k >= 1; --k) {
    const int64_t S = p.S[k], n = p.dims[k] * r[k + 1];
    double* A = b.C[cur];
    NDMPS_TRY(ndmps_dgemm(0, 1, S, S, n, A, n, A, n, b.G2, S, s));
    ndmps::GramTrunc g = b.g;
    g.chi = S;
    int64_t cap = std::min(p.left[k], n);
    if (max_bond > 0) cap = std::min(cap, max_bond);
    int64_t rk = 0;
    NDMPS_TRY(ndmps::gram_truncate<double>(g, b.GL[k], b.G2, A, n, 1, n, cutoff, floor, floor * scale, cap, f64, true,
                                           &rk, hs.data(), s));
    if (rk == 0) return zero_result();  // nothing survives
    NDMPS_REQUIRE(rk <= p.ub[k], "internal: bond %d kept %lld > %lld", k, (long long)rk, (long long)p.ub[k]);
    r[k] = rk;
    memcpy(h_spectra + (int64_t)k * spec_stride, hs.data(), rk * sizeof(double));
    // site k = diag(1/s) (Lt V_r)^T C_k
    NDMPS_TRY(ndmps_dgemm(0, 0, S, rk, S, g.Lt, S, g.V, S, g.P1, rk, s));
    NDMPS_TRY(ndmps_dgemm(1, 0, rk, n, S, g.P1, rk, A, n, b.Y, n, s));
    hipLaunchKernelGGL(rows_over_s_kernel<TO>, dim3(grid1d(rk * n)), dim3(256), 0, s, b.Y, rk, n, g.sig,
                       d_out + p.out_off[k]);
    // P = G2 Lt V_r diag(1/s)
    NDMPS_TRY(ndmps_dgemm(0, 0, S, rk, S, g.tmp, S, g.V, S, b.P2, rk, s));
    hipLaunchKernelGGL(cols_over_s_kernel, dim3(grid1d(S * rk)), dim3(256), 0, s, b.P2, S, rk, g.sig);
    NDMPS_LAUNCH_CHECK();
    NDMPS_TRY(launch_tasks(b.tasks, tasks, proj0 + (int64_t)(k - 1) * K, K, true, b.P2, b.C[cur ^ 1], rk, s));
    cur ^= 1;
  }
  hipLaunchKernelGGL(weighted_sum_kernel<TO>, dim3(grid1d(p.dims[0] * r[1])), dim3(256), 0, s, b.C[cur], K,
                     p.dims[0] * r[1], b.wts, d_out);
  NDMPS_LAUNCH_CHECK();
  for (int j = 0; j <= L; ++j) h_out_bonds[j] = r[j];
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));
  return NDMPS_OK;
}

}  // namespace

extern "C" int64_t ndmps_lincomb_layout(int K, int L, const int64_t* h_dims, const int64_t* h_bonds, int64_t max_bond,
                                        int64_t* h_out_off, int64_t* h_ws_bytes, int64_t* h_spec_stride) {
  Plan p;
  NDMPS_TRY(make_plan(K, L, h_dims, h_bonds, max_bond, p));
  if (h_out_off)
    for (int j = 0; j <= L; ++j) h_out_off[j] = p.out_off[j];
  if (h_ws_bytes) {
    Arena ar(nullptr, 0);
    Buffers b;
    carve(p, ar, b);
    *h_ws_bytes = ar.query_bytes();
  }
  if (h_spec_stride) *h_spec_stride = p.smax;
  return p.out_off[L];
}

extern "C" int ndmps_lincomb_round(int K, int L, const int64_t* h_dims, const int64_t* h_bonds, const int* h_codes,
                                   const void* const* h_cores, const double* h_weights, double cutoff, int64_t max_bond,
                                   int out_code, double scale, void* d_out, int64_t out_elems, int64_t* h_out_bonds,
                                   double* h_spectra, int64_t spec_stride, void* d_ws, int64_t ws_bytes,
                                   ndmps_stream_t stream) {
  NDMPS_REQUIRE(h_codes && h_cores && h_weights, "NULL lincomb argument");
  NDMPS_REQUIRE(out_code == 0 || out_code == 2, "output dtype code must be 0 (fp32) or 2 (fp64)");
  Plan p;
  NDMPS_TRY(make_plan(K, L, h_dims, h_bonds, max_bond, p));
  hipStream_t s = (hipStream_t)stream;
  if (out_code == 2)
    return lincomb_impl<double>(p, h_codes, h_cores, h_weights, cutoff, max_bond, scale, (double*)d_out, out_elems,
                                h_out_bonds, h_spectra, spec_stride, d_ws, ws_bytes, s);
  return lincomb_impl<float>(p, h_codes, h_cores, h_weights, cutoff, max_bond, scale, (float*)d_out, out_elems,
                             h_out_bonds, h_spectra, spec_stride, d_ws, ws_bytes, s);
}
