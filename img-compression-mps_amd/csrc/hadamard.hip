// Elementwise product of two MPS by a randomised sketch (core/hadamard.py, NDMPS.multiply / square).
//
// The product chain  Z_k[(a,a'), i, (b,b')] = A_k[a,i,b] B_k[a',i,b']  has the bonds m_k = chi_a chi_b (4096 at
// chi = 64).  It is never formed.  Random cores R_k (l_k, d_k, l_{k+1}), fp64, drawn on the host, sketch it down to
// a left-orthonormal fp64 chain of bonds r_k <= l_k ("randomise then orthogonalise", Al Daas et al., SISC 2023), which
// ndmps_lincomb_round then rounds at that small order:
//   1. right environments, k = L-1 .. 1, stored transposed  Wt_k (l_k x m_k),  Wt_L = [1]:
//        Y[(lam,i), (b,b')] = sum_mu R_k[lam,i,mu] Wt_{k+1}[mu,(b,b')]          one ndmps_dgemm  (Y = R_k where l_{k+1} = m_{k+1})
//        Wt_k[lam] (chi_a x chi_b) = sum_i A_k[:,i,:] Y[lam,i] B_k[:,i,:]^T      the sandwich, environment form
//      A bond with l_k = m_k needs no environment: the sketch is the identity there.
//   2. forward, k = 0 .. L-2, carrying X_k ((r_k d_k) x m_{k+1}), M_0 = [1]:
//        X_k[(rho,i)] (chi_a' x chi_b') = A_k[:,i,:]^T M_k[rho] B_k[:,i,:]        the sandwich, forward form
//        S = X_k Wt_{k+1}^T   ((r_k d_k) x l_{k+1};  S = X_k where l_{k+1} = m_{k+1})
//        twice:  G = S^T S = V diag(s^2) V^T (ndmps_syevj_f64, order <= 512), keep s_j > 1e-7 s_0,  S <- S V_r diag(1/s)   (gram_pass.h)
//        site k = S (left-orthonormal after the second pass),  M_{k+1} = S^T X_k  (r_{k+1} x m_{k+1})
//      s_0 = 0 at some bond: the product is zero.  The last site is X_{L-1}.
//
// The sandwich  out[t] (+)= op(A[:,i,:]) E[t] op(B[:,i,:])  is the hot path.  Resident route (all four bonds of the
// site <= 64): the two-phase pair product of pair_product.h (the LDS images, the operand loader with its transposed
// read for the environment form) and pair_product_step.inc (phase 1, Z, phase 2 of one i) on v_mfma_f64_16x16x4_f64,
// one workgroup of four waves per rho and i (forward) or per lam with i ascending inside (environment: no atomics).
// What is the sandwich's own: E comes from global memory and is transposed into LDS for every task and i, and the
// result leaves by a guarded store (tiles past the bonds are skipped and never stored).
// General route (some bond of the site > 64): the cores widened to fp64 once per call, then per site one ndmps_dgemm
//   and ndmps_dgemm_batched over the tasks in chunks of ndmps_gemm_batched_max().
// Nothing waits across workgroups; the order of every sum is fixed, so the same inputs give the same bits.
#include <math.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "gram_pass.h"
#include "pair_host.h"
#include "pair_product.h"

namespace {

using ndmps::Arena;
using ndmps::f64x4;
using ndmps::core64;
using ndmps::grid1d;

constexpr int kResident = ndmps::kPairResident;  // largest bond of the resident sandwich
constexpr int kMaxSketch = 512;    // largest sketch bond (order of the eigenproblems)

struct SandwichArgs {
  const void* A;    // (ca, d, ca2) in storage type code_a
  const void* B;    // (cb, d, cb2) in storage type code_b
  const double* E;  // forward: n matrices ca x cb; environment: n d matrices ca2 x cb2 (task (rho, i) at rho d + i)
  double* out;      // forward: n d matrices ca2 x cb2; environment: n matrices ca x cb
  int ca, ca2, cb, cb2, d, n, code_a, code_b;
};

// One workgroup's sandwich: E comes from global memory for every i, the step of one i is pair_product_step.inc, and
// the result goes to out[task] by a guarded store.
//   kEnv == false: blockIdx.x = rho d + i,  out[rho d + i] = A_i^T E[rho] B_i
//   kEnv == true:  blockIdx.x = rho,        out[rho] = sum_i A_i E[rho d + i] B_i^T   (i ascending)
template <bool kEnv>
__global__ void __launch_bounds__(256, 2) hadamard_sandwich_kernel(SandwichArgs g) {
  using ndmps::pair_img;
  constexpr int kLd = ndmps::kPairLd;
  constexpr bool kTrans = kEnv;
  __shared__ double Et[kLd * kLd];
  __shared__ double Z[kLd * kLd];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lc = lane & 15, lr = lane >> 4;
  const int d = g.d;
  const int64_t task = blockIdx.x;
  if (task >= (kEnv ? (int64_t)g.n : (int64_t)g.n * d)) return;
  const void* B = g.B;
  const int cb = g.cb, cb2 = g.cb2, code_b = g.code_b;
  // E is re x ce; the output ro x co
  const int re = kEnv ? g.ca2 : g.ca, ce = kEnv ? g.cb2 : g.cb;
  const int ro = kEnv ? g.ca : g.ca2, co = kEnv ? g.cb : g.cb2;
  const int tiles_re = (re + 15) >> 4, tiles_ro = (ro + 15) >> 4, tiles_co = (co + 15) >> 4;
  const int steps1 = (ce + 3) >> 2, steps2 = (re + 3) >> 2;
  const bool own1 = wave < tiles_co, own2 = wave < tiles_ro;  // this wave's tile of Z / of the output exists
  const int col = wave * 16 + lc;
  const int i0 = kEnv ? 0 : (int)(task % d), i1 = kEnv ? d : i0 + 1;
  const int64_t e0 = kEnv ? task * d : task / d;  // first matrix of E this workgroup reads

  f64x4 acc[4];  // output rows 16 wave + lr + 4 r, columns 16 nt + lc
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) acc[nt] = (f64x4){0.0, 0.0, 0.0, 0.0};
  double bq[16], aq[16];
  ndmps::pair_load_operands<kTrans>(bq, B, code_b, cb, d, cb2, i0, lr, col, own1);

  for (int i = i0; i < i1; ++i) {
    // ---- E of this task, transposed into Et: Et[k][m] = E[m][k], zero outside re x ce.  A wave's pass reads 16
    // consecutive k of four rows m (128-byte runs) and writes four consecutive m of 16 image rows.
    ndmps::pair_load_et(Et, g.E + (e0 + (kEnv ? i : 0)) * (int64_t)re * ce, re, ce, ce, tid);
    ndmps::pair_load_operands<kTrans>(aq, g.A, g.code_a, g.ca, d, g.ca2, i, lr, col, own2);
    __syncthreads();
#include "pair_product_step.inc"
  }
  ndmps::pair_store_strip(g.out + task * (int64_t)ro * co, co, acc, ro, co, wave, lr, lc);
}

// One site's sandwich: the checked extents and, on the general route, the fp64 cores and the scratch T.
struct Site {
  int64_t ca = 1, ca2 = 1, cb = 1, cb2 = 1, d = 1;
  int code_a = 0, code_b = 0;
  const void *A = nullptr, *B = nullptr;
  bool resident() const { return std::max({ca, ca2, cb, cb2}) <= kResident; }
};

int check_site(const Site& t, int64_t n) {
  NDMPS_REQUIRE(t.ca >= 1 && t.ca2 >= 1 && t.cb >= 1 && t.cb2 >= 1 && t.d >= 1 && n >= 1, "bad sandwich extents");
  NDMPS_REQUIRE(std::max({t.ca, t.ca2, t.cb, t.cb2}) <= (1 << 20) && t.d <= INT32_MAX / 2, "bad sandwich extents");
  NDMPS_REQUIRE(n <= kMaxSketch && n * t.d <= INT32_MAX / 2, "a sandwich takes at most %d matrices, got %lld", kMaxSketch, (long long)n);
  NDMPS_REQUIRE(t.code_a >= 0 && t.code_a <= 2 && t.code_b >= 0 && t.code_b <= 2, "bad dtype code (%d, %d)", t.code_a, t.code_b);
  NDMPS_REQUIRE(t.A && t.B, "NULL core");
  return NDMPS_OK;
}

int sandwich_resident(const Site& t, bool env, int64_t n, const double* E, double* out, hipStream_t s) {
  SandwichArgs g;
  g.A = t.A;
  g.B = t.B;
  g.E = E;
  g.out = out;
  g.ca = (int)t.ca;
  g.ca2 = (int)t.ca2;
  g.cb = (int)t.cb;
  g.cb2 = (int)t.cb2;
  g.d = (int)t.d;
  g.n = (int)n;
  g.code_a = t.code_a;
  g.code_b = t.code_b;
  if (env)
    hipLaunchKernelGGL(hadamard_sandwich_kernel<true>, dim3((unsigned)n), dim3(256), 0, s, g);
  else
    hipLaunchKernelGGL(hadamard_sandwich_kernel<false>, dim3((unsigned)(n * t.d)), dim3(256), 0, s, g);
  NDMPS_LAUNCH_CHECK();
  return NDMPS_OK;
}

// doubles of the general route's scratch T for n matrices
int64_t general_scratch(const Site& t, int64_t n) { return n * t.ca * t.d * t.cb2; }

// General route on fp64 cores A64 / B64.
//   forward:      sandwich_forward_general of pair_host.h
//   environment:  T[lam][:, i, :] (ca x cb2) = A_i E[lam, i];        out[lam] = T[lam] (ca x d cb2) B (cb x d cb2)^T
int sandwich_general(const Site& t, bool env, int64_t n, const double* A64, const double* B64, const double* E, double* out,
                     double* T, hipStream_t s) {
  const int64_t ca = t.ca, ca2 = t.ca2, cb = t.cb, cb2 = t.cb2, d = t.d;
  if (!env) return ndmps::sandwich_forward_general(ca, ca2, cb, cb2, d, n, A64, B64, E, out, T, s);
  const int chunk = ndmps_gemm_batched_max();
  std::vector<const double*> pa(chunk), pb(chunk);
  std::vector<double*> pc(chunk);
  for (int64_t t0 = 0; t0 < n * d; t0 += chunk) {
    const int nb = (int)std::min<int64_t>(chunk, n * d - t0);
    for (int q = 0; q < nb; ++q) {
      const int64_t lam = (t0 + q) / d, i = (t0 + q) % d;
      pa[q] = A64 + i * ca2;
      pb[q] = E + (t0 + q) * ca2 * cb2;
      pc[q] = T + lam * ca * d * cb2 + i * cb2;
    }
    NDMPS_TRY(ndmps_dgemm_batched(nb, 0, 0, ca, cb2, ca2, pa.data(), d * ca2, pb.data(), cb2, pc.data(), d * cb2, s));
  }
  for (int64_t l0 = 0; l0 < n; l0 += chunk) {
    const int nb = (int)std::min<int64_t>(chunk, n - l0);
    for (int q = 0; q < nb; ++q) {
      pa[q] = T + (l0 + q) * ca * d * cb2;
      pb[q] = B64;
      pc[q] = out + (l0 + q) * ca * cb;
    }
    NDMPS_TRY(ndmps_dgemm_batched(nb, 0, 1, ca, cb, d * cb2, pa.data(), d * cb2, pb.data(), d * cb2, pc.data(), cb, s));
  }
  return NDMPS_OK;
}

// Host plan of a sketch: the checked arguments, the output layout and the workspace carve.
struct Plan : ndmps::SketchLayout {
  int L = 0;
  bool resident = true;
  std::vector<int64_t> ba, bb, m;
  int64_t xy = 1, mm = 1, tmax = 1;
  bool identity(int k) const { return ell[k] == m[k]; }
  int64_t core_a(int k) const { return ba[k] * dims[k] * ba[k + 1]; }
  int64_t core_b(int k) const { return bb[k] * dims[k] * bb[k + 1]; }
};

int make_plan(int L, const int64_t* h_dims, const int64_t* h_ba, const int64_t* h_bb, const int64_t* h_ell, Plan& p) {
  NDMPS_REQUIRE(L >= 1 && h_dims && h_ba && h_bb && h_ell, "bad hadamard argument (L = %d)", L);
  p.L = L;
  p.dims.assign(h_dims, h_dims + L);
  p.ba.assign(h_ba, h_ba + L + 1);
  p.bb.assign(h_bb, h_bb + L + 1);
  p.ell.assign(h_ell, h_ell + L + 1);
  p.m.assign(L + 1, 1);
  for (int k = 0; k < L; ++k)
    NDMPS_REQUIRE(p.dims[k] >= 1 && p.dims[k] <= (1 << 20), "site %d: bad physical dim %lld", k, (long long)p.dims[k]);
  NDMPS_REQUIRE(p.ba[0] == 1 && p.ba[L] == 1 && p.bb[0] == 1 && p.bb[L] == 1, "the outer bonds must be 1");
  NDMPS_REQUIRE(p.ell[0] == 1 && p.ell[L] == 1, "the outer sketch bonds must be 1");
  int64_t top = 1;
  for (int k = 0; k <= L; ++k) {
    NDMPS_REQUIRE(p.ba[k] >= 1 && p.ba[k] <= 4096 && p.bb[k] >= 1 && p.bb[k] <= 4096, "bond %d: bad bond (%lld, %lld)", k,
                  (long long)p.ba[k], (long long)p.bb[k]);
    p.m[k] = p.ba[k] * p.bb[k];
    NDMPS_REQUIRE(p.ell[k] >= 1 && p.ell[k] <= p.m[k], "bond %d: sketch bond %lld outside [1, %lld]", k, (long long)p.ell[k],
                  (long long)p.m[k]);
    NDMPS_REQUIRE(p.ell[k] <= kMaxSketch, "bond %d: sketch bond %lld exceeds %d", k, (long long)p.ell[k], kMaxSketch);
    top = std::max({top, p.ba[k], p.bb[k]});
  }
  p.resident = top <= kResident;
  for (int k = 0; k < L; ++k) {
    p.xy = std::max(p.xy, p.ell[k] * p.dims[k] * p.m[k + 1]);
    p.mm = std::max(p.mm, p.ell[k] * p.m[k]);
    p.tmax = std::max(p.tmax, p.ell[k] * p.ba[k] * p.dims[k] * p.bb[k + 1]);
  }
  return ndmps::fill_sketch_layout(p);
}

struct Buffers {
  double *R = nullptr, *XY = nullptr, *M = nullptr, *S = nullptr, *Q = nullptr, *T = nullptr;
  ndmps::GramPassWs gw;
  std::vector<double*> Wt, wa, wb;  // Wt[k]: null where the bond is an identity; wa / wb: the general route's cores
};

// Workspace (doubles, every piece 256-byte aligned), in this order:
//   R          sum_k l_k d_k l_{k+1}
//   Wt_k       l_k m_k for every inner bond with l_k < m_k
//   XY         max_k l_k d_k m_{k+1}      Y_k of step 1, then X_k of step 2: never live together
//   M          max_k l_k m_k
//   S, Q       max_k l_k d_k l_{k+1} each
//   G, V       lmax^2 each;  w  lmax;  the eigen-solver's workspace for order lmax
//   general route only: both chains' cores in fp64 and T, max_k l_k chi_{a,k} d_k chi_{b,k+1}
void carve(const Plan& p, Arena& ar, Buffers& b) {
  const int L = p.L;
  b.R = ar.take<double>(p.r_elems);
  b.Wt.assign(L + 1, nullptr);
  for (int k = 1; k < L; ++k)
    if (!p.identity(k)) b.Wt[k] = ar.take<double>(p.ell[k] * p.m[k]);
  b.XY = ar.take<double>(p.xy);
  b.M = ar.take<double>(p.mm);
  b.S = ar.take<double>(p.sq);
  b.Q = ar.take<double>(p.sq);
  b.gw = ndmps::carve_gram_pass(ar, p.lmax, p.eig);
  if (!p.resident) {
    b.wa.assign(L, nullptr);
    b.wb.assign(L, nullptr);
    for (int k = 0; k < L; ++k) b.wa[k] = ar.take<double>(p.core_a(k));
    for (int k = 0; k < L; ++k) b.wb[k] = ar.take<double>(p.core_b(k));
    b.T = ar.take<double>(p.tmax);
  }
}

}  // namespace

extern "C" int64_t ndmps_hadamard_layout(int L, const int64_t* h_dims, const int64_t* h_bonds_a, const int64_t* h_bonds_b,
                                         const int64_t* h_ell, int64_t* h_out_off, int64_t* h_ws_bytes) {
  Plan p;
  NDMPS_TRY(make_plan(L, h_dims, h_bonds_a, h_bonds_b, h_ell, p));
  if (h_out_off)
    for (int k = 0; k <= L; ++k) h_out_off[k] = p.out_off[k];
  if (h_ws_bytes) {
    Arena ar(nullptr, 0);
    Buffers b;
    carve(p, ar, b);
    *h_ws_bytes = ar.query_bytes();
  }
  return p.out_off[L];
}

extern "C" int ndmps_hadamard_sandwich(int form, int64_t ca, int64_t d, int64_t ca2, int64_t cb, int64_t cb2, int code_a,
                                       const void* d_core_a, int code_b, const void* d_core_b, int64_t n, const double* d_E,
                                       double* d_out, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  NDMPS_REQUIRE(form == 0 || form == 1, "sandwich form must be 0 (forward) or 1 (environment), got %d", form);
  NDMPS_REQUIRE(d_E && d_out, "NULL sandwich argument");
  Site t;
  t.ca = ca, t.ca2 = ca2, t.cb = cb, t.cb2 = cb2, t.d = d;
  t.code_a = code_a, t.code_b = code_b;
  t.A = d_core_a, t.B = d_core_b;
  NDMPS_TRY(check_site(t, n));
  hipStream_t s = (hipStream_t)stream;
  if (t.resident()) return sandwich_resident(t, form == 1, n, d_E, d_out, s);
  Arena ar(d_ws, ws_bytes);
  double* wa = ar.take<double>(ca * d * ca2);
  double* wb = ar.take<double>(cb * d * cb2);
  double* T = ar.take<double>(general_scratch(t, n));
  NDMPS_REQUIRE(ar.fits(), "sandwich workspace too small: %lld < %lld", (long long)ws_bytes, (long long)ar.used);
  const double *A64, *B64;
  NDMPS_TRY(core64(d_core_a, code_a, ca * d * ca2, wa, s, &A64));
  NDMPS_TRY(core64(d_core_b, code_b, cb * d * cb2, wb, s, &B64));
  return sandwich_general(t, form == 1, n, A64, B64, d_E, d_out, T, s);
}

extern "C" int ndmps_hadamard_sketch(int L, const int64_t* h_dims, const int64_t* h_bonds_a, int code_a,
                                     const void* const* h_cores_a, const int64_t* h_bonds_b, int code_b,
                                     const void* const* h_cores_b, const int64_t* h_ell, const double* h_R, int64_t r_len,
                                     double* d_out, int64_t out_elems, int64_t* h_ranks, void* d_ws, int64_t ws_bytes,
                                     ndmps_stream_t stream) {
  NDMPS_REQUIRE(h_cores_a && h_cores_b && h_R && d_out && h_ranks, "NULL hadamard argument");
  NDMPS_REQUIRE(code_a >= 0 && code_a <= 2 && code_b >= 0 && code_b <= 2, "bad dtype code (%d, %d)", code_a, code_b);
  Plan p;
  NDMPS_TRY(make_plan(L, h_dims, h_bonds_a, h_bonds_b, h_ell, p));
  for (int k = 0; k < L; ++k) NDMPS_REQUIRE(h_cores_a[k] && h_cores_b[k], "site %d: NULL core", k);
  NDMPS_TRY(ndmps::check_sketch_cores(p, r_len));
  NDMPS_REQUIRE(out_elems >= p.out_off[L], "output arena too small: %lld < %lld", (long long)out_elems, (long long)p.out_off[L]);
  Arena ar(d_ws, ws_bytes);
  Buffers b;
  carve(p, ar, b);
  NDMPS_REQUIRE(ar.fits(), "hadamard workspace too small: %lld < %lld", (long long)ws_bytes, (long long)ar.used);
  hipStream_t s = (hipStream_t)stream;
  NDMPS_CHECK_HIP(hipMemcpyAsync(b.R, h_R, r_len * sizeof(double), hipMemcpyHostToDevice, s));

  std::vector<Site> site(L);
  std::vector<const double*> A64(L, nullptr), B64(L, nullptr);
  for (int k = 0; k < L; ++k) {
    Site& t = site[k];
    t.ca = p.ba[k], t.ca2 = p.ba[k + 1], t.cb = p.bb[k], t.cb2 = p.bb[k + 1], t.d = p.dims[k];
    t.code_a = code_a, t.code_b = code_b;
    t.A = h_cores_a[k], t.B = h_cores_b[k];
    if (p.resident) continue;
    NDMPS_TRY(core64(t.A, code_a, p.core_a(k), b.wa[k], s, &A64[k]));
    NDMPS_TRY(core64(t.B, code_b, p.core_b(k), b.wb[k], s, &B64[k]));
  }
  auto sandwich = [&](int k, bool env, int64_t n, const double* E, double* out) -> int {
    if (p.resident) return sandwich_resident(site[k], env, n, E, out, s);
    return sandwich_general(site[k], env, n, A64[k], B64[k], E, out, b.T, s);
  };

  // ---- 1. right environments
  for (int k = L - 1; k >= 1; --k) {
    if (p.identity(k)) continue;
    const double* Rk = b.R + p.out_off[k];
    const double* Y = Rk;  // identity on the right: Y = R_k
    if (!p.identity(k + 1)) {
      NDMPS_TRY(ndmps_dgemm(0, 0, p.ell[k] * p.dims[k], p.m[k + 1], p.ell[k + 1], Rk, p.ell[k + 1], b.Wt[k + 1], p.m[k + 1],
                            b.XY, p.m[k + 1], s));
      Y = b.XY;
    }
    NDMPS_TRY(sandwich(k, true, p.ell[k], Y, b.Wt[k]));
  }

  // ---- 2. forward pass
  std::vector<int64_t> r(L + 1, 1);
  std::vector<double> hw(p.lmax);
  const double one = 1.0;
  NDMPS_CHECK_HIP(hipMemcpyAsync(b.M, &one, sizeof(double), hipMemcpyHostToDevice, s));
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));  // `one` and h_R are read
  auto zero_product = [&]() -> int {
    for (int k = 0; k <= L; ++k) h_ranks[k] = 1;
    NDMPS_CHECK_HIP(hipStreamSynchronize(s));
    return 1;
  };
  for (int k = 0; k < L; ++k) {
    const int64_t rows = r[k] * p.dims[k], mk = p.m[k + 1], l = p.ell[k + 1];
    NDMPS_TRY(sandwich(k, false, r[k], b.M, b.XY));  // X_k (rows x m_{k+1})
    if (k == L - 1) {
      NDMPS_CHECK_HIP(hipMemcpyAsync(d_out + p.out_off[k], b.XY, rows * sizeof(double), hipMemcpyDeviceToDevice, s));
      break;
    }
    const double* S = b.XY;
    if (!p.identity(k + 1)) {
      NDMPS_TRY(ndmps_dgemm(0, 1, rows, l, mk, b.XY, mk, b.Wt[k + 1], mk, b.S, l, s));
      S = b.S;
    }
    int64_t r1 = 0, r2 = 0;
    NDMPS_TRY(ndmps::gram_pass(b.gw, S, rows, l, b.Q, &r1, hw, s));
    if (r1 == 0) return zero_product();
    double* site_out = d_out + p.out_off[k];
    NDMPS_TRY(ndmps::gram_pass(b.gw, b.Q, rows, r1, site_out, &r2, hw, s));
    if (r2 == 0) return zero_product();
    r[k + 1] = r2;
    // M_{k+1} (r2 x m_{k+1}) = site^T X_k
    NDMPS_TRY(ndmps_dgemm(1, 0, r2, mk, rows, site_out, r2, b.XY, mk, b.M, mk, s));
  }
  for (int k = 0; k <= L; ++k) h_ranks[k] = r[k];
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));
  return NDMPS_OK;
}
