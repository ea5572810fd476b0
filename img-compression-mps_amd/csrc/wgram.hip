// Masked / weighted Gram matrix of a series of MPS (core/wgram.py, NDMPS.gram / inner / pca with weight=):
//     G_w[a, b] = sum_x  w(x) X^a(x) X^b(x)
// for every pair of two lists of chains and one weight chain w over the same site dims, computed on the cores by the
// three-chain contraction.  Nothing is rounded or sketched.
//
// For one pair the transfer object is a stack of matrices E_j[w] (w < chi_{w,j}; chi_{a,j} x chi_{b,j}, fp64,
// E_0 = [[1]]):
//     P_j[w, i]   = A_j[:, i, :]^T ( E_j[w] B_j[:, i, :] )            chi_{w,j} d_j sandwiches, forward form
//     E_{j+1}[w'] = sum_{(w,i)} W_j[w, i, w'] P_j[w, i]               one product against the weight's core
//     G_w[a, b]   = E_L[0][0, 0]
// Pairs are independent.  They are processed in chunks that fit the workspace the caller gives; a chunk's E and P live
// in the workspace as  E[w][pair][slot]  and  P[(w, i)][pair][slot],  slot = the largest chi_a chi_b of that bond in
// the chunk, a matrix row-major at the start of its slot.  The rest of a slot is never written and never enters a
// result: the sandwich reads and stores by the pair's own extents, and the weight product works column by column.
//
// Resident route (every inner bond of both lists <= 64; chi_w unrestricted): per site ONE launch of
//   series_wgram_site_kernel, one workgroup of four waves per (pair, w, i), on the two-phase pair product of
//   pair_product.h / pair_product_step.inc in the forward form (E_j[w] read from the workspace and transposed into the
//   Et image, one step, guarded store of P), then ONE ndmps_dgemm(transA = 1) over the whole chunk:
//   E_{j+1} (chi_w' x n slot) = W_j (chi_w d x chi_w')^T  P (chi_w d x n slot).  A last tiny kernel gathers E_L into G.
// General route (some inner bond of the lists > 64): pair by pair on ndmps_dgemm / ndmps_dgemm_batched, cores widened
//   to fp64 once:  T[w] = E[w] B  (one product over all w),  P[w, i] = A_i^T T[w][:, i, :]  (batched over (w, i)),
//   and the same weight product.
// The order of every sum is fixed and does not depend on the chunking: the same inputs give the same bits.
#include <algorithm>
#include <vector>

#include "common.h"
#include "pair_product.h"

namespace {

using ndmps::Arena;
using ndmps::grid1d;
using ndmps::round_up;
using ndmps::widen;

constexpr int kResident = ndmps::kPairResident;  // largest inner bond of the resident sandwich
constexpr int64_t kGemmColumns = 1 << 19;        // columns of one weight product (ndmps_dgemm: n / 16 < 65536)

enum { kRouteResident = 0, kRoutePerPair = 2 };

struct WgramArgs {
  const void* const* cores_a;  // Ka x L
  const void* const* cores_b;  // Kb x L
  const int* bonds_a;          // Ka x (L + 1)
  const int* bonds_b;          // Kb x (L + 1)
  const int* codes_a;          // storage codes: 0 fp32, 1 bf16, 2 fp64
  const int* codes_b;
  const int* pairs;            // (a, b) of every pair of the call
  const double* E;             // [w][pair of the chunk][slot_e]; not read at site 0
  double* P;                   // [(w, i)][pair of the chunk][slot_p]
  int64_t slot_e, slot_p;
  int L, j, d, cw, n, p0;      // site, its physical dim, chi_{w,j}, pairs of the chunk, its first pair
};

// One workgroup's sandwich  P[w, i] = A_i^T E[w] B_i  of one pair at site j: E[w] comes from the workspace and is
// transposed into Et (site 0: E_0 = [1]), the step is pair_product_step.inc, and the result leaves by a guarded store.
__global__ void __launch_bounds__(256, 2) series_wgram_site_kernel(WgramArgs g) {
  using ndmps::f64x4;
  using ndmps::pair_img;
  constexpr int kLd = ndmps::kPairLd;
  constexpr bool kTrans = false;
  __shared__ double Et[kLd * kLd];
  __shared__ double Z[kLd * kLd];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lc = lane & 15, lr = lane >> 4;
  const int d = g.d, L = g.L, j = g.j;
  const int64_t wd = (int64_t)g.cw * d;
  const int q = (int)(blockIdx.x / wd);
  if (q >= g.n) return;
  const int rem = (int)(blockIdx.x % wd), w = rem / d, i = rem % d, i1 = i + 1;
  const int a = g.pairs[2 * (int64_t)(g.p0 + q)], b = g.pairs[2 * (int64_t)(g.p0 + q) + 1];
  const int ca = g.bonds_a[(int64_t)a * (L + 1) + j], ca2 = g.bonds_a[(int64_t)a * (L + 1) + j + 1];
  const int cb = g.bonds_b[(int64_t)b * (L + 1) + j], cb2 = g.bonds_b[(int64_t)b * (L + 1) + j + 1];
  const int code_a = g.codes_a[a], code_b = g.codes_b[b];
  const void* A = g.cores_a[(int64_t)a * L + j];
  const void* B = g.cores_b[(int64_t)b * L + j];
  // E is ca x cb, P ca2 x cb2
  const int tiles_re = (ca + 15) >> 4, tiles_ro = (ca2 + 15) >> 4, tiles_co = (cb2 + 15) >> 4;
  const int steps1 = (cb + 3) >> 2, steps2 = (ca + 3) >> 2;
  const bool own1 = wave < tiles_co, own2 = wave < tiles_ro;  // this wave's tile of Z / of P exists
  const int col = wave * 16 + lc;

  f64x4 acc[4];  // P rows 16 wave + lr + 4 r, columns 16 nt + lc
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) acc[nt] = (f64x4){0.0, 0.0, 0.0, 0.0};
  double bq[16], aq[16];
  ndmps::pair_load_operands<kTrans>(bq, B, code_b, cb, d, cb2, i, lr, col, own1);

  // ---- E[w] of this pair, transposed into Et: Et[k][m] = E[m][k], zero outside ca x cb
  if (j == 0) {
    for (int e = tid; e < kLd * kLd; e += 256) Et[e] = e == 0 ? 1.0 : 0.0;
  } else {
    const double* E = g.E + ((int64_t)w * g.n + q) * g.slot_e;
    const int kk = tid & 15, mm = tid >> 4;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) {
        const int k = 16 * kb + kk, m = 16 * mb + mm;
        const bool ok = k < cb && m < ca;
        const double v = E[ok ? (int64_t)m * cb + k : 0];
        Et[pair_img(k, m)] = ok ? v : 0.0;
      }
  }
  ndmps::pair_load_operands<kTrans>(aq, A, code_a, ca, d, ca2, i, lr, col, own2);
  __syncthreads();
#include "pair_product_step.inc"

  double* out = g.P + (((int64_t)w * d + i) * g.n + q) * g.slot_p;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * wave + lr + 4 * r, c = 16 * nt + lc;
      if (row < ca2 && c < cb2) out[(int64_t)row * cb2 + c] = acc[nt][r];
    }
}

// G[a, b] <- E_L of the chunk's pairs (the first element of each slot), and the mirror entry of a symmetric call
__global__ void __launch_bounds__(256) wgram_gather_kernel(const double* __restrict__ E, int64_t slot, const int* __restrict__ pairs,
                                                           int p0, int n, double* __restrict__ G, int Kb, int symmetric) {
  for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
    const int a = pairs[2 * (int64_t)(p0 + q)], b = pairs[2 * (int64_t)(p0 + q) + 1];
    const double v = E[(int64_t)q * slot];
    G[(int64_t)a * Kb + b] = v;
    if (symmetric && a != b) G[(int64_t)b * Kb + a] = v;
  }
}

// Host plan: the checked arguments, the route and what one pair costs in the workspace.
struct Plan {
  int Ka = 0, Kb = 0, L = 0, route = 0, symmetric = 0;
  int64_t n_pairs = 0;
  std::vector<int64_t> dims;
  const int64_t *ba = nullptr, *bb = nullptr, *bw = nullptr;
  int64_t e_pair = 1, p_pair = 1, t_pair = 1;  // doubles of one pair: E (one of two), P, and T of the general route
  int64_t chi_a(int a, int j) const { return ba[(int64_t)a * (L + 1) + j]; }
  int64_t chi_b(int b, int j) const { return bb[(int64_t)b * (L + 1) + j]; }
  int64_t core_a(int a, int j) const { return chi_a(a, j) * dims[j] * chi_a(a, j + 1); }
  int64_t core_b(int b, int j) const { return chi_b(b, j) * dims[j] * chi_b(b, j + 1); }
  int64_t core_w(int j) const { return bw[j] * dims[j] * bw[j + 1]; }
  // bytes of one pair of a chunk: two E and one P, each a whole number of 256-byte pieces
  int64_t pair_bytes() const { return 2 * round_up(8 * e_pair, 256) + round_up(8 * p_pair, 256); }
};

int make_plan(int Ka, int Kb, int symmetric, int L, const int64_t* h_dims, const int64_t* ba, const int64_t* bb,
              const int64_t* bw, Plan& p) {
  NDMPS_REQUIRE(Ka >= 1 && Kb >= 1 && L >= 1 && h_dims && ba && bb && bw,
                "bad weighted series argument (Ka = %d, Kb = %d, L = %d)", Ka, Kb, L);
  NDMPS_REQUIRE((int64_t)Ka * Kb <= INT32_MAX / 2, "series of %d x %d pairs exceeds one pair table", Ka, Kb);
  p.Ka = Ka;
  p.Kb = Kb;
  p.L = L;
  p.symmetric = symmetric != 0;
  p.ba = ba;
  p.bb = bb;
  p.bw = bw;
  p.dims.assign(h_dims, h_dims + L);
  for (int j = 0; j < L; ++j)
    NDMPS_REQUIRE(p.dims[j] >= 1 && p.dims[j] <= INT32_MAX, "site %d: bad physical dim %lld", j, (long long)p.dims[j]);
  int64_t top = 1;
  for (int side = 0; side < 3; ++side) {
    const int64_t* bl = side == 0 ? ba : side == 1 ? bb : bw;
    for (int a = 0; a < (side == 0 ? Ka : side == 1 ? Kb : 1); ++a) {
      const int64_t* row = bl + (int64_t)a * (L + 1);
      NDMPS_REQUIRE(row[0] == 1 && row[L] == 1, "list %d (2: the weight), chain %d: the outer bonds must be 1", side, a);
      for (int j = 0; j <= L; ++j) {
        NDMPS_REQUIRE(row[j] >= 1 && row[j] <= (1 << 20), "list %d, chain %d, bond %d: bad bond %lld", side, a, j,
                      (long long)row[j]);
        if (side < 2) top = std::max(top, row[j]);
      }
    }
  }
  if (p.symmetric) {
    NDMPS_REQUIRE(Ka == Kb, "a symmetric series needs one list (Ka = %d, Kb = %d)", Ka, Kb);
    for (int64_t e = 0; e < (int64_t)Ka * (L + 1); ++e)
      NDMPS_REQUIRE(ba[e] == bb[e], "a symmetric series needs the same bonds in both lists");
  }
  p.n_pairs = p.symmetric ? (int64_t)Ka * (Ka + 1) / 2 : (int64_t)Ka * Kb;
  p.route = top <= kResident ? kRouteResident : kRoutePerPair;
  std::vector<int64_t> amax(L + 1, 1), bmax(L + 1, 1);  // per bond, the largest of either list: bounds over all pairs
  for (int j = 0; j <= L; ++j) {
    for (int a = 0; a < Ka; ++a) amax[j] = std::max(amax[j], p.chi_a(a, j));
    for (int b = 0; b < Kb; ++b) bmax[j] = std::max(bmax[j], p.chi_b(b, j));
  }
  for (int j = 0; j <= L; ++j) p.e_pair = std::max(p.e_pair, bw[j] * amax[j] * bmax[j]);
  for (int j = 0; j < L; ++j) {
    NDMPS_REQUIRE(bw[j] * p.dims[j] <= INT32_MAX / 2, "site %d: chi_w d = %lld is too large", j, (long long)(bw[j] * p.dims[j]));
    p.p_pair = std::max(p.p_pair, bw[j] * p.dims[j] * amax[j + 1] * bmax[j + 1]);
    p.t_pair = std::max(p.t_pair, bw[j] * amax[j] * p.dims[j] * bmax[j + 1]);
  }
  return NDMPS_OK;
}

struct Buffers {
  // resident: the tables of WgramArgs
  const void** cores = nullptr;
  int *bonds = nullptr, *codes = nullptr, *pairs = nullptr;
  // the widened cores (null where a core is fp64 already); a and b on the general route only
  std::vector<double*> wa, wb, ww;
  // per chunk: two E, one P, and T on the general route
  double *E[2] = {nullptr, nullptr}, *P = nullptr, *T = nullptr;
};

// what does not grow with the chunk.  Without codes (the size query) every core counts as if it had to be widened.
void carve_fixed(const Plan& p, const int* codes_a, const int* codes_b, const int* code_w, Arena& ar, Buffers& b) {
  const int64_t K = (int64_t)p.Ka + p.Kb;
  if (p.route == kRouteResident) {
    b.cores = ar.take<const void*>(K * p.L);
    b.bonds = ar.take<int>(K * (p.L + 1));
    b.codes = ar.take<int>(K);
  } else {
    b.wa.assign((size_t)p.Ka * p.L, nullptr);
    b.wb.assign((size_t)p.Kb * p.L, nullptr);
    for (int a = 0; a < p.Ka; ++a)
      for (int j = 0; j < p.L; ++j)
        if (!codes_a || codes_a[a] != 2) b.wa[(size_t)a * p.L + j] = ar.take<double>(p.core_a(a, j));
    if (!p.symmetric || !codes_a)
      for (int c = 0; c < p.Kb; ++c)
        for (int j = 0; j < p.L; ++j)
          if (!codes_b || codes_b[c] != 2) b.wb[(size_t)c * p.L + j] = ar.take<double>(p.core_b(c, j));
    b.T = ar.take<double>(p.t_pair);
  }
  b.pairs = ar.take<int>(2 * p.n_pairs);
  b.ww.assign((size_t)p.L, nullptr);
  for (int j = 0; j < p.L; ++j)
    if (!code_w || *code_w != 2) b.ww[j] = ar.take<double>(p.core_w(j));
}

// the buffers of a chunk of n pairs: whole 256-byte pieces per pair, so that a cap maps to n without a remainder
void carve_chunk(const Plan& p, int64_t n, Arena& ar, Buffers& b) {
  b.E[0] = (double*)ar.take<char>(n * round_up(8 * p.e_pair, 256));
  b.E[1] = (double*)ar.take<char>(n * round_up(8 * p.e_pair, 256));
  b.P = (double*)ar.take<char>(n * round_up(8 * p.p_pair, 256));
}

// pairs per chunk under a workspace of `cap` bytes: all of them if they fit, at least one, else NDMPS_EWORKSPACE
int64_t chunk_for(const Plan& p, int64_t cap) {
  Arena ar(nullptr, 0);
  Buffers b;
  carve_fixed(p, nullptr, nullptr, nullptr, ar, b);
  const int64_t room = cap - 256 - round_up(ar.used, 256);
  int64_t n = room < 0 ? 0 : room / p.pair_bytes();
  if (n < 1) {
    ndmps::set_error("weighted series: one pair needs %lld bytes of workspace, the cap is %lld",
                     (long long)(round_up(ar.used, 256) + 256 + p.pair_bytes()), (long long)cap);
    return NDMPS_EWORKSPACE;
  }
  if (p.route != kRouteResident) return 1;
  int64_t grid = 1;  // the site kernel's grid is n chi_w d workgroups
  for (int j = 0; j < p.L; ++j) grid = std::max(grid, p.bw[j] * p.dims[j]);
  return std::min({n, p.n_pairs, (int64_t)INT32_MAX / grid});
}

struct Weight {
  std::vector<const double*> W;  // the weight's cores in fp64
};

int widen_weight(const Plan& p, int code_w, const void* const* cores_w, const Buffers& b, Weight& wt, hipStream_t s) {
  wt.W.resize(p.L);
  for (int j = 0; j < p.L; ++j) {
    wt.W[j] = (const double*)cores_w[j];
    if (code_w != 2) {
      NDMPS_TRY(widen(cores_w[j], code_w, p.core_w(j), b.ww[j], s));
      wt.W[j] = b.ww[j];
    }
  }
  return NDMPS_OK;
}

std::vector<int> pair_table(const Plan& p) {
  std::vector<int> t;
  t.reserve((size_t)2 * p.n_pairs);
  for (int a = 0; a < p.Ka; ++a)
    for (int c = p.symmetric ? a : 0; c < p.Kb; ++c) t.push_back(a), t.push_back(c);
  return t;
}

// E' (cw2 x cols) = W_j (cw d x cw2)^T P (cw d x cols), in pieces of kGemmColumns columns (columns are independent)
int weight_product(const double* W, int64_t cw, int64_t d, int64_t cw2, int64_t cols, const double* P, double* E2, hipStream_t s) {
  for (int64_t c0 = 0; c0 < cols; c0 += kGemmColumns) {
    const int64_t nc = std::min(kGemmColumns, cols - c0);
    NDMPS_TRY(ndmps_dgemm(1, 0, cw2, nc, cw * d, W, cw2, P + c0, cols, E2 + c0, cols, s));
  }
  return NDMPS_OK;
}

int gather(const Plan& p, const double* E, int64_t slot, const int* d_pairs, int64_t p0, int64_t n, double* d_G, hipStream_t s) {
  hipLaunchKernelGGL(wgram_gather_kernel, dim3(grid1d(n)), dim3(256), 0, s, E, slot, d_pairs, (int)p0, (int)n, d_G, p.Kb,
                     p.symmetric);
  NDMPS_LAUNCH_CHECK();
  return NDMPS_OK;
}

int run_resident(const Plan& p, int64_t chunk, const int* codes_a, const void* const* cores_a, const int* codes_b,
                 const void* const* cores_b, const Weight& wt, double* d_G, const Buffers& b, hipStream_t s) {
  const int L = p.L, Ka = p.Ka, Kb = p.Kb;
  std::vector<const void*> hc(cores_a, cores_a + (size_t)Ka * L);
  hc.insert(hc.end(), cores_b, cores_b + (size_t)Kb * L);
  std::vector<int> hb((size_t)(Ka + Kb) * (L + 1)), hk(codes_a, codes_a + Ka);
  for (size_t e = 0; e < (size_t)Ka * (L + 1); ++e) hb[e] = (int)p.ba[e];
  for (size_t e = 0; e < (size_t)Kb * (L + 1); ++e) hb[(size_t)Ka * (L + 1) + e] = (int)p.bb[e];
  hk.insert(hk.end(), codes_b, codes_b + Kb);
  const std::vector<int> hp = pair_table(p);
  NDMPS_CHECK_HIP(hipMemcpyAsync(b.cores, hc.data(), hc.size() * sizeof(void*), hipMemcpyHostToDevice, s));
  NDMPS_CHECK_HIP(hipMemcpyAsync(b.bonds, hb.data(), hb.size() * sizeof(int), hipMemcpyHostToDevice, s));
  NDMPS_CHECK_HIP(hipMemcpyAsync(b.codes, hk.data(), hk.size() * sizeof(int), hipMemcpyHostToDevice, s));
  NDMPS_CHECK_HIP(hipMemcpyAsync(b.pairs, hp.data(), hp.size() * sizeof(int), hipMemcpyHostToDevice, s));
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));  // the host vectors go out of scope; nothing waits after the launches
  WgramArgs g;
  g.cores_a = b.cores;
  g.cores_b = b.cores + (size_t)Ka * L;
  g.bonds_a = b.bonds;
  g.bonds_b = b.bonds + (size_t)Ka * (L + 1);
  g.codes_a = b.codes;
  g.codes_b = b.codes + Ka;
  g.pairs = b.pairs;
  g.L = L;
  for (int64_t p0 = 0; p0 < p.n_pairs; p0 += chunk) {
    const int64_t n = std::min(chunk, p.n_pairs - p0);
    // slot of bond j: the largest chi_a chi_b of the chunk
    std::vector<int64_t> slot(L + 1, 1);
    for (int64_t q = 0; q < n; ++q) {
      const int a = hp[2 * (p0 + q)], c = hp[2 * (p0 + q) + 1];
      for (int j = 0; j <= L; ++j) slot[j] = std::max(slot[j], p.chi_a(a, j) * p.chi_b(c, j));
    }
    int cur = 0;
    for (int j = 0; j < L; ++j) {
      const int64_t cw = p.bw[j], cw2 = p.bw[j + 1], d = p.dims[j];
      g.E = b.E[cur];
      g.P = b.P;
      g.slot_e = slot[j];
      g.slot_p = slot[j + 1];
      g.j = j;
      g.d = (int)d;
      g.cw = (int)cw;
      g.n = (int)n;
      g.p0 = (int)p0;
      hipLaunchKernelGGL(series_wgram_site_kernel, dim3((unsigned)(n * cw * d)), dim3(256), 0, s, g);
      NDMPS_LAUNCH_CHECK();
      NDMPS_TRY(weight_product(wt.W[j], cw, d, cw2, n * slot[j + 1], b.P, b.E[cur ^ 1], s));
      cur ^= 1;
    }
    NDMPS_TRY(gather(p, b.E[cur], slot[L], b.pairs, p0, n, d_G, s));
  }
  return NDMPS_OK;
}

int run_general(const Plan& p, const int* codes_a, const void* const* cores_a, const int* codes_b, const void* const* cores_b,
                const Weight& wt, double* d_G, const Buffers& b, hipStream_t s) {
  const int L = p.L, Ka = p.Ka, Kb = p.Kb;
  std::vector<const double*> A((size_t)Ka * L), B((size_t)Kb * L);
  for (int a = 0; a < Ka; ++a)
    for (int j = 0; j < L; ++j) {
      const size_t e = (size_t)a * L + j;
      A[e] = (const double*)cores_a[e];
      if (codes_a[a] != 2) {
        NDMPS_TRY(widen(cores_a[e], codes_a[a], p.core_a(a, j), b.wa[e], s));
        A[e] = b.wa[e];
      }
    }
  for (int c = 0; c < Kb; ++c)
    for (int j = 0; j < L; ++j) {
      const size_t e = (size_t)c * L + j;
      if (p.symmetric) {
        B[e] = A[e];
        continue;
      }
      B[e] = (const double*)cores_b[e];
      if (codes_b[c] != 2) {
        NDMPS_TRY(widen(cores_b[e], codes_b[c], p.core_b(c, j), b.wb[e], s));
        B[e] = b.wb[e];
      }
    }
  const std::vector<int> hp = pair_table(p);
  NDMPS_CHECK_HIP(hipMemcpyAsync(b.pairs, hp.data(), hp.size() * sizeof(int), hipMemcpyHostToDevice, s));
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));
  static const double one = 1.0;
  const int batch = ndmps_gemm_batched_max();
  std::vector<const double*> pa(batch), pb(batch);
  std::vector<double*> pc(batch);
  for (int64_t q = 0; q < p.n_pairs; ++q) {
    const int a = hp[2 * q], c = hp[2 * q + 1];
    int cur = 0;
    NDMPS_CHECK_HIP(hipMemcpyAsync(b.E[0], &one, sizeof(double), hipMemcpyHostToDevice, s));  // E_0 = [[1]]
    for (int j = 0; j < L; ++j) {
      const int64_t ca = p.chi_a(a, j), ca2 = p.chi_a(a, j + 1), cb = p.chi_b(c, j), cb2 = p.chi_b(c, j + 1);
      const int64_t cw = p.bw[j], cw2 = p.bw[j + 1], d = p.dims[j];
      const double *Aj = A[(size_t)a * L + j], *Bj = B[(size_t)c * L + j];
      // T (cw ca x d cb2) = E (cw ca x cb) B_j (cb x d cb2)
      NDMPS_TRY(ndmps_dgemm(0, 0, cw * ca, d * cb2, cb, b.E[cur], cb, Bj, d * cb2, b.T, d * cb2, s));
      // P[w, i] (ca2 x cb2) = A_i^T T[w][:, i, :]
      for (int64_t t0 = 0; t0 < cw * d; t0 += batch) {
        const int nb = (int)std::min<int64_t>(batch, cw * d - t0);
        for (int t = 0; t < nb; ++t) {
          const int64_t w = (t0 + t) / d, i = (t0 + t) % d;
          pa[t] = Aj + i * ca2;
          pb[t] = b.T + w * ca * d * cb2 + i * cb2;
          pc[t] = b.P + (t0 + t) * ca2 * cb2;
        }
        NDMPS_TRY(ndmps_dgemm_batched(nb, 1, 0, ca2, cb2, ca, pa.data(), d * ca2, pb.data(), d * cb2, pc.data(), cb2, s));
      }
      NDMPS_TRY(weight_product(wt.W[j], cw, d, cw2, ca2 * cb2, b.P, b.E[cur ^ 1], s));
      cur ^= 1;
    }
    NDMPS_TRY(gather(p, b.E[cur], 1, b.pairs, q, 1, d_G, s));
  }
  return NDMPS_OK;
}

}  // namespace

extern "C" int ndmps_series_wgram_route(int Ka, int Kb, int L, const int64_t* h_dims, const int64_t* h_bonds_a,
                                        const int64_t* h_bonds_b, const int64_t* h_bonds_w) {
  Plan p;
  NDMPS_TRY(make_plan(Ka, Kb, 0, L, h_dims, h_bonds_a, h_bonds_b, h_bonds_w, p));
  return p.route;
}

extern "C" int64_t ndmps_series_wgram_workspace_bytes(int Ka, int Kb, int symmetric, int L, const int64_t* h_dims,
                                                      const int64_t* h_bonds_a, const int64_t* h_bonds_b,
                                                      const int64_t* h_bonds_w, int64_t cap_bytes) {
  Plan p;
  NDMPS_TRY(make_plan(Ka, Kb, symmetric, L, h_dims, h_bonds_a, h_bonds_b, h_bonds_w, p));
  const int64_t n = chunk_for(p, cap_bytes);
  if (n < 0) return n;
  Arena ar(nullptr, 0);
  Buffers b;
  carve_fixed(p, nullptr, nullptr, nullptr, ar, b);
  carve_chunk(p, n, ar, b);
  return ar.query_bytes();
}

extern "C" int ndmps_series_wgram(int Ka, int Kb, int symmetric, int L, const int64_t* h_dims, const int64_t* h_bonds_a,
                                  const int* h_codes_a, const void* const* h_cores_a, const int64_t* h_bonds_b,
                                  const int* h_codes_b, const void* const* h_cores_b, const int64_t* h_bonds_w, int code_w,
                                  const void* const* h_cores_w, double* d_G, void* d_ws, int64_t ws_bytes,
                                  ndmps_stream_t stream) {
  NDMPS_REQUIRE(h_codes_a && h_cores_a && h_codes_b && h_cores_b && h_cores_w && d_G, "NULL weighted series argument");
  Plan p;
  NDMPS_TRY(make_plan(Ka, Kb, symmetric, L, h_dims, h_bonds_a, h_bonds_b, h_bonds_w, p));
  if (p.symmetric)
    for (int64_t e = 0; e < (int64_t)Ka * L; ++e)
      NDMPS_REQUIRE(h_cores_a[e] == h_cores_b[e], "a symmetric series needs the same cores in both lists");
  for (int side = 0; side < 2; ++side)
    for (int a = 0; a < (side ? Kb : Ka); ++a) {
      const int code = (side ? h_codes_b : h_codes_a)[a];
      NDMPS_REQUIRE(code >= 0 && code <= 2, "list %d, chain %d: bad dtype code %d", side, a, code);
      for (int j = 0; j < L; ++j)
        NDMPS_REQUIRE((side ? h_cores_b : h_cores_a)[(int64_t)a * L + j], "list %d, chain %d, site %d: NULL core", side, a, j);
    }
  NDMPS_REQUIRE(code_w >= 0 && code_w <= 2, "the weight: bad dtype code %d", code_w);
  for (int j = 0; j < L; ++j) NDMPS_REQUIRE(h_cores_w[j], "the weight, site %d: NULL core", j);
  const int64_t chunk = chunk_for(p, ws_bytes);
  if (chunk < 0) return (int)chunk;
  Arena ar(d_ws, ws_bytes);
  Buffers b;
  carve_fixed(p, h_codes_a, h_codes_b, &code_w, ar, b);
  carve_chunk(p, chunk, ar, b);
  if (!ar.fits()) {
    ndmps::set_error("weighted series workspace too small: %lld < %lld", (long long)ws_bytes, (long long)ar.used);
    return NDMPS_EWORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  Weight wt;
  NDMPS_TRY(widen_weight(p, code_w, h_cores_w, b, wt, s));
  if (p.route == kRouteResident)
    return run_resident(p, chunk, h_codes_a, h_cores_a, h_codes_b, h_cores_b, wt, d_G, b, s);
  return run_general(p, h_codes_a, h_cores_a, h_codes_b, h_cores_b, wt, d_G, b, s);
}
