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
#include "pair_host.h"
#include "pair_product.h"

namespace {

using ndmps::Arena;
using ndmps::ChainList;
using ndmps::grid1d;
using ndmps::round_up;

constexpr int kResident = ndmps::kPairResident;  // largest inner bond of the resident sandwich
constexpr int64_t kGemmColumns = 1 << 19;        // columns of one weight product (ndmps_dgemm: n / 16 < 65536)

enum { kRouteResident = 0, kRoutePerPair = 2 };

struct WgramArgs {
  ndmps::PairListArgs t;   // the tables of both lists
  const int* pairs;        // (a, b) of every pair of the call
  const double* E;         // [w][pair of the chunk][slot_e]; not read at site 0
  double* P;               // [(w, i)][pair of the chunk][slot_p]
  int64_t slot_e, slot_p;
  int j, d, cw, n, p0;     // site, its physical dim, chi_{w,j}, pairs of the chunk, its first pair
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
  const int d = g.d, L = g.t.L, j = g.j;
  const int64_t wd = (int64_t)g.cw * d;
  const int q = (int)(blockIdx.x / wd);
  if (q >= g.n) return;
  const int rem = (int)(blockIdx.x % wd), w = rem / d, i = rem % d, i1 = i + 1;
  const int a = g.pairs[2 * (int64_t)(g.p0 + q)], b = g.pairs[2 * (int64_t)(g.p0 + q) + 1];
  const int ca = g.t.bonds_a[(int64_t)a * (L + 1) + j], ca2 = g.t.bonds_a[(int64_t)a * (L + 1) + j + 1];
  const int cb = g.t.bonds_b[(int64_t)b * (L + 1) + j], cb2 = g.t.bonds_b[(int64_t)b * (L + 1) + j + 1];
  const int code_a = g.t.codes_a[a], code_b = g.t.codes_b[b];
  const void* A = g.t.cores_a[(int64_t)a * L + j];
  const void* B = g.t.cores_b[(int64_t)b * L + j];
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
    ndmps::pair_set_unit(Et, tid);
  } else {  // this kernel's own spelling of pair_load_et: with the helper's address pin it measured slower
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

  // and of pair_store_strip, so that the instructions stay those that were measured
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
  ChainList la, lb, lw;  // the weight is a list of one; codes and cores: set by the entry point
  const int64_t* bw = nullptr;
  int64_t e_pair = 1, p_pair = 1, t_pair = 1;  // doubles of one pair: E (one of two), P, and T of the general route
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
  p.la.count = Ka, p.la.L = L, p.la.dims = h_dims, p.la.bonds = ba;
  p.lb.count = Kb, p.lb.L = L, p.lb.dims = h_dims, p.lb.bonds = bb;
  p.lw.count = 1, p.lw.L = L, p.lw.dims = h_dims, p.lw.bonds = bw;
  p.bw = bw;
  p.dims.assign(h_dims, h_dims + L);
  for (int j = 0; j < L; ++j)
    NDMPS_REQUIRE(p.dims[j] >= 1 && p.dims[j] <= INT32_MAX, "site %d: bad physical dim %lld", j, (long long)p.dims[j]);
  int64_t top = 1;  // of the two lists: the weight's bonds are unrestricted
  NDMPS_TRY(ndmps::check_chain_bonds(p.la, 0, " (2: the weight)", &top));
  NDMPS_TRY(ndmps::check_chain_bonds(p.lb, 1, " (2: the weight)", &top));
  NDMPS_TRY(ndmps::check_chain_bonds(p.lw, 2, " (2: the weight)", nullptr));
  if (p.symmetric) NDMPS_TRY(ndmps::check_symmetric(p.la, p.lb));
  p.n_pairs = p.symmetric ? (int64_t)Ka * (Ka + 1) / 2 : (int64_t)Ka * Kb;
  p.route = top <= kResident ? kRouteResident : kRoutePerPair;
  std::vector<int64_t> amax(L + 1, 1), bmax(L + 1, 1);  // per bond, the largest of either list: bounds over all pairs
  for (int j = 0; j <= L; ++j) {
    for (int a = 0; a < Ka; ++a) amax[j] = std::max(amax[j], p.la.chi(a, j));
    for (int b = 0; b < Kb; ++b) bmax[j] = std::max(bmax[j], p.lb.chi(b, j));
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
  ndmps::ChainTables tables;  // resident: the tables of WgramArgs
  int* pairs = nullptr;
  ndmps::WidenedLists w;    // the general route's cores in fp64
  std::vector<double*> ww;  // room for the weight's (null where it is fp64 already)
  // per chunk: two E, one P, and T on the general route
  double *E[2] = {nullptr, nullptr}, *P = nullptr, *T = nullptr;
};

// what does not grow with the chunk.  Without codes (the size query) every core counts as if it had to be widened.
void carve_fixed(const Plan& p, Arena& ar, Buffers& b) {
  if (p.route == kRouteResident) {
    b.tables.carve(p.la, p.lb, ar);
  } else {
    b.w.carve(p.la, p.lb, p.symmetric, ar);
    b.T = ar.take<double>(p.t_pair);
  }
  b.pairs = ar.take<int>(2 * p.n_pairs);
  ndmps::carve_list64(p.lw, ar, b.ww);
}

// the buffers of a chunk of n pairs: whole 256-byte pieces per pair, so that a cap maps to n without a remainder
void carve_chunk(const Plan& p, int64_t n, Arena& ar, Buffers& b) {
  b.E[0] = (double*)ar.take<char>(n * round_up(8 * p.e_pair, 256));
  b.E[1] = (double*)ar.take<char>(n * round_up(8 * p.e_pair, 256));
  b.P = (double*)ar.take<char>(n * round_up(8 * p.p_pair, 256));
}

// pairs per chunk under a workspace of `cap` bytes: all of them if they fit, at least one, else NDMPS_EWORKSPACE
int64_t chunk_for(Plan p, int64_t cap) {
  p.la.codes = p.lb.codes = p.lw.codes = nullptr;  // as the size query counts
  Arena ar(nullptr, 0);
  Buffers b;
  carve_fixed(p, ar, b);
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

int run_resident(const Plan& p, int64_t chunk, const std::vector<const double*>& W, double* d_G, Buffers& b, hipStream_t s) {
  const int L = p.L;
  WgramArgs g;
  NDMPS_TRY(b.tables.upload(p.la, p.lb, s, g.t));
  const std::vector<int> hp = ndmps::pair_table(p.Ka, p.Kb, p.symmetric);
  NDMPS_CHECK_HIP(hipMemcpyAsync(b.pairs, hp.data(), hp.size() * sizeof(int), hipMemcpyHostToDevice, s));
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));  // the host vectors go out of scope; nothing waits after the launches
  g.pairs = b.pairs;
  for (int64_t p0 = 0; p0 < p.n_pairs; p0 += chunk) {
    const int64_t n = std::min(chunk, p.n_pairs - p0);
    // slot of bond j: the largest chi_a chi_b of the chunk
    std::vector<int64_t> slot(L + 1, 1);
    for (int64_t q = 0; q < n; ++q) {
      const int a = hp[2 * (p0 + q)], c = hp[2 * (p0 + q) + 1];
      for (int j = 0; j <= L; ++j) slot[j] = std::max(slot[j], p.la.chi(a, j) * p.lb.chi(c, j));
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
      NDMPS_TRY(weight_product(W[j], cw, d, cw2, n * slot[j + 1], b.P, b.E[cur ^ 1], s));
      cur ^= 1;
    }
    NDMPS_TRY(gather(p, b.E[cur], slot[L], b.pairs, p0, n, d_G, s));
  }
  return NDMPS_OK;
}

int run_general(const Plan& p, const std::vector<const double*>& W, double* d_G, Buffers& b, hipStream_t s) {
  const int L = p.L;
  NDMPS_TRY(b.w.fill(p.la, p.lb, p.symmetric, s));
  const std::vector<int> hp = ndmps::pair_table(p.Ka, p.Kb, p.symmetric);
  NDMPS_CHECK_HIP(hipMemcpyAsync(b.pairs, hp.data(), hp.size() * sizeof(int), hipMemcpyHostToDevice, s));
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));
  static const double one = 1.0;
  for (int64_t q = 0; q < p.n_pairs; ++q) {
    const int a = hp[2 * q], c = hp[2 * q + 1];
    int cur = 0;
    NDMPS_CHECK_HIP(hipMemcpyAsync(b.E[0], &one, sizeof(double), hipMemcpyHostToDevice, s));  // E_0 = [[1]]
    for (int j = 0; j < L; ++j) {
      const int64_t ca = p.la.chi(a, j), ca2 = p.la.chi(a, j + 1), cb = p.lb.chi(c, j), cb2 = p.lb.chi(c, j + 1);
      const int64_t cw = p.bw[j], cw2 = p.bw[j + 1], d = p.dims[j];
      // T[w] = E[w] B_j over all w, then P[w, i] (ca2 x cb2) = A_i^T T[w][:, i, :]
      NDMPS_TRY(ndmps::sandwich_forward_general(ca, ca2, cb, cb2, d, cw, b.w.A[(size_t)a * L + j], b.w.B[(size_t)c * L + j], b.E[cur],
                                                b.P, b.T, s));
      NDMPS_TRY(weight_product(W[j], cw, d, cw2, ca2 * cb2, b.P, b.E[cur ^ 1], s));
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
  carve_fixed(p, ar, b);
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
  p.la.codes = h_codes_a, p.la.cores = h_cores_a;
  p.lb.codes = h_codes_b, p.lb.cores = h_cores_b;
  p.lw.codes = &code_w, p.lw.cores = h_cores_w;
  if (p.symmetric) NDMPS_TRY(ndmps::check_symmetric(p.la, p.lb));  // the cores: make_plan saw the rest
  NDMPS_TRY(ndmps::check_chain_cores(p.la, 0));
  NDMPS_TRY(ndmps::check_chain_cores(p.lb, 1));
  NDMPS_REQUIRE(code_w >= 0 && code_w <= 2, "the weight: bad dtype code %d", code_w);
  for (int j = 0; j < L; ++j) NDMPS_REQUIRE(h_cores_w[j], "the weight, site %d: NULL core", j);
  const int64_t chunk = chunk_for(p, ws_bytes);
  if (chunk < 0) return (int)chunk;
  Arena ar(d_ws, ws_bytes);
  Buffers b;
  carve_fixed(p, ar, b);
  carve_chunk(p, chunk, ar, b);
  if (!ar.fits()) {
    ndmps::set_error("weighted series workspace too small: %lld < %lld", (long long)ws_bytes, (long long)ar.used);
    return NDMPS_EWORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  std::vector<const double*> W;  // the weight's cores in fp64
  NDMPS_TRY(ndmps::fill_list64(p.lw, b.ww, s, W));
  if (p.route == kRouteResident) return run_resident(p, chunk, W, d_G, b, s);
  return run_general(p, W, d_G, b, s);
}
