// Gram matrix of a series of MPS (core/series.py, NDMPS.gram / inner / pca):  G[a, b] = <X^a, X^b>  for every pair of
// two lists of chains over the same site dims, computed on the cores.
//
// For one pair the transfer matrix E_j (chi_{a,j} x chi_{b,j}, fp64, E_0 = [1]) moves through the chain as
//     E_{j+1} = sum_i  A_j[:, i, :]^T ( E_j B_j[:, i, :] ),        G[a, b] = E_L[0, 0]
// (`E B` first: the other association of oracle.mps.mps_overlap and of ndmps_overlap_*).  Pairs are independent.
//
// Resident route (every inner bond of both lists <= 64): ONE launch, one workgroup of four waves per pair, all L sites,
//   on the two-phase pair product of pair_product.h (the LDS images Et and Z, the operand loader) and
//   pair_product_step.inc (phase 1, Z, phase 2 of one physical index i), in the forward form: E_j stays in LDS as Et
//   from site to site, a site's accumulators are transposed back into Et, and E_L[0, 0] is G[a, b].  Order of
//   summation is fixed (k ascending inside a product, i ascending), nothing is shared between workgroups, and nothing
//   waits.
// General route (some inner bond > 64): every core widened to fp64 once, then per site and pair two products on
//   ndmps_dgemm; when all chains of both lists have the same bonds the pairs go through ndmps_dgemm_batched in chunks
//   of ndmps_gemm_batched_max().  The last product writes its 1 x 1 result into G.
// The symmetric case computes a <= b and copies G[a, b] to G[b, a].
#include <algorithm>
#include <vector>

#include "common.h"
#include "pair_host.h"
#include "pair_product.h"

namespace {

using ndmps::Arena;
using ndmps::ChainList;
using ndmps::grid1d;

constexpr int kResident = ndmps::kPairResident;  // largest inner bond of the resident kernel

struct SeriesArgs {
  ndmps::PairListArgs t;  // the tables of both lists
  const int* dims;        // L
  double* G;              // Ka x Kb
  int Ka, Kb, symmetric;
};

// One workgroup per pair (a, b): E stays in LDS over all L sites, every site runs all its i through the step of
// pair_product_step.inc, and E_L[0, 0] goes to G[a, b] and its mirror.
__global__ void __launch_bounds__(256, 2) series_gram_resident_kernel(SeriesArgs g) {
  using ndmps::f64x4;
  using ndmps::pair_img;
  constexpr int kLd = ndmps::kPairLd;
  constexpr bool kTrans = false;
  const int a = (int)(blockIdx.x / (unsigned)g.Kb), b = (int)(blockIdx.x % (unsigned)g.Kb);
  if (a >= g.Ka || (g.symmetric && a > b)) return;
  __shared__ double Et[kLd * kLd];
  __shared__ double Z[kLd * kLd];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lc = lane & 15, lr = lane >> 4;
  const int L = g.t.L;
  const int* ba = g.t.bonds_a + (int64_t)a * (L + 1);
  const int* bb = g.t.bonds_b + (int64_t)b * (L + 1);
  const int code_a = g.t.codes_a[a], code_b = g.t.codes_b[b];

  ndmps::pair_set_unit(Et, tid);  // E_0 = [1]
  __syncthreads();

  for (int j = 0; j < L; ++j) {
    const int ca = ba[j], ca2 = ba[j + 1], cb = bb[j], cb2 = bb[j + 1], d = g.dims[j], i1 = d;
    const void* A = g.t.cores_a[(int64_t)a * L + j];
    const void* B = g.t.cores_b[(int64_t)b * L + j];
    // E_j is ca x cb, E_{j+1} ca2 x cb2
    const int tiles_re = (ca + 15) >> 4, tiles_ro = (ca2 + 15) >> 4, tiles_co = (cb2 + 15) >> 4;
    const int steps1 = (cb + 3) >> 2, steps2 = (ca + 3) >> 2;
    const bool own1 = wave < tiles_co, own2 = wave < tiles_ro;  // this wave's tile of Z / of E' exists
    const int col = wave * 16 + lc;

    f64x4 acc[4];  // E_{j+1}: rows 16 wave + lr + 4 r, columns 16 nt + lc
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = (f64x4){0.0, 0.0, 0.0, 0.0};
    double bq[16], aq[16];
    ndmps::pair_load_operands<kTrans>(bq, B, code_b, cb, d, cb2, 0, lr, col, own1);

    for (int i = 0; i < i1; ++i) {
      ndmps::pair_load_operands<kTrans>(aq, A, code_a, ca, d, ca2, i, lr, col, own2);
#include "pair_product_step.inc"
    }
    // E_{j+1} transposed into Et (every entry: the padding is zero in the accumulators)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) Et[pair_img(16 * nt + lc, 16 * wave + lr + 4 * r)] = acc[nt][r];
    __syncthreads();
  }
  if (tid == 0) {
    const double v = Et[0];
    g.G[(int64_t)a * g.Kb + b] = v;
    if (g.symmetric && a != b) g.G[(int64_t)b * g.Kb + a] = v;
  }
}

// G[b, a] <- G[a, b] for a < b (K x K)
__global__ void __launch_bounds__(256) mirror_kernel(double* __restrict__ G, int64_t K) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < K * K; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / K, c = e % K;
    if (r > c) G[e] = G[c * K + r];
  }
}

enum { kRouteResident = 0, kRouteBatched = 1, kRoutePerPair = 2 };

// Host plan: the checked arguments, the route and the workspace carve (a null arena counts bytes).
struct Plan {
  int Ka = 0, Kb = 0, L = 0, route = 0, chunk = 1;
  std::vector<int64_t> dims;
  ChainList la, lb;            // codes and cores: set by the entry point
  int64_t emax = 1, zmax = 1;  // largest E_j and Z of any pair
};

int make_plan(int Ka, int Kb, int L, const int64_t* h_dims, const int64_t* ba, const int64_t* bb, Plan& p) {
  NDMPS_REQUIRE(Ka >= 1 && Kb >= 1 && L >= 1 && h_dims && ba && bb, "bad series argument (Ka = %d, Kb = %d, L = %d)", Ka, Kb, L);
  NDMPS_REQUIRE((int64_t)Ka * Kb <= INT32_MAX, "series of %d x %d pairs exceeds one grid", Ka, Kb);
  p.Ka = Ka;
  p.Kb = Kb;
  p.L = L;
  p.la.count = Ka, p.la.L = L, p.la.dims = h_dims, p.la.bonds = ba;
  p.lb.count = Kb, p.lb.L = L, p.lb.dims = h_dims, p.lb.bonds = bb;
  p.dims.assign(h_dims, h_dims + L);
  for (int j = 0; j < L; ++j)
    NDMPS_REQUIRE(p.dims[j] >= 1 && p.dims[j] <= INT32_MAX, "site %d: bad physical dim %lld", j, (long long)p.dims[j]);
  int64_t top = 1, amax = 1, bmax = 1, a2max = 1, b2max = 1;
  NDMPS_TRY(ndmps::check_chain_bonds(p.la, 0, "", &top));
  NDMPS_TRY(ndmps::check_chain_bonds(p.lb, 1, "", &top));
  bool same = true;  // every chain of both lists has the bonds of the first
  for (int a = 0; a < Ka; ++a)
    for (int j = 0; j <= L; ++j) same = same && p.la.chi(a, j) == ba[j];
  for (int b = 0; b < Kb; ++b)
    for (int j = 0; j <= L; ++j) same = same && p.lb.chi(b, j) == ba[j];
  for (int j = 0; j < L; ++j) {  // bounds over all pairs: per site, largest factors of either list
    amax = a2max = bmax = b2max = 1;
    for (int a = 0; a < Ka; ++a) amax = std::max(amax, p.la.chi(a, j)), a2max = std::max(a2max, p.la.chi(a, j + 1));
    for (int b = 0; b < Kb; ++b) bmax = std::max(bmax, p.lb.chi(b, j)), b2max = std::max(b2max, p.lb.chi(b, j + 1));
    p.emax = std::max(p.emax, a2max * b2max);
    p.zmax = std::max(p.zmax, amax * p.dims[j] * b2max);
  }
  p.route = top <= kResident ? kRouteResident : same ? kRouteBatched : kRoutePerPair;
  p.chunk = p.route == kRouteBatched ? (int)std::min<int64_t>((int64_t)Ka * Kb, ndmps_gemm_batched_max()) : 1;
  return NDMPS_OK;
}

struct Buffers {
  ndmps::ChainTables tables;  // resident: the tables of SeriesArgs, and its dims
  int* dims = nullptr;
  // general: the cores in fp64, and per pair of a chunk two E and one Z
  ndmps::WidenedLists w;
  double *E[2] = {nullptr, nullptr}, *Z = nullptr;
};

void carve(const Plan& p, bool symmetric, Arena& ar, Buffers& b) {
  if (p.route == kRouteResident) {
    b.tables.carve(p.la, p.lb, ar);
    b.dims = ar.take<int>(p.L);
    return;
  }
  b.w.carve(p.la, p.lb, symmetric, ar);
  b.E[0] = ar.take<double>(p.emax * p.chunk);
  b.E[1] = ar.take<double>(p.emax * p.chunk);
  b.Z = ar.take<double>(p.zmax * p.chunk);
}

int run_resident(const Plan& p, int symmetric, double* d_G, Buffers& b, hipStream_t s) {
  SeriesArgs g;
  NDMPS_TRY(b.tables.upload(p.la, p.lb, s, g.t));
  const std::vector<int> hd(p.dims.begin(), p.dims.end());
  NDMPS_CHECK_HIP(hipMemcpyAsync(b.dims, hd.data(), hd.size() * sizeof(int), hipMemcpyHostToDevice, s));
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));  // the host vectors go out of scope; nothing waits after the launch
  g.dims = b.dims;
  g.G = d_G;
  g.Ka = p.Ka;
  g.Kb = p.Kb;
  g.symmetric = symmetric;
  // 1-D grid over the pairs (a, b) = (x / Kb, x % Kb): no 65535 limit; the symmetric case leaves a > b at once
  hipLaunchKernelGGL(series_gram_resident_kernel, dim3((unsigned)((int64_t)p.Ka * p.Kb)), dim3(256), 0, s, g);
  NDMPS_LAUNCH_CHECK();
  return NDMPS_OK;
}

int run_general(const Plan& p, int symmetric, double* d_G, Buffers& b, hipStream_t s) {
  const int L = p.L, Ka = p.Ka, Kb = p.Kb;
  NDMPS_TRY(b.w.fill(p.la, p.lb, symmetric, s));
  const std::vector<const double*>&A = b.w.A, &B = b.w.B;
  const std::vector<int> pairs = ndmps::pair_table(Ka, Kb, symmetric);
  const size_t n_pairs = pairs.size() / 2;
  const int chunk = p.chunk;
  std::vector<const double*> pa(chunk), pb(chunk);
  std::vector<double*> pc(chunk);
  for (size_t p0 = 0; p0 < n_pairs; p0 += chunk) {
    const int n = (int)std::min<size_t>(chunk, n_pairs - p0);
    int cur = 0;
    for (int j = 0; j < L; ++j) {
      // shapes of the chunk: one pair, or pairs that share every bond
      const int a0 = pairs[2 * p0], c0 = pairs[2 * p0 + 1];
      const int64_t ca = p.la.chi(a0, j), ca2 = p.la.chi(a0, j + 1), cb = p.lb.chi(c0, j), cb2 = p.lb.chi(c0, j + 1), d = p.dims[j];
      if (j > 0) {  // Z (ca x d cb2) = E_j (ca x cb) B_j (cb x d cb2); at site 0 E_0 = [1] and Z is the core itself
        for (int q = 0; q < n; ++q) {
          pa[q] = b.E[cur] + (int64_t)q * p.emax;
          pb[q] = B[(size_t)pairs[2 * (p0 + q) + 1] * L + j];
          pc[q] = b.Z + (int64_t)q * p.zmax;
        }
        if (p.route == kRouteBatched)
          NDMPS_TRY(ndmps_dgemm_batched(n, 0, 0, ca, d * cb2, cb, pa.data(), cb, pb.data(), d * cb2, pc.data(), d * cb2, s));
        else
          NDMPS_TRY(ndmps_dgemm(0, 0, ca, d * cb2, cb, pa[0], cb, pb[0], d * cb2, pc[0], d * cb2, s));
      }
      // E_{j+1} (ca2 x cb2) = (A_j viewed ca d x ca2)^T (Z viewed ca d x cb2); the last one is G[a, b]
      for (int q = 0; q < n; ++q) {
        const int a = pairs[2 * (p0 + q)], c = pairs[2 * (p0 + q) + 1];
        pa[q] = A[(size_t)a * L + j];
        pb[q] = j > 0 ? b.Z + (int64_t)q * p.zmax : B[(size_t)c * L + j];
        pc[q] = j + 1 == L ? d_G + (int64_t)a * Kb + c : b.E[cur ^ 1] + (int64_t)q * p.emax;
      }
      if (p.route == kRouteBatched)
        NDMPS_TRY(ndmps_dgemm_batched(n, 1, 0, ca2, cb2, ca * d, pa.data(), ca2, pb.data(), cb2, pc.data(), cb2, s));
      else
        NDMPS_TRY(ndmps_dgemm(1, 0, ca2, cb2, ca * d, pa[0], ca2, pb[0], cb2, pc[0], cb2, s));
      cur ^= 1;
    }
  }
  if (symmetric) {
    hipLaunchKernelGGL(mirror_kernel, dim3(grid1d((int64_t)Ka * Ka)), dim3(256), 0, s, d_G, (int64_t)Ka);
    NDMPS_LAUNCH_CHECK();
  }
  return NDMPS_OK;
}

}  // namespace

extern "C" int ndmps_series_gram_route(int Ka, int Kb, int L, const int64_t* h_dims, const int64_t* h_bonds_a,
                                       const int64_t* h_bonds_b) {
  Plan p;
  NDMPS_TRY(make_plan(Ka, Kb, L, h_dims, h_bonds_a, h_bonds_b, p));
  return p.route;
}

extern "C" int64_t ndmps_series_gram_workspace_bytes(int Ka, int Kb, int L, const int64_t* h_dims, const int64_t* h_bonds_a,
                                                     const int64_t* h_bonds_b) {
  Plan p;
  NDMPS_TRY(make_plan(Ka, Kb, L, h_dims, h_bonds_a, h_bonds_b, p));
  Arena ar(nullptr, 0);
  Buffers b;
  carve(p, false, ar, b);
  return ar.query_bytes();
}

extern "C" int ndmps_series_gram(int Ka, int Kb, int symmetric, int L, const int64_t* h_dims, const int64_t* h_bonds_a,
                                 const int* h_codes_a, const void* const* h_cores_a, const int64_t* h_bonds_b,
                                 const int* h_codes_b, const void* const* h_cores_b, double* d_G, void* d_ws,
                                 int64_t ws_bytes, ndmps_stream_t stream) {
  NDMPS_REQUIRE(h_codes_a && h_cores_a && h_codes_b && h_cores_b && d_G, "NULL series argument");
  Plan p;
  NDMPS_TRY(make_plan(Ka, Kb, L, h_dims, h_bonds_a, h_bonds_b, p));
  p.la.codes = h_codes_a, p.la.cores = h_cores_a;
  p.lb.codes = h_codes_b, p.lb.cores = h_cores_b;
  symmetric = symmetric != 0;
  if (symmetric) NDMPS_TRY(ndmps::check_symmetric(p.la, p.lb));
  NDMPS_TRY(ndmps::check_chain_cores(p.la, 0));
  NDMPS_TRY(ndmps::check_chain_cores(p.lb, 1));
  Arena ar(d_ws, ws_bytes);
  Buffers b;
  carve(p, symmetric, ar, b);
  if (!ar.fits()) {
    ndmps::set_error("series workspace too small: %lld < %lld", (long long)ws_bytes, (long long)ar.used);
    return NDMPS_EWORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  if (p.route == kRouteResident) return run_resident(p, symmetric, d_G, b, s);
  return run_general(p, symmetric, d_G, b, s);
}
