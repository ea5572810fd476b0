// Host front end of the pair-product family (pair_product.h): what series.hip, wgram.hip, hadamard.hip and sumsketch.hip
// do around their kernels with lists of chains.  The only definition of the view of a list and its checks, of the
// fp64 copy of a core, of the fp64 copies and the device tables of two lists, of the pair table and of the general
// route's forward sandwich.  Host only; the layout of a sketch is in gram_pass.h.
#pragma once
#include <algorithm>
#include <vector>

#include "common.h"

namespace ndmps {

// A view of one list of `count` chains over the same L sites; codes and cores are absent in a size query.
struct ChainList {
  int count = 0, L = 0;
  const int64_t* dims = nullptr;       // L
  const int64_t* bonds = nullptr;      // count x (L + 1)
  const int* codes = nullptr;          // count storage codes: 0 fp32, 1 bf16, 2 fp64
  const void* const* cores = nullptr;  // count x L device pointers
  int64_t chi(int a, int j) const { return bonds[(int64_t)a * (L + 1) + j]; }
  int64_t core_elems(int a, int j) const { return chi(a, j) * dims[j] * chi(a, j + 1); }
};

// The outer bonds are 1 and every bond lies in [1, 2^20]; `top` (when given) collects the largest bond.  `note` follows
// "list <side>" in the first message.
static inline int check_chain_bonds(const ChainList& l, int side, const char* note, int64_t* top) {
  for (int a = 0; a < l.count; ++a) {
    NDMPS_REQUIRE(l.chi(a, 0) == 1 && l.chi(a, l.L) == 1, "list %d%s, chain %d: the outer bonds must be 1", side, note, a);
    for (int j = 0; j <= l.L; ++j) {
      NDMPS_REQUIRE(l.chi(a, j) >= 1 && l.chi(a, j) <= (1 << 20), "list %d, chain %d, bond %d: bad bond %lld", side, a, j,
                    (long long)l.chi(a, j));
      if (top) *top = std::max(*top, l.chi(a, j));
    }
  }
  return NDMPS_OK;
}

// every storage code lies in [0, 2] and no core is NULL
static inline int check_chain_cores(const ChainList& l, int side) {
  for (int a = 0; a < l.count; ++a) {
    NDMPS_REQUIRE(l.codes[a] >= 0 && l.codes[a] <= 2, "list %d, chain %d: bad dtype code %d", side, a, l.codes[a]);
    for (int j = 0; j < l.L; ++j) NDMPS_REQUIRE(l.cores[(int64_t)a * l.L + j], "list %d, chain %d, site %d: NULL core", side, a, j);
  }
  return NDMPS_OK;
}

// a symmetric call names one list twice: the same count, the same cores (where both views have them), the same bonds
static inline int check_symmetric(const ChainList& a, const ChainList& b) {
  NDMPS_REQUIRE(a.count == b.count, "a symmetric series needs one list (Ka = %d, Kb = %d)", a.count, b.count);
  if (a.cores && b.cores)
    for (int64_t e = 0; e < (int64_t)a.count * a.L; ++e)
      NDMPS_REQUIRE(a.cores[e] == b.cores[e], "a symmetric series needs the same cores in both lists");
  for (int64_t e = 0; e < (int64_t)a.count * (a.L + 1); ++e)
    NDMPS_REQUIRE(a.bonds[e] == b.bonds[e], "a symmetric series needs the same bonds in both lists");
  return NDMPS_OK;
}

// *out = the core of n elements in fp64: the core itself where it is fp64 (code 2), else its widened copy in dst
static inline int core64(const void* core, int code, int64_t n, double* dst, hipStream_t s, const double** out) {
  *out = (const double*)core;
  if (code == 2) return NDMPS_OK;
  NDMPS_TRY(widen(core, code, n, dst, s));
  *out = dst;
  return NDMPS_OK;
}

// Room for the fp64 copies of a list's cores, chain by chain and site by site: null where a core is fp64 already.
// Without codes (the size query) every core counts as if it had to be widened.
static inline void carve_list64(const ChainList& l, Arena& ar, std::vector<double*>& w) {
  w.assign((size_t)l.count * l.L, nullptr);
  for (int a = 0; a < l.count; ++a)
    for (int j = 0; j < l.L; ++j)
      if (!l.codes || l.codes[a] != 2) w[(size_t)a * l.L + j] = ar.take<double>(l.core_elems(a, j));
}
// the list's cores in fp64, widened into the room of carve_list64 where they have to be
static inline int fill_list64(const ChainList& l, const std::vector<double*>& w, hipStream_t s, std::vector<const double*>& out) {
  out.resize((size_t)l.count * l.L);
  for (int a = 0; a < l.count; ++a)
    for (int j = 0; j < l.L; ++j) {
      const size_t e = (size_t)a * l.L + j;
      NDMPS_TRY(core64(l.cores[e], l.codes[a], l.core_elems(a, j), w[e], s, &out[e]));
    }
  return NDMPS_OK;
}

// The fp64 copies of two lists.  A symmetric call with codes carves and widens list a only, and list b shares its
// copies; the size query counts both lists.
struct WidenedLists {
  std::vector<double*> wa, wb;
  std::vector<const double*> A, B;  // count x L each, after fill()
  void carve(const ChainList& a, const ChainList& b, bool symmetric, Arena& ar) {
    carve_list64(a, ar, wa);
    wb.assign((size_t)b.count * b.L, nullptr);
    if (!symmetric || !a.codes) carve_list64(b, ar, wb);
  }
  int fill(const ChainList& a, const ChainList& b, bool symmetric, hipStream_t s) {
    NDMPS_TRY(fill_list64(a, wa, s, A));
    if (symmetric) B = A;
    else NDMPS_TRY(fill_list64(b, wb, s, B));
    return NDMPS_OK;
  }
};

// what a kernel reads of two lists: the device tables of ChainTables
struct PairListArgs {
  const void* const* cores_a;  // Ka x L
  const void* const* cores_b;  // Kb x L
  const int* bonds_a;          // Ka x (L + 1)
  const int* bonds_b;          // Kb x (L + 1)
  const int* codes_a;          // storage codes: 0 fp32, 1 bf16, 2 fp64
  const int* codes_b;
  int L;
};

// The device tables cores / bonds / codes of two lists, list a then list b in each.  upload() enqueues the copies from
// host vectors that live here: the caller synchronises the stream before this object goes away.
struct ChainTables {
  const void** cores = nullptr;
  int *bonds = nullptr, *codes = nullptr;
  std::vector<const void*> hc;
  std::vector<int> hb, hk;
  void carve(const ChainList& a, const ChainList& b, Arena& ar) {
    const int64_t K = (int64_t)a.count + b.count;
    cores = ar.take<const void*>(K * a.L);
    bonds = ar.take<int>(K * (a.L + 1));
    codes = ar.take<int>(K);
  }
  int upload(const ChainList& a, const ChainList& b, hipStream_t s, PairListArgs& g) {
    const int L = a.L;
    hc.assign(a.cores, a.cores + (size_t)a.count * L);
    hc.insert(hc.end(), b.cores, b.cores + (size_t)b.count * L);
    hb.resize((size_t)(a.count + b.count) * (L + 1));
    for (size_t e = 0; e < (size_t)a.count * (L + 1); ++e) hb[e] = (int)a.bonds[e];
    for (size_t e = 0; e < (size_t)b.count * (L + 1); ++e) hb[(size_t)a.count * (L + 1) + e] = (int)b.bonds[e];
    hk.assign(a.codes, a.codes + a.count);
    hk.insert(hk.end(), b.codes, b.codes + b.count);
    NDMPS_CHECK_HIP(hipMemcpyAsync(cores, hc.data(), hc.size() * sizeof(void*), hipMemcpyHostToDevice, s));
    NDMPS_CHECK_HIP(hipMemcpyAsync(bonds, hb.data(), hb.size() * sizeof(int), hipMemcpyHostToDevice, s));
    NDMPS_CHECK_HIP(hipMemcpyAsync(codes, hk.data(), hk.size() * sizeof(int), hipMemcpyHostToDevice, s));
    g.cores_a = cores;
    g.cores_b = cores + (size_t)a.count * L;
    g.bonds_a = bonds;
    g.bonds_b = bonds + (size_t)a.count * (L + 1);
    g.codes_a = codes;
    g.codes_b = codes + a.count;
    g.L = L;
    return NDMPS_OK;
  }
};

// (a, b) of every pair of a call, two ints per pair, a ascending and b ascending inside; a symmetric call has a <= b
static inline std::vector<int> pair_table(int Ka, int Kb, bool symmetric) {
  std::vector<int> t;
  t.reserve(2 * (symmetric ? (size_t)Ka * (Ka + 1) / 2 : (size_t)Ka * Kb));
  for (int a = 0; a < Ka; ++a)
    for (int c = symmetric ? a : 0; c < Kb; ++c) t.push_back(a), t.push_back(c);
  return t;
}

// The forward sandwich of the general route on fp64 cores A64 (ca, d, ca2) and B64 (cb, d, cb2), for n matrices E:
//   T (n ca x d cb2) = E (n ca x cb) B (cb x d cb2);   out[rho, i] (ca2 x cb2) = A_i^T T[rho][:, i, :]
// by one ndmps_dgemm and ndmps_dgemm_batched over the (rho, i) in chunks of ndmps_gemm_batched_max().
static inline int sandwich_forward_general(int64_t ca, int64_t ca2, int64_t cb, int64_t cb2, int64_t d, int64_t n, const double* A64,
                                           const double* B64, const double* E, double* out, double* T, hipStream_t s) {
  const int chunk = ndmps_gemm_batched_max();
  std::vector<const double*> pa(chunk), pb(chunk);
  std::vector<double*> pc(chunk);
  NDMPS_TRY(ndmps_dgemm(0, 0, n * ca, d * cb2, cb, E, cb, B64, d * cb2, T, d * cb2, s));
  for (int64_t t0 = 0; t0 < n * d; t0 += chunk) {
    const int nb = (int)std::min<int64_t>(chunk, n * d - t0);
    for (int q = 0; q < nb; ++q) {
      const int64_t rho = (t0 + q) / d, i = (t0 + q) % d;
      pa[q] = A64 + i * ca2;
      pb[q] = T + rho * ca * d * cb2 + i * cb2;
      pc[q] = out + (t0 + q) * ca2 * cb2;
    }
    NDMPS_TRY(ndmps_dgemm_batched(nb, 1, 0, ca2, cb2, ca, pa.data(), d * ca2, pb.data(), d * cb2, pc.data(), cb2, s));
  }
  return NDMPS_OK;
}

}  // namespace ndmps
