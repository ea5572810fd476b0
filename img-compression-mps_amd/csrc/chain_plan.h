// The plan of a chain contraction (chain.hip): which products run, in which order, between which buffers, and how
// the workspace is laid out.  Pure host arithmetic in plain C++17 -- no HIP call, no environment, no globals -- so
// it compiles and is tested without a GPU; the executor (run_chain), every size query and ndmps_chain_plan_query
// answer from it.
//
// The tail of a chain is the longest run of trailing sites, never site 0, whose physical dims multiply to at most
// kChainTailMax.  Its sites j0 .. L-1 are contracted among themselves first, right to left, into R (k_{j0} x
// N_{j0}); the sites before it are contracted cumulatively, left to right; one final product Left R joins the two
// and is the only one that writes N elements.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace ndmps {

constexpr int64_t kChainTailMax = 4096;

enum class ChainKind : int { Tail = 0, Left = 1, Final = 2 };

// operand of a product: core i (>= 0), one of the three workspace buffers, or the caller's output
constexpr int kChainLeft = -1, kChainTail0 = -2, kChainTail1 = -3, kChainOut = -4, kChainNone = -5;

struct ChainProduct {  // C (m x n) = A (m x k) B (k x n), all row-major and dense
  ChainKind kind;
  int64_t m, n, k;
  int a, b, c;
  int spare;  // Final: the tail buffer that does not hold R (takes R's columns in memory order); else kChainNone
};

struct ChainPlan {
  int L = 0;
  int j0 = 0;             // first site of the pre-contracted tail (== L: no tail, j0 == 0 never)
  int64_t tail_cols = 0;  // N_{j0} = product of the dims of the tail sites, 0 without a tail
  int64_t numel = 1;      // N = product of all dims: the elements of the output
  int64_t left_elems = 0, tail_elems = 0;  // capacity of ws_left / of either tail buffer, in elements
  // workspace: ws_left, ws_tail0, ws_tail1, then the transposed right operand of a bf16 product
  int64_t off_left = 0, off_tail0 = 0, off_tail1 = 0, off_scratch = 0, total_bytes = 0;
  std::vector<ChainProduct> products;  // L - 1 of them; the last one writes kChainOut

  bool has_tail() const { return j0 < L; }
};

inline int64_t chain_round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// elem_bytes: 4 for fp32 and bf16 cores (the fp32 size covers the bf16 intermediates), 8 for fp64
inline ChainPlan chain_plan(int L, const int64_t* dims, const int64_t* bonds, int64_t elem_bytes) {
  ChainPlan p;
  p.L = p.j0 = L;
  int64_t right = 1;
  for (int i = L - 1; i >= 1; --i) {
    if (right * dims[i] > kChainTailMax) break;
    right *= dims[i];
    p.j0 = i;
  }
  if (p.has_tail()) p.tail_cols = right;

  // ---- tail, right to left: R_i (k_i x N_i) = [core_i as (k_i d_i) x k_{i+1}] R_{i+1}, each into the tail buffer
  //      that does not hold R_{i+1}
  const auto other_tail = [](int R) { return R == kChainTail0 ? kChainTail1 : kChainTail0; };
  int R = L - 1;
  int64_t n_tail = dims[L - 1];
  for (int i = L - 2; i >= p.j0; --i) {
    p.products.push_back({ChainKind::Tail, bonds[i] * dims[i], n_tail, bonds[i + 1], i, R, other_tail(R), kChainNone});
    R = other_tail(R);
    n_tail *= dims[i];
  }
  // ---- left part, cumulative: Left_i (rows_i x k_{i+1}) = Left_{i-1} [core_i as k_i x (d_i k_{i+1})].  The last
  //      product of the whole chain writes the output; going back from it, the destinations alternate between the
  //      output and ws_left, so no product writes the buffer it reads
  const int last_left = p.has_tail() ? p.j0 - 1 : L - 1;  // site of the last cumulative product, 0: none
  int left = 0;
  int64_t rows = dims[0];
  for (int i = 1; i <= last_left; ++i) {
    const int remaining = (last_left - i) + (p.has_tail() ? 1 : 0);  // products after this one
    const int dst = remaining % 2 == 0 ? kChainOut : kChainLeft;
    p.products.push_back({ChainKind::Left, rows, dims[i] * bonds[i + 1], bonds[i], left, i, dst, kChainNone});
    left = dst;
    rows *= dims[i];
  }
  if (p.has_tail())
    p.products.push_back({ChainKind::Final, rows, n_tail, bonds[p.j0], left, R, kChainOut, other_tail(R)});

  // ---- capacities: every Left_i of a site before the tail, every R_i of a tail site
  for (int i = 0; i < L; ++i) p.numel *= dims[i];
  rows = 1;
  for (int i = 0; i < p.j0; ++i) {
    rows *= dims[i];
    p.left_elems = std::max(p.left_elems, rows * bonds[i + 1]);
  }
  int64_t n = 1;
  for (int i = L - 1; i >= p.j0; --i) {
    n *= dims[i];
    p.tail_elems = std::max(p.tail_elems, bonds[i] * n);
  }
  int64_t biggest_b = p.tail_elems;  // right operand of a bf16 product: a core or a tail matrix
  for (int i = 0; i < L; ++i) biggest_b = std::max(biggest_b, bonds[i] * dims[i] * bonds[i + 1]);
  p.off_tail0 = p.off_left + chain_round_up(p.left_elems, 64) * elem_bytes;
  p.off_tail1 = p.off_tail0 + chain_round_up(p.tail_elems, 64) * elem_bytes;
  p.off_scratch = p.off_tail1 + chain_round_up(p.tail_elems, 64) * elem_bytes;
  p.total_bytes = p.off_scratch + chain_round_up(biggest_b * 2, 256) + 1024;
  return p;
}

}  // namespace ndmps
