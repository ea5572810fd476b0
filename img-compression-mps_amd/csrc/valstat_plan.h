// The plan of a chain contraction whose last product is REDUCED instead of stored (valstat.hip): value statistics and
// the error against an original, from the cores.  Pure host arithmetic beside chain_plan (chain_plan.h), which it
// calls and does not change: the same products in the same order, with two differences.
//
//   * the last product has destination kChainNone: its accumulator tiles go to a reducing epilogue;
//   * every earlier product that the decode plan sends to kChainOut (the caller's N-element output, used as the
//     second cumulative buffer under the parity rule) goes to kChainLeft2, a second left buffer of left_elems
//     elements.  The two left buffers alternate, so no product writes the buffer it reads.
//
// Workspace: the decode plan's workspace, then ws_left2, then the reduction scratch (the unit operand of a
// single-site chain, the partial records, the result record, the histogram's counters and its edges).
#pragma once
#include "chain_plan.h"

namespace ndmps {

constexpr int kChainLeft2 = -6;          // second cumulative buffer (stands in for the output of the decode plan)
constexpr int kChainUnit = -7;           // a 1 x 1 matrix holding 1: the left operand of a single-site chain
constexpr int kValstatMaxBins = 4096;    // edges and 32-bit counters of one workgroup fit in LDS beside the tiles
constexpr int kValstatMaxGroups = 512;   // workgroups of the reducing product (two per CU): one partial record each
constexpr int64_t kValstatRecordBytes = 64;  // a partial or result record: eight 8-byte slots

struct ChainStatsPlan {
  ChainPlan chain;       // chain_plan with the two differences above (its total_bytes: the decode plan's workspace)
  ChainProduct reduced;  // the product whose tiles are reduced: chain.products.back(), or core 0 behind the unit (L == 1)
  int64_t left2_bytes = 0, reduce_bytes = 0;
  int64_t off_left2 = 0, off_unit = 0, off_partials = 0, off_result = 0, off_hist = 0, off_edges = 0, total_bytes = 0;
};

// n_bins: bins of the histogram the workspace has room for (0: moments and error only)
inline ChainStatsPlan chain_stats_plan(int L, const int64_t* dims, const int64_t* bonds, int64_t elem_bytes,
                                       int64_t n_bins = 0) {
  ChainStatsPlan s;
  s.chain = chain_plan(L, dims, bonds, elem_bytes);
  std::vector<ChainProduct>& pr = s.chain.products;
  for (size_t i = 0; i < pr.size(); ++i) {
    if (pr[i].c == kChainOut) pr[i].c = i + 1 == pr.size() ? kChainNone : kChainLeft2;
    if (pr[i].a == kChainOut) pr[i].a = kChainLeft2;
  }
  s.reduced = pr.empty() ? ChainProduct{ChainKind::Final, 1, dims[0], 1, kChainUnit, 0, kChainNone, kChainNone} : pr.back();

  s.left2_bytes = chain_round_up(s.chain.left_elems, 64) * elem_bytes;
  s.off_left2 = chain_round_up(s.chain.total_bytes, 256);
  s.off_unit = chain_round_up(s.off_left2 + s.left2_bytes, 256);
  s.off_partials = s.off_unit + 256;
  s.off_result = s.off_partials + kValstatMaxGroups * kValstatRecordBytes;
  s.off_hist = s.off_result + 256;                                  // n_bins counters, then below / above / NaN
  s.off_edges = s.off_hist + chain_round_up((n_bins + 3) * 8, 256);  // n_bins + 1 edges in the element type
  s.total_bytes = s.off_edges + chain_round_up((n_bins + 1) * elem_bytes, 256);
  s.reduce_bytes = s.total_bytes - s.off_unit;
  return s;
}

}  // namespace ndmps
