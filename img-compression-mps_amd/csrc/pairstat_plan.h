// The plan of a statistics call on TWO chains of one shape and one factorisation (pairstat.hip): the joint histogram
// and the pair moments of the volumes they decode to.  Pure host arithmetic beside chain_stats_plan (valstat_plan.h),
// which it calls once per chain and does not change.
//
// chain_plan decides j0, and with it the m x n of the last product, from the physical dims alone, so the two reduced
// products agree in m and n and differ only in k (the bonds at j0): element (r, c) of either is the same voxel.
//
// Workspace: the statistics workspace of a (chain_stats_plan with no bins: its products, its second left buffer, its
// unit operand for L == 1), the one of b behind it, then the pair scratch: kValstatMaxGroups partial pair records, the
// result record, cells + 2 64-bit counters (the cells row-major as ia * bins_b + ib, then outside, then n_nan) and
// the two edge tables in the element type.
#pragma once
#include "valstat_plan.h"

namespace ndmps {

constexpr int kPairstatMaxAxisBins = 1024;   // bins of one axis
constexpr int kPairstatMaxCells = 16384;     // bins_a * bins_b: 64 KiB of 32-bit counters in LDS per workgroup
constexpr int64_t kPairstatRecordBytes = 128;  // a partial or result pair record: sixteen 8-byte slots

struct ChainPairPlan {
  ChainStatsPlan a, b;       // each with its own workspace, a's at 0 and b's at off_b
  const char* error = nullptr;  // non-NULL: why the two chains make no pair
  int64_t off_b = 0, off_partials = 0, off_result = 0, off_counts = 0, off_edges_a = 0, off_edges_b = 0;
  int64_t pair_bytes = 0, total_bytes = 0;
};

// cells = bins_a * bins_b (0, 0, 0: the moments call, which has no counters and no edges)
inline ChainPairPlan chain_pair_plan(int L, const int64_t* dims, const int64_t* bonds_a, const int64_t* bonds_b,
                                     int64_t elem_bytes, int64_t cells = 0, int64_t bins_a = 0, int64_t bins_b = 0) {
  ChainPairPlan p;
  p.a = chain_stats_plan(L, dims, bonds_a, elem_bytes, 0);
  p.b = chain_stats_plan(L, dims, bonds_b, elem_bytes, 0);
  if (p.a.reduced.m != p.b.reduced.m || p.a.reduced.n != p.b.reduced.n)
    p.error = "the last products of the two chains differ in rows or columns: their voxels do not correspond";
  else if (cells != bins_a * bins_b)
    p.error = "cells is not bins_a * bins_b";
  p.off_b = chain_round_up(p.a.total_bytes, 256);
  p.off_partials = chain_round_up(p.off_b + p.b.total_bytes, 256);
  p.off_result = p.off_partials + kValstatMaxGroups * kPairstatRecordBytes;
  p.off_counts = p.off_result + 256;
  const bool hist = cells > 0;
  p.off_edges_a = p.off_counts + (hist ? chain_round_up((cells + 2) * 8, 256) : 0);
  p.off_edges_b = p.off_edges_a + (hist ? chain_round_up((bins_a + 1) * elem_bytes, 256) : 0);
  p.total_bytes = p.off_edges_b + (hist ? chain_round_up((bins_b + 1) * elem_bytes, 256) : 0);
  p.pair_bytes = p.total_bytes - p.off_partials;
  return p;
}

}  // namespace ndmps
