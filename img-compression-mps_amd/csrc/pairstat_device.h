// The device layer of the statistics of TWO chains (pairstat.hip, labelpair.hip): the pair record and its epilogue, the
// product kernel that forms both accumulator tiles of a tile index, its launch and the argument check of a pair.
// Internal linkage, as valstat_device.h: each translation unit gets its own copy of what it uses.
#pragma once
#include "pairstat_plan.h"
#include "valstat_device.h"

namespace {

using ndmps::ChainPairPlan;

// the pair moments as a thread, a wavefront and a workgroup hold them
struct PairRecord {
  double sum_a, sum_b, sumsq_a, sumsq_b, sum_ab, sse;
  double min_a, max_a, min_b, max_b, max_abs_diff;
  long long count, n_nan;  // voxels where neither value is NaN / where either is

  __device__ __forceinline__ void clear() {
    sum_a = sum_b = sumsq_a = sumsq_b = sum_ab = sse = 0.0;
    min_a = min_b = INFINITY;
    max_a = max_b = max_abs_diff = -INFINITY;
    count = n_nan = 0;
  }
  __device__ __forceinline__ void fold(const PairRecord& b) {
    sum_a += b.sum_a;
    sum_b += b.sum_b;
    sumsq_a += b.sumsq_a;
    sumsq_b += b.sumsq_b;
    sum_ab += b.sum_ab;
    sse += b.sse;
    min_a = fmin(min_a, b.min_a);
    max_a = fmax(max_a, b.max_a);
    min_b = fmin(min_b, b.min_b);
    max_b = fmax(max_b, b.max_b);
    max_abs_diff = fmax(max_abs_diff, b.max_abs_diff);
    count += b.count;
    n_nan += b.n_nan;
  }
};
// a partial or the result in the workspace (ndmps::kPairstatRecordBytes): the thirteen fields and three spare slots
struct PairSlot : PairRecord {
  long long unused[3];
};
static_assert(sizeof(PairSlot) == ndmps::kPairstatRecordBytes, "record layout");

// ------------------------------------------------------------------------------------------------ the record epilogue
// (the contract: valstat_device.h; take() gets the pair of one accumulator slot.  An epilogue that may stand behind
// OriginalEpi (labelpair.hip) also has take_at(args, at, va, vb): a valid pair whose C-order address is already known.)
struct PairRecordArgs {
  PairSlot* partials;  // one per workgroup
};

template <typename T>
struct PairRecordEpi {
  typedef PairRecordArgs Args;
  PairRecord r;
  __device__ __forceinline__ void begin(const Args&) { r.clear(); }
  __device__ __forceinline__ void take(const Args&, bool valid, int64_t, int64_t, T va, T vb) {
    if (!valid) return;
    if (va != va || vb != vb) {
      ++r.n_nan;
      return;
    }
    ++r.count;
    const double a = (double)va, b = (double)vb, d = a - b;
    r.sum_a += a;
    r.sumsq_a += a * a;
    r.min_a = fmin(r.min_a, a);
    r.max_a = fmax(r.max_a, a);
    r.sum_b += b;
    r.sumsq_b += b * b;
    r.min_b = fmin(r.min_b, b);
    r.max_b = fmax(r.max_b, b);
    r.sum_ab += a * b;
    r.sse += d * d;
    r.max_abs_diff = fmax(r.max_abs_diff, fabs(d));
  }
  __device__ __forceinline__ void take_at(const Args& a, int64_t, T va, T vb) { take(a, true, 0, 0, va, vb); }
  __device__ __forceinline__ void finish(const Args& a) { stat_fold_group<PairRecord>(r, &a.partials[blockIdx.x]); }
};

// ------------------------------------------------------------------------------------------------ the product
// Ca = Aa (m x ka) Ba (ka x n) and Cb = Ab (m x kb) Bb (kb x n), dense row-major, tile by tile on a persistent grid:
// both accumulator tiles of a tile index, one after the other through the same staging buffers, then the pairs
// (valid, row, col, Ca[row, col], Cb[row, col]) to the epilogue.  Rows and columns beyond m and n are staged as zeros
// and handed over as invalid.  perm_a / perm_b: the column order of Ba / Bb inside the kernel (NULL: as stored), as
// valstat_product_kernel takes it; an epilogue that reads through col_off needs both chains in the order of col_off.
template <typename T, typename Epi>
__global__ void __launch_bounds__(256)
pairstat_product_kernel(const T* __restrict__ Aa, const T* __restrict__ Ba, const int32_t* __restrict__ perm_a, int64_t ka,
                        const T* __restrict__ Ab, const T* __restrict__ Bb, const int32_t* __restrict__ perm_b, int64_t kb,
                        int64_t m, int64_t n, const typename Epi::Args args) {
  __shared__ typename StatTile<T>::StageA As;
  __shared__ typename StatTile<T>::StageB Bs;

  Epi epi;
  epi.begin(args);

  const int64_t tiles_n = (n + kBN - 1) / kBN, tiles = (m + kBM - 1) / kBM * tiles_n;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t m0 = (t / tiles_n) * kBM, n0 = (t % tiles_n) * kBN;
    typename StatTile<T>::Frag acc_a[StatTile<T>::kFrags], acc_b[StatTile<T>::kFrags];
    stat_tile_accumulate<T>(Aa, Ba, perm_a, m, n, ka, m0, n0, As, Bs, acc_a);
    stat_tile_accumulate<T>(Ab, Bb, perm_b, m, n, kb, m0, n0, As, Bs, acc_b);
    stat_tile_for_each<T>(m0, n0, m, n, [&](bool valid, int64_t row, int64_t col, int i, int r) {
      epi.take(args, valid, row, col, acc_a[i][r], acc_b[i][r]);
    });
  }
  epi.finish(args);
}

// the pair product over the operands of two run chains (each with the column order its run() left in ops.perm)
template <typename T, typename Epi>
int pairstat_launch(const StatCall<T>& a, const StatCall<T>& b, const typename Epi::Args& args, int grid, size_t lds) {
  hipLaunchKernelGGL((pairstat_product_kernel<T, Epi>), dim3(grid), dim3(256), lds, a.s, (const T*)a.ops.A, (const T*)a.ops.B,
                     a.ops.perm, a.q.k, (const T*)b.ops.A, (const T*)b.ops.B, b.ops.perm, b.q.k, a.q.m, a.q.n, args);
  NDMPS_LAUNCH_CHECK();
  return NDMPS_OK;
}

// The argument check of a pair entry, before the first launch: each chain as the single-chain entries check it, on its
// own part of the workspace (tables: the offset tables of an entry that reads through them, else NULL), then the pair.
template <typename T>
int pairstat_check(const ChainPairPlan& pp, const StatCall<T>& a, const StatCall<T>& b, const int64_t* dims,
                   const int64_t* bonds_a, const int64_t* bonds_b, int64_t ws_bytes, const ErrorTables* tables = nullptr) {
  NDMPS_TRY(a.check(dims, bonds_a, ws_bytes, tables));
  NDMPS_TRY(b.check(dims, bonds_b, ws_bytes - pp.off_b, tables));
  NDMPS_REQUIRE(!pp.error, "pairstat: %s", pp.error ? pp.error : "");
  if (ws_bytes < pp.total_bytes) {
    ndmps::set_error("pairstat workspace too small: %lld < %lld", (long long)ws_bytes, (long long)pp.total_bytes);
    return NDMPS_EWORKSPACE;
  }
  return NDMPS_OK;
}

}  // namespace
