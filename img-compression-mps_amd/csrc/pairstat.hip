// Statistics of TWO chains of one shape and one factorisation, from the cores: the joint histogram (and from it the
// mutual information) and the pair moments of the volumes they decode to, with neither volume written.
//
//   ndmps_pairstat_moments_*    <- NDMPS.pair_stats                                    (core/pairstat.py)
//   ndmps_pairstat_histogram_*  <- NDMPS.joint_histogram / mutual_information(_many)
//
// chain_pair_plan (pairstat_plan.h) is chain_stats_plan once per chain, the two workspaces back to back, and the pair
// scratch behind them.  chain_plan decides the m x n of the last product from the physical dims alone, so the two
// last products have the same rows and columns with the same meaning and differ only in k.  Every product before the
// last runs per chain exactly as the single-chain statistics run it (valstat_run_chain); then ONE kernel forms, tile
// by tile, the accumulator tile of a and the accumulator tile of b through the same LDS staging buffers, so that
// voxel x of a and voxel x of b sit in the same register slot of the same lane, and hands the pairs to an epilogue:
//
//   PairRecord  over the voxels where neither value is NaN: their number, sum a, sum b, sum a^2, sum b^2, sum a b,
//               sum (a - b)^2 in fp64, min / max of either, max |a - b|; the others are counted in n_nan.
//   JointHist   numpy.histogram2d against two explicit edge tables held in LDS: cell ia * bins_b + ib, each index by
//               the binary search of the single-chain histogram (last bin closed on the right, exact for the computed
//               value).  A voxel with either value NaN goes to n_nan, otherwise one with either value out of range
//               to outside.  32-bit counters in LDS per workgroup, flushed once with 64-bit integer atomics; before
//               the LDS atomic a wavefront folds the lanes that share the first lane's cell into one add (the
//               background of two medical volumes is one cell).
//
// A voxel's value is computed by the one text valstat_product_kernel computes it by (stat_tile_accumulate,
// valstat_device.h: its k order, its zero padding), so the marginals of the joint histogram are the single-chain
// histograms bit for bit.  Determinism as there: tile t goes to workgroup t mod grid, a fixed shuffle tree, one
// partial record per workgroup folded in index order, and only integers are added atomically.
#include <mutex>

#include "common.h"
#include "pairstat_device.h"
#include "pairstat_plan.h"
#include "typed.h"
#include "valstat_device.h"

namespace {

// ------------------------------------------------------------------------------------------------ epilogues
// (PairRecord, PairRecordEpi and the product kernel: pairstat_device.h)
struct JointHistArgs {
  const void *edges_a, *edges_b;  // [bins_a + 1], [bins_b + 1] in the element type, ascending
  unsigned long long* counts;     // [bins_a * bins_b + 2]: the cells, then outside, then NaN
  int bins_a, bins_b;
};

extern __shared__ double pairstat_dyn_lds[];  // the edges of a, the edges of b, then the 32-bit counters

// bytes of the dynamic LDS of a joint histogram
inline size_t joint_hist_lds(int bins_a, int bins_b, size_t elem_bytes) {
  return ((size_t)(bins_a + 1) * elem_bytes + 7) / 8 * 8 + ((size_t)(bins_b + 1) * elem_bytes + 7) / 8 * 8 +
         ((size_t)bins_a * bins_b + 2) * 4;
}
constexpr size_t kJointHistMaxLds = 2 * (size_t)(ndmps::kPairstatMaxAxisBins + 1) * 8 + ((size_t)ndmps::kPairstatMaxCells + 2) * 4;

template <typename T>
struct JointHistEpi {
  typedef JointHistArgs Args;
  T *ea, *eb;
  unsigned int* cnt;
  __device__ __forceinline__ void begin(const Args& a) {
    const int cells = a.bins_a * a.bins_b;
    double* at = pairstat_dyn_lds;
    ea = reinterpret_cast<T*>(at);
    at += ((size_t)(a.bins_a + 1) * sizeof(T) + 7) / 8;
    eb = reinterpret_cast<T*>(at);
    at += ((size_t)(a.bins_b + 1) * sizeof(T) + 7) / 8;
    cnt = reinterpret_cast<unsigned int*>(at);
    for (int i = threadIdx.x; i <= a.bins_a; i += 256) ea[i] = static_cast<const T*>(a.edges_a)[i];
    for (int i = threadIdx.x; i <= a.bins_b; i += 256) eb[i] = static_cast<const T*>(a.edges_b)[i];
    for (int i = threadIdx.x; i < cells + 2; i += 256) cnt[i] = 0u;
    __syncthreads();
  }
  __device__ __forceinline__ void take(const Args& a, bool valid, int64_t, int64_t, T va, T vb) {
    int cell = -1;
    if (valid) {
      const int cells = a.bins_a * a.bins_b;
      const int ia = valstat_bin(ea, a.bins_a, va), ib = valstat_bin(eb, a.bins_b, vb);
      if (ia == a.bins_a + 2 || ib == a.bins_b + 2)
        cell = cells + 1;  // NaN wins over out of range
      else if (ia >= a.bins_a || ib >= a.bins_b)
        cell = cells;
      else
        cell = ia * a.bins_b + ib;
    }
    valstat_add_folded(cnt, cell);
  }
  __device__ __forceinline__ void finish(const Args& a) {
    __syncthreads();
    const int cells = a.bins_a * a.bins_b;
    for (int i = threadIdx.x; i < cells + 2; i += 256)
      if (cnt[i]) atomicAdd(&a.counts[i], (unsigned long long)cnt[i]);
  }
};

// ------------------------------------------------------------------------------------------------ host
// the joint histogram may ask for more than 64 KB of dynamic LDS: opted in once per device
int pairstat_opt_in() {
  static std::mutex mu;
  static bool done[64] = {};
  int dev = 0;
  NDMPS_CHECK_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  if (dev < 0 || dev >= 64 || done[dev]) return NDMPS_OK;
  NDMPS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&pairstat_product_kernel<float, JointHistEpi<float>>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)kJointHistMaxLds));
  NDMPS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&pairstat_product_kernel<double, JointHistEpi<double>>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)kJointHistMaxLds));
  done[dev] = true;
  return NDMPS_OK;
}

// h_stats[11] = {sum a, sum b, sum a^2, sum b^2, sum a b, sum (a - b)^2, min a, max a, min b, max b, max |a - b|},
// h_counts[2] = {voxels where neither value is NaN, voxels where either is}
template <typename T>
int pairstat_moments(int L, const int64_t* h_dims, const int64_t* h_bonds_a, const int64_t* h_bonds_b,
                     const T* const* h_cores_a, const T* const* h_cores_b, double* h_stats, int64_t* h_counts, void* d_ws,
                     int64_t ws_bytes, ndmps_stream_t stream) {
  NDMPS_REQUIRE(L >= 1 && h_dims && h_bonds_a && h_bonds_b && h_stats && h_counts, "bad pairstat argument");
  const ChainPairPlan pp = ndmps::chain_pair_plan(L, h_dims, h_bonds_a, h_bonds_b, sizeof(T));
  StatCall<T> a(pp.a, h_cores_a, d_ws, stream), b(pp.b, h_cores_b, (char*)d_ws + pp.off_b, stream);
  NDMPS_TRY(pairstat_check(pp, a, b, h_dims, h_bonds_a, h_bonds_b, ws_bytes));
  NDMPS_TRY(a.run(nullptr));
  NDMPS_TRY(b.run(nullptr));
  PairSlot* partials = (PairSlot*)(a.ws + pp.off_partials);
  PairSlot* result = (PairSlot*)(a.ws + pp.off_result);
  const PairRecordArgs args{partials};
  NDMPS_TRY((pairstat_launch<T, PairRecordEpi<T>>(a, b, args, a.grid, 0)));
  PairRecord host;
  NDMPS_TRY((stat_fetch_record<PairRecord>(partials, a.grid, result, &host, a.s)));
  const double stats[11] = {host.sum_a, host.sum_b, host.sumsq_a, host.sumsq_b, host.sum_ab, host.sse,
                            host.min_a, host.max_a, host.min_b, host.max_b, host.max_abs_diff};
  std::copy(stats, stats + 11, h_stats);
  h_counts[0] = host.count, h_counts[1] = host.n_nan;
  return NDMPS_OK;
}

// h_counts[bins_a * bins_b + 2]: the cells (row-major, a along the rows), then outside, then n_nan
template <typename T>
int pairstat_histogram(int L, const int64_t* h_dims, const int64_t* h_bonds_a, const int64_t* h_bonds_b,
                       const T* const* h_cores_a, const T* const* h_cores_b, const T* h_edges_a, int bins_a,
                       const T* h_edges_b, int bins_b, int64_t* h_counts, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  NDMPS_REQUIRE(L >= 1 && h_dims && h_bonds_a && h_bonds_b && h_edges_a && h_edges_b && h_counts, "bad pairstat argument");
  NDMPS_REQUIRE(bins_a >= 1 && bins_a <= ndmps::kPairstatMaxAxisBins && bins_b >= 1 && bins_b <= ndmps::kPairstatMaxAxisBins,
                "joint histogram: %d x %d bins, an axis takes 1 to %d", bins_a, bins_b, ndmps::kPairstatMaxAxisBins);
  NDMPS_REQUIRE((int64_t)bins_a * bins_b <= ndmps::kPairstatMaxCells, "joint histogram: %d x %d bins are more than %d cells",
                bins_a, bins_b, ndmps::kPairstatMaxCells);
  NDMPS_TRY(stat_edges_ok(h_edges_a, bins_a, "joint histogram: edges of a"));
  NDMPS_TRY(stat_edges_ok(h_edges_b, bins_b, "joint histogram: edges of b"));
  const int cells = bins_a * bins_b;
  const ChainPairPlan pp = ndmps::chain_pair_plan(L, h_dims, h_bonds_a, h_bonds_b, sizeof(T), cells, bins_a, bins_b);
  StatCall<T> a(pp.a, h_cores_a, d_ws, stream), b(pp.b, h_cores_b, (char*)d_ws + pp.off_b, stream);
  NDMPS_TRY(pairstat_check(pp, a, b, h_dims, h_bonds_a, h_bonds_b, ws_bytes));
  const size_t lds = joint_hist_lds(bins_a, bins_b, sizeof(T));
  const int64_t tiles = stat_tiles(a.q);
  // above 64 KB of counters and edges a CU holds one workgroup
  const int grid = (int)std::min<int64_t>(tiles, lds > 65536 ? ndmps::kNumCU : ndmps::kValstatMaxGroups);
  NDMPS_TRY(stat_counters_fit(tiles, grid, "joint histogram"));
  NDMPS_TRY(pairstat_opt_in());
  NDMPS_TRY(a.run(nullptr));
  NDMPS_TRY(b.run(nullptr));
  hipStream_t s = a.s;
  char* ws = a.ws;
  unsigned long long* counts = (unsigned long long*)(ws + pp.off_counts);
  T* edges_a = (T*)(ws + pp.off_edges_a);
  T* edges_b = (T*)(ws + pp.off_edges_b);
  NDMPS_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)(cells + 2) * 8, s));
  NDMPS_CHECK_HIP(hipMemcpyAsync(edges_a, h_edges_a, (size_t)(bins_a + 1) * sizeof(T), hipMemcpyHostToDevice, s));
  NDMPS_CHECK_HIP(hipMemcpyAsync(edges_b, h_edges_b, (size_t)(bins_b + 1) * sizeof(T), hipMemcpyHostToDevice, s));
  const JointHistArgs args{edges_a, edges_b, counts, bins_a, bins_b};
  NDMPS_TRY((pairstat_launch<T, JointHistEpi<T>>(a, b, args, grid, lds)));
  static_assert(sizeof(int64_t) == sizeof(unsigned long long), "counter width");
  NDMPS_CHECK_HIP(hipMemcpyAsync(h_counts, counts, (size_t)(cells + 2) * 8, hipMemcpyDeviceToHost, s));
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));
  return NDMPS_OK;
}

bool pairstat_bins_ok(int64_t bins_a, int64_t bins_b) {
  if (bins_a == 0 && bins_b == 0) return true;  // the moments call
  return bins_a >= 1 && bins_a <= ndmps::kPairstatMaxAxisBins && bins_b >= 1 && bins_b <= ndmps::kPairstatMaxAxisBins &&
         bins_a * bins_b <= ndmps::kPairstatMaxCells;
}

}  // namespace

extern "C" int64_t ndmps_pairstat_workspace_bytes(int L, const int64_t* h_dims, const int64_t* h_bonds_a,
                                                  const int64_t* h_bonds_b, int64_t elem_bytes, int64_t bins_a,
                                                  int64_t bins_b) {
  if (L < 1 || !h_dims || !h_bonds_a || !h_bonds_b || (elem_bytes != 4 && elem_bytes != 8) || !pairstat_bins_ok(bins_a, bins_b))
    return 0;
  const ChainPairPlan pp = ndmps::chain_pair_plan(L, h_dims, h_bonds_a, h_bonds_b, elem_bytes, bins_a * bins_b, bins_a, bins_b);
  return pp.error ? 0 : pp.total_bytes;
}

// The plan of a pair call, for tests and tools (slot order: include/ndmps_hip.h).  Host arithmetic only.
extern "C" int ndmps_pairstat_plan_query(int elem, int L, const int64_t* h_dims, const int64_t* h_bonds_a,
                                         const int64_t* h_bonds_b, int64_t bins_a, int64_t bins_b, int64_t* h_out) {
  NDMPS_REQUIRE(h_out && (elem == 0 || elem == 2) && L >= 1 && h_dims && h_bonds_a && h_bonds_b,
                "bad pairstat plan query (elem=%d)", elem);
  NDMPS_REQUIRE(bins_a <= ndmps::kPairstatMaxAxisBins && bins_b <= ndmps::kPairstatMaxAxisBins,
                "joint histogram: %lld x %lld bins, an axis takes 1 to %d", (long long)bins_a, (long long)bins_b,
                ndmps::kPairstatMaxAxisBins);
  NDMPS_REQUIRE(bins_a * bins_b <= ndmps::kPairstatMaxCells, "joint histogram: %lld x %lld bins are more than %d cells",
                (long long)bins_a, (long long)bins_b, ndmps::kPairstatMaxCells);
  NDMPS_REQUIRE(pairstat_bins_ok(bins_a, bins_b), "joint histogram: %lld x %lld bins: both at least 1, or both 0 for the moments",
                (long long)bins_a, (long long)bins_b);
  const ChainPairPlan pp = ndmps::chain_pair_plan(L, h_dims, h_bonds_a, h_bonds_b, elem == 2 ? 8 : 4, bins_a * bins_b, bins_a, bins_b);
  NDMPS_REQUIRE(!pp.error, "pairstat: %s", pp.error ? pp.error : "");
  const int64_t out[NDMPS_PAIRSTAT_PLAN_SLOTS] = {pp.a.reduced.m,  pp.a.reduced.n, pp.a.reduced.k, pp.b.reduced.k,
                                                  pp.a.total_bytes, pp.b.total_bytes, pp.off_b,      pp.off_partials,
                                                  pp.off_result,    pp.off_counts,    pp.off_edges_a, pp.off_edges_b,
                                                  pp.pair_bytes,    pp.total_bytes};
  std::copy(out, out + NDMPS_PAIRSTAT_PLAN_SLOTS, h_out);
  return NDMPS_OK;
}

extern "C" int ndmps_pairstat_moments_f32(int L, const int64_t* h_dims, const int64_t* h_bonds_a, const int64_t* h_bonds_b,
                                          const float* const* h_cores_a, const float* const* h_cores_b, double* h_stats,
                                          int64_t* h_counts, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  return pairstat_moments<float>(L, h_dims, h_bonds_a, h_bonds_b, h_cores_a, h_cores_b, h_stats, h_counts, d_ws, ws_bytes, stream);
}
extern "C" int ndmps_pairstat_moments_f64(int L, const int64_t* h_dims, const int64_t* h_bonds_a, const int64_t* h_bonds_b,
                                          const double* const* h_cores_a, const double* const* h_cores_b, double* h_stats,
                                          int64_t* h_counts, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  return pairstat_moments<double>(L, h_dims, h_bonds_a, h_bonds_b, h_cores_a, h_cores_b, h_stats, h_counts, d_ws, ws_bytes, stream);
}
extern "C" int ndmps_pairstat_histogram_f32(int L, const int64_t* h_dims, const int64_t* h_bonds_a, const int64_t* h_bonds_b,
                                            const float* const* h_cores_a, const float* const* h_cores_b,
                                            const float* h_edges_a, int bins_a, const float* h_edges_b, int bins_b,
                                            int64_t* h_counts, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  return pairstat_histogram<float>(L, h_dims, h_bonds_a, h_bonds_b, h_cores_a, h_cores_b, h_edges_a, bins_a, h_edges_b, bins_b,
                                   h_counts, d_ws, ws_bytes, stream);
}
extern "C" int ndmps_pairstat_histogram_f64(int L, const int64_t* h_dims, const int64_t* h_bonds_a, const int64_t* h_bonds_b,
                                            const double* const* h_cores_a, const double* const* h_cores_b,
                                            const double* h_edges_a, int bins_a, const double* h_edges_b, int bins_b,
                                            int64_t* h_counts, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  return pairstat_histogram<double>(L, h_dims, h_bonds_a, h_bonds_b, h_cores_a, h_cores_b, h_edges_a, bins_a, h_edges_b, bins_b,
                                    h_counts, d_ws, ws_bytes, stream);
}
