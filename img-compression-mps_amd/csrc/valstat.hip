// Value statistics and the error against an original, from the cores: the chain contraction whose last product is
// reduced in registers and LDS instead of stored, so the N voxels are never written.
//
//   ndmps_valstat_moments_*    <- NDMPS.value_stats / min / max      (core/valstat.py)
//   ndmps_valstat_histogram_*  <- NDMPS.histogram / quantile
//   ndmps_valstat_error_*      <- NDMPS.error_to / psnr_to
//
// chain_stats_plan (valstat_plan.h) is chain_plan with the last product's destination removed and the output's
// role as second cumulative buffer taken by ws_left2.  Every product before the last runs through ndmps_sgemm /
// ndmps_dgemm exactly as run_chain issues them (chain.hip); the last one is valstat_product_kernel (valstat_device.h),
// a tiled MFMA product on a persistent grid whose accumulator tiles are handed, element by element, to an epilogue:
// the three below (RecordEpi stands in valstat_device.h, HistEpi here), the two of the extremes (axisext.hip) and the
// one of the label statistics (labelstat.hip):
//
//   Moments    count, min, max, sum, sum of squares, NaN count.  NaN voxels are counted and take no part in the rest.
//   Histogram  np.histogram against an explicit edge table held in LDS: bin b takes edges[b] <= v < edges[b + 1], the
//              last bin is closed on the right; below / above / NaN are counted apart.  The bin is found by binary
//              search in the table, so it is exact for the computed v.  32-bit counters in LDS per workgroup, flushed
//              once with 64-bit integer atomics.  Before the LDS atomic, a wavefront folds the lanes that share the
//              first lane's bin into one add (a background of equal voxels costs one atomic per wavefront).
//   Error      y = d_ref[row_off[r] + col_off[c]] through the additive offset tables of the fused decode:
//              sum (v - y)^2, max |v - y|, sum y^2, max y.
//
// Determinism: sums are fp64 and nothing floating-point is added atomically.  A thread's elements are a fixed
// function of the shape (tile t goes to workgroup t mod grid, the grid is a function of the tile count), a
// workgroup folds its threads by a fixed shuffle tree and writes one partial record, and stat_fold_kernel folds
// the records in index order: the same inputs give the same bits.  The histogram adds integers, the extremes
// along axes take integer maxima of order-preserving keys, and the label statistics do both on fixed-point sums:
// all associative and commutative.
#include "common.h"
#include "typed.h"
#include "valstat_device.h"  // the family's device layer and host prologue
#include "valstat_plan.h"

namespace {

struct HistArgs {
  const void* edges;              // [bins + 1] in the element type, ascending
  unsigned long long* counts;     // [bins + 3]: the bins, then below, above, NaN
  int bins;
};

// valstat_dyn_lds: the edges, then the 32-bit counters
template <typename T>
struct HistEpi {
  typedef HistArgs Args;
  T* e;
  unsigned int* cnt;
  __device__ __forceinline__ void begin(const Args& a) {
    e = reinterpret_cast<T*>(valstat_dyn_lds);
    cnt = reinterpret_cast<unsigned int*>(valstat_dyn_lds + ((size_t)(a.bins + 1) * sizeof(T) + 7) / 8);
    for (int i = threadIdx.x; i <= a.bins; i += 256) e[i] = static_cast<const T*>(a.edges)[i];
    for (int i = threadIdx.x; i < a.bins + 3; i += 256) cnt[i] = 0u;
    __syncthreads();
  }
  __device__ __forceinline__ void take(const Args& a, bool valid, int64_t, int64_t, T v) {
    const int bin = valid ? valstat_bin(e, a.bins, v) : -1;
    valstat_add_folded(cnt, bin);
  }
  __device__ __forceinline__ void finish(const Args& a) {
    __syncthreads();
    for (int i = threadIdx.x; i < a.bins + 3; i += 256)
      if (cnt[i]) atomicAdd(&a.counts[i], (unsigned long long)cnt[i]);
  }
};

// ------------------------------------------------------------------------------------------------ host
// moments (err == NULL) or the error against an original: h_stats[4], h_counts[3]
template <typename T>
int valstat_record(int L, const int64_t* h_dims, const int64_t* h_bonds, const T* const* h_cores, const ErrorTables* err,
                   double clip_lo, double clip_hi, double* h_stats, int64_t* h_counts, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  NDMPS_REQUIRE(L >= 1 && h_dims && h_bonds && h_stats && h_counts, "bad valstat argument");
  NDMPS_REQUIRE(clip_lo == clip_lo && clip_hi == clip_hi, "moments: the clip range must not be NaN");
  const ChainStatsPlan sp = ndmps::chain_stats_plan(L, h_dims, h_bonds, sizeof(T), 0);
  StatCall<T> c(sp, h_cores, d_ws, stream);
  NDMPS_TRY(c.check(h_dims, h_bonds, ws_bytes, err));
  NDMPS_TRY(c.run(err ? err->col_perm : nullptr));
  RecordArgs args{c.template partials<Record>(), nullptr, nullptr, nullptr, sp.chain.numel, clip_lo, clip_hi};
  if (err) {
    args.ref = err->ref;
    args.row_off = err->row_off;
    args.col_off = err->col_off;
    NDMPS_TRY((stat_launch<T, RecordEpi<T, true>>(c.q, c.ops, args, c.grid, 0, c.s)));
  } else {
    NDMPS_TRY((stat_launch<T, RecordEpi<T, false>>(c.q, c.ops, args, c.grid, 0, c.s)));
  }
  Record host;
  NDMPS_TRY(stat_fetch_record(args.partials, c.grid, c.template result<Record>(), &host, c.s));
  if (err) {
    h_stats[0] = host.s0, h_stats[1] = host.hi0, h_stats[2] = host.s1, h_stats[3] = host.hi1;
  } else {
    h_stats[0] = host.lo, h_stats[1] = host.hi0, h_stats[2] = host.s0, h_stats[3] = host.s1;
  }
  h_counts[0] = host.c0, h_counts[1] = host.c1, h_counts[2] = host.c2;
  return NDMPS_OK;
}

template <typename T>
int valstat_histogram(int L, const int64_t* h_dims, const int64_t* h_bonds, const T* const* h_cores, const T* h_edges,
                      int n_bins, int64_t* h_counts, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  NDMPS_REQUIRE(L >= 1 && h_dims && h_bonds && h_edges && h_counts, "bad valstat argument");
  NDMPS_REQUIRE(n_bins >= 1 && n_bins <= ndmps::kValstatMaxBins, "histogram: %d bins outside [1, %d]", n_bins,
                ndmps::kValstatMaxBins);
  NDMPS_TRY(stat_edges_ok(h_edges, n_bins, "histogram: edges"));
  const ChainStatsPlan sp = ndmps::chain_stats_plan(L, h_dims, h_bonds, sizeof(T), n_bins);
  StatCall<T> c(sp, h_cores, d_ws, stream);
  NDMPS_TRY(c.check(h_dims, h_bonds, ws_bytes, nullptr));
  NDMPS_TRY(stat_counters_fit(stat_tiles(c.q), c.grid, "histogram"));
  NDMPS_TRY(c.run(nullptr));
  hipStream_t s = c.s;
  unsigned long long* counts = (unsigned long long*)(c.ws + sp.off_hist);
  T* edges = (T*)(c.ws + sp.off_edges);
  NDMPS_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)(n_bins + 3) * 8, s));
  NDMPS_CHECK_HIP(hipMemcpyAsync(edges, h_edges, (size_t)(n_bins + 1) * sizeof(T), hipMemcpyHostToDevice, s));
  const HistArgs args{edges, counts, n_bins};
  const size_t lds = ((size_t)(n_bins + 1) * sizeof(T) + 7) / 8 * 8 + (size_t)(n_bins + 3) * 4;
  NDMPS_TRY((stat_launch<T, HistEpi<T>>(c.q, c.ops, args, c.grid, lds, s)));
  static_assert(sizeof(int64_t) == sizeof(unsigned long long), "counter width");
  NDMPS_CHECK_HIP(hipMemcpyAsync(h_counts, counts, (size_t)(n_bins + 3) * 8, hipMemcpyDeviceToHost, s));
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));
  return NDMPS_OK;
}

}  // namespace

extern "C" int64_t ndmps_valstat_workspace_bytes(int L, const int64_t* h_dims, const int64_t* h_bonds, int64_t elem_bytes,
                                                 int64_t n_bins) {
  if (L < 1 || !h_dims || !h_bonds || (elem_bytes != 4 && elem_bytes != 8) || n_bins < 0 || n_bins > ndmps::kValstatMaxBins)
    return 0;
  return ndmps::chain_stats_plan(L, h_dims, h_bonds, elem_bytes, n_bins).total_bytes;
}

// The plan of a statistics call, for tests and tools (slot order: include/ndmps_hip.h).  Host arithmetic only.
extern "C" int ndmps_valstat_plan_query(int elem, int L, const int64_t* h_dims, const int64_t* h_bonds, int64_t n_bins,
                                        int64_t* h_out) {
  NDMPS_REQUIRE(h_out && (elem == 0 || elem == 2) && L >= 1 && h_dims && h_bonds && n_bins >= 0 &&
                    n_bins <= ndmps::kValstatMaxBins,
                "bad valstat plan query (elem=%d, n_bins=%lld)", elem, (long long)n_bins);
  const ChainStatsPlan sp = ndmps::chain_stats_plan(L, h_dims, h_bonds, elem == 2 ? 8 : 4, n_bins);
  const ndmps::ChainPlan& p = sp.chain;
  const int64_t head[9] = {p.j0, p.tail_cols, (int64_t)p.products.size(), p.left_elems, p.tail_elems,
                           p.total_bytes, sp.left2_bytes, sp.reduce_bytes, sp.total_bytes};
  h_out = std::copy(head, head + 9, h_out);
  auto put = [&](const ChainProduct& q) {
    const int64_t row[8] = {(int64_t)q.kind, q.m, q.n, q.k, q.a, q.b, q.c, q.spare};
    h_out = std::copy(row, row + 8, h_out);
  };
  for (const ChainProduct& q : p.products) put(q);
  put(sp.reduced);
  return NDMPS_OK;
}

extern "C" int ndmps_valstat_moments_f32(int L, const int64_t* h_dims, const int64_t* h_bonds, const float* const* h_cores,
                                         double clip_lo, double clip_hi, double* h_stats, int64_t* h_counts, void* d_ws,
                                         int64_t ws_bytes, ndmps_stream_t stream) {
  return valstat_record<float>(L, h_dims, h_bonds, h_cores, nullptr, clip_lo, clip_hi, h_stats, h_counts, d_ws, ws_bytes, stream);
}
extern "C" int ndmps_valstat_moments_f64(int L, const int64_t* h_dims, const int64_t* h_bonds, const double* const* h_cores,
                                         double clip_lo, double clip_hi, double* h_stats, int64_t* h_counts, void* d_ws,
                                         int64_t ws_bytes, ndmps_stream_t stream) {
  return valstat_record<double>(L, h_dims, h_bonds, h_cores, nullptr, clip_lo, clip_hi, h_stats, h_counts, d_ws, ws_bytes, stream);
}
extern "C" int ndmps_valstat_histogram_f32(int L, const int64_t* h_dims, const int64_t* h_bonds, const float* const* h_cores,
                                           const float* h_edges, int n_bins, int64_t* h_counts, void* d_ws,
                                           int64_t ws_bytes, ndmps_stream_t stream) {
  return valstat_histogram<float>(L, h_dims, h_bonds, h_cores, h_edges, n_bins, h_counts, d_ws, ws_bytes, stream);
}
extern "C" int ndmps_valstat_histogram_f64(int L, const int64_t* h_dims, const int64_t* h_bonds,
                                           const double* const* h_cores, const double* h_edges, int n_bins,
                                           int64_t* h_counts, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  return valstat_histogram<double>(L, h_dims, h_bonds, h_cores, h_edges, n_bins, h_counts, d_ws, ws_bytes, stream);
}
extern "C" int ndmps_valstat_error_f32(int L, const int64_t* h_dims, const int64_t* h_bonds, const float* const* h_cores,
                                       const float* d_ref, const int64_t* d_row_off, const int64_t* d_col_off,
                                       const int32_t* d_col_perm, int64_t n_cols, double* h_stats, int64_t* h_counts,
                                       void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  const ErrorTables err{d_ref, d_row_off, d_col_off, d_col_perm, n_cols};
  return valstat_record<float>(L, h_dims, h_bonds, h_cores, &err, -INFINITY, INFINITY, h_stats, h_counts, d_ws, ws_bytes, stream);
}
extern "C" int ndmps_valstat_error_f64(int L, const int64_t* h_dims, const int64_t* h_bonds, const double* const* h_cores,
                                       const double* d_ref, const int64_t* d_row_off, const int64_t* d_col_off,
                                       const int32_t* d_col_perm, int64_t n_cols, double* h_stats, int64_t* h_counts,
                                       void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  const ErrorTables err{d_ref, d_row_off, d_col_off, d_col_perm, n_cols};
  return valstat_record<double>(L, h_dims, h_bonds, h_cores, &err, -INFINITY, INFINITY, h_stats, h_counts, d_ws, ws_bytes, stream);
}
