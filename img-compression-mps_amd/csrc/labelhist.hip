// Histograms per label of an atlas or segmentation, from the cores: the labelled reading of labelstat.hip and the exact
// bin search of the histogram (valstat_device.h) in one more epilogue of the same reducing product, run once per window
// of labels, so the N voxels are never written.  Quantiles and medians per label are repeated calls with one edge row
// per label (core/labelhist.py).
//
//   ndmps_labelhist_*  <- NDMPS.label_histogram / label_histogram_many / label_quantile / label_median and the
//                         mask= keyword of histogram / quantile / median   (core/labelhist.py)
#include <vector>

#include "common.h"
#include "labelstat_device.h"
#include "typed.h"
#include "valstat_device.h"
#include "valstat_plan.h"

namespace {

constexpr int kLabelHistMaxLabels = 4096;
constexpr int kLabelHistMaxLaunches = 64;       // a refusal, not a tuned figure: nobody measured where the passes stop paying
constexpr int64_t kLabelHistMaxLds = 64 * 1024;  // dynamic LDS of one launch: two workgroups and their tiles fit in a CU

// The launches of a call.  A window of w labels holds in LDS the edge rows (one shared, or w), two keys per label in
// the element's width and bins + 3 32-bit counters per label (the bins, below, above, NaN).
struct LabelHistPlan {
  int window = 0, launches = 0;
  int64_t lds_bytes = 0;    // of the widest launch
  int64_t table_bytes = 0;  // the global table, rounded up to 256
  int64_t edge_bytes = 0;   // the edge rows on the device, rounded up to 256
};
inline int64_t labelhist_lds(int64_t elem_bytes, int64_t w, int64_t bins, bool per_label) {
  return elem_bytes * ((per_label ? w : 1) * (bins + 1) + 2 * w) + 4 * w * (bins + 3);
}
inline int64_t labelhist_words(int64_t n_labels, int64_t bins) { return n_labels * (bins + 3) + 2 * n_labels + 1; }
inline LabelHistPlan labelhist_plan(int64_t elem_bytes, int64_t n_labels, int64_t bins, bool per_label) {
  LabelHistPlan p;
  const int64_t fixed = per_label ? 0 : elem_bytes * (bins + 1);
  const int64_t each = labelhist_lds(elem_bytes, 1, bins, per_label) - fixed;
  p.window = (int)std::min<int64_t>(n_labels, (kLabelHistMaxLds - fixed) / each);  // at least 1 for bins <= 4096
  p.launches = (int)ceil_div(n_labels, (int64_t)p.window);
  p.lds_bytes = labelhist_lds(elem_bytes, p.window, bins, per_label);
  p.table_bytes = ndmps::chain_round_up(labelhist_words(n_labels, bins) * 8, 256);
  p.edge_bytes = ndmps::chain_round_up((per_label ? n_labels : 1) * (bins + 1) * elem_bytes, 256);
  return p;
}
// the checks of the label count, the bin count and the launch limit, shared by every entry
inline int labelhist_plan_checked(int64_t elem_bytes, int64_t n_labels, int64_t bins, bool per_label, LabelHistPlan* out) {
  NDMPS_REQUIRE(n_labels >= 1 && n_labels <= kLabelHistMaxLabels, "label histogram: 1 to %d labels, got %lld", kLabelHistMaxLabels,
                (long long)n_labels);
  NDMPS_REQUIRE(bins >= 1 && bins <= ndmps::kValstatMaxBins, "label histogram: %lld bins outside [1, %d]", (long long)bins,
                ndmps::kValstatMaxBins);
  *out = labelhist_plan(elem_bytes, n_labels, bins, per_label);
  NDMPS_REQUIRE(out->launches <= kLabelHistMaxLaunches,
                "label histogram: %lld labels x %lld bins need %d launches (windows of %d labels), more than %d: use fewer bins "
                "or split the atlas",
                (long long)n_labels, (long long)bins, out->launches, out->window, kLabelHistMaxLaunches);
  return NDMPS_OK;
}

struct LabelHistArgs {
  const void* lab;             // the label volume, C order
  int lab_bytes;               // 1: uint8, 2: int16, 4: int32
  const int64_t* row_off;      // [m]
  const int64_t* col_off;      // [n], in the column order of B as the kernel sees it
  int64_t numel;               // elements of lab
  const void* edges;           // device, [rows x (bins + 1)] in the element type; rows: 1, or n_labels
  int edge_stride;             // 0: one row for every label; bins + 1: one row per label
  unsigned long long* table;   // [n_labels x (bins + 3)] counts, [n_labels] min keys, [n_labels] max keys, outside
  int n_labels, bins;
  int label_base, window;      // this launch takes the labels label_base <= l < label_base + window
};

// valstat_dyn_lds: the edge rows, the min keys and the max keys of the window, then the 32-bit counters, label-major.
// A voxel's cell is label * (bins + 3) + valstat_bin against its label's row; the lanes that share the first lane's
// cell make one add.  The extremes of the voxels inside [e[0], e[bins]] are held per thread while the label stays the
// same, as LabelEpi holds its run.  Keys: the largest wins for both extremes, key 0 is "nothing".
template <typename T>
struct LabelHistEpi {
  typedef LabelHistArgs Args;
  typedef typename KeyOf<T>::type K;
  T* e;
  K *kmin, *kmax;
  unsigned int* cnt;
  int h_label;
  K h_min, h_max;
  unsigned int outside;

  __device__ __forceinline__ void begin(const Args& a) {
    const int W = a.window, B = a.bins;
    const int n_edges = (a.edge_stride ? W : 1) * (B + 1);
    e = reinterpret_cast<T*>(valstat_dyn_lds);
    kmin = reinterpret_cast<K*>(e + n_edges);
    kmax = kmin + W;
    cnt = reinterpret_cast<unsigned int*>(kmax + W);
    const T* src = static_cast<const T*>(a.edges) + (size_t)a.label_base * a.edge_stride;
    for (int i = threadIdx.x; i < n_edges; i += 256) e[i] = src[i];
    for (int i = threadIdx.x; i < W; i += 256) kmin[i] = kmax[i] = (K)0;
    for (int i = threadIdx.x; i < W * (B + 3); i += 256) cnt[i] = 0u;
    h_label = -1;
    h_min = h_max = (K)0;
    outside = 0u;
    __syncthreads();
  }
  __device__ __forceinline__ void flush() {
    if (h_label < 0 || !h_min) return;
    atomicMax(&kmin[h_label], h_min);
    atomicMax(&kmax[h_label], h_max);
  }
  __device__ __forceinline__ void take(const Args& a, bool valid, int64_t row, int64_t col, T v) {
    int cell = -1;
    if (valid) {
      const int64_t at = a.row_off[row] + a.col_off[col];
      if (at >= 0 && at < a.numel) {  // the tables are not trusted: nothing is read outside lab
        int label = label_read(a.lab, a.lab_bytes, at);
        if (label < 0 || label >= a.n_labels) {
          if (a.label_base == 0) ++outside;
        } else {
          label -= a.label_base;
          if (label >= 0 && label < a.window) {  // otherwise another window's launch takes it
            const int bin = valstat_bin(e + (size_t)label * a.edge_stride, a.bins, v);
            cell = label * (a.bins + 3) + bin;
            if (bin < a.bins) {
              if (label != h_label) {
                flush();
                h_label = label;
                h_min = h_max = (K)0;
              }
              const K lo = ext_key<T, true>(v), hi = ext_key<T, false>(v);
              if (lo > h_min) h_min = lo;
              if (hi > h_max) h_max = hi;
            }
          }
        }
      }
    }
    valstat_add_folded(cnt, cell);
  }
  __device__ __forceinline__ void finish(const Args& a) {
    flush();
    __syncthreads();
    const size_t L = (size_t)a.n_labels, stride = (size_t)a.bins + 3;
    unsigned long long* counts = a.table + (size_t)a.label_base * stride;  // the window's cells are consecutive
    for (int i = threadIdx.x; i < a.window * (a.bins + 3); i += 256)
      if (cnt[i]) atomicAdd(&counts[i], (unsigned long long)cnt[i]);
    for (int i = threadIdx.x; i < a.window; i += 256) {
      if (!kmin[i]) continue;
      const size_t g = (size_t)a.label_base + i;
      atomicMax(&a.table[L * stride + g], (unsigned long long)kmin[i]);
      atomicMax(&a.table[L * stride + L + g], (unsigned long long)kmax[i]);
    }
    if (a.label_base == 0) {  // lane 0 <- the wavefront's count
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) outside += __shfl_down(outside, off);
      if ((threadIdx.x & 63) == 0 && outside) atomicAdd(&a.table[L * stride + 2 * L], (unsigned long long)outside);
    }
  }
};

// Histograms per label.  The products before the last run once; the last runs once per window of labels over the same
// operands (the same gathered right operand: a voxel has the same bits in every launch).  One synchronisation, at the
// final copy.
template <typename T>
int labelhist_run(int L, const int64_t* h_dims, const int64_t* h_bonds, const T* const* h_cores, const void* d_labels,
                  int label_elem_bytes, const int64_t* d_row_off, const int64_t* d_col_off, const int32_t* d_col_perm,
                  int64_t n_cols, int n_labels, const T* h_edges, int n_bins, int per_label, int64_t* h_counts,
                  double* h_minmax, int64_t* h_info, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  typedef typename KeyOf<T>::type K;
  NDMPS_REQUIRE(L >= 1 && h_dims && h_bonds && h_edges && h_counts && h_minmax && h_info, "bad labelhist argument");
  NDMPS_REQUIRE(label_elem_bytes == 1 || label_elem_bytes == 2 || label_elem_bytes == 4,
                "labels are uint8, int16 or int32 (1, 2 or 4 bytes), got %d bytes", label_elem_bytes);
  LabelHistPlan hp;
  NDMPS_TRY(labelhist_plan_checked(sizeof(T), n_labels, n_bins, per_label != 0, &hp));
  const int rows = per_label ? n_labels : 1;
  for (int r = 0; r < rows; ++r)  // rows need not be strictly ascending: a short row is padded with its last edge
    NDMPS_TRY(stat_edges_ok(h_edges + (size_t)r * (n_bins + 1), n_bins, "label histogram: edges"));
  const ChainStatsPlan sp = ndmps::chain_stats_plan(L, h_dims, h_bonds, sizeof(T), 0);
  const ErrorTables tables{d_labels, d_row_off, d_col_off, d_col_perm, n_cols};
  StatCall<T> c(sp, h_cores, d_ws, stream);
  NDMPS_TRY(c.check(h_dims, h_bonds, ws_bytes, &tables));
  const int64_t need = sp.total_bytes + hp.table_bytes + hp.edge_bytes;
  if (ws_bytes < need) {
    ndmps::set_error("labelhist workspace too small: %lld < %lld", (long long)ws_bytes, (long long)need);
    return NDMPS_EWORKSPACE;
  }
  NDMPS_TRY(stat_counters_fit(stat_tiles(c.q), c.grid, "label histogram"));
  NDMPS_TRY(c.run(d_col_perm));
  hipStream_t s = c.s;
  unsigned long long* table = (unsigned long long*)(c.ws + sp.total_bytes);
  T* edges = (T*)(c.ws + sp.total_bytes + hp.table_bytes);
  NDMPS_CHECK_HIP(hipMemsetAsync(table, 0, (size_t)hp.table_bytes, s));
  NDMPS_CHECK_HIP(hipMemcpyAsync(edges, h_edges, (size_t)rows * (n_bins + 1) * sizeof(T), hipMemcpyHostToDevice, s));
  for (int base = 0; base < n_labels; base += hp.window) {
    const int window = std::min(hp.window, n_labels - base);
    const LabelHistArgs args{d_labels, label_elem_bytes, d_row_off, d_col_off, sp.chain.numel, edges,
                             per_label ? n_bins + 1 : 0, table, n_labels, n_bins, base, window};
    const size_t lds = (size_t)labelhist_lds(sizeof(T), window, n_bins, per_label != 0);
    NDMPS_TRY((stat_launch<T, LabelHistEpi<T>>(c.q, c.ops, args, c.grid, lds, s)));
  }
  const size_t n = (size_t)n_labels, cells = n * ((size_t)n_bins + 3), words = (size_t)labelhist_words(n_labels, n_bins);
  std::vector<unsigned long long> host(words);
  NDMPS_CHECK_HIP(hipMemcpyAsync(host.data(), table, words * 8, hipMemcpyDeviceToHost, s));
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));
  for (size_t i = 0; i < cells; ++i) h_counts[i] = (int64_t)host[i];
  for (size_t l = 0; l < n; ++l) {
    h_minmax[l] = (double)ext_value<T>((K)host[cells + l], true);
    h_minmax[n + l] = (double)ext_value<T>((K)host[cells + n + l], false);
  }
  h_info[0] = (int64_t)host[cells + 2 * n];
  h_info[1] = sp.chain.numel;
  return NDMPS_OK;
}

}  // namespace

extern "C" int64_t ndmps_labelhist_workspace_bytes(int L, const int64_t* h_dims, const int64_t* h_bonds, int64_t elem_bytes,
                                                   int64_t n_labels, int64_t n_bins, int per_label) {
  if (L < 1 || !h_dims || !h_bonds || (elem_bytes != 4 && elem_bytes != 8) || n_labels < 1 || n_labels > kLabelHistMaxLabels ||
      n_bins < 1 || n_bins > ndmps::kValstatMaxBins)
    return 0;
  const LabelHistPlan hp = labelhist_plan(elem_bytes, n_labels, n_bins, per_label != 0);
  if (hp.launches > kLabelHistMaxLaunches) return 0;
  return ndmps::chain_stats_plan(L, h_dims, h_bonds, elem_bytes, 0).total_bytes + hp.table_bytes + hp.edge_bytes;
}

// The launches of a call, for tests and tools (slot order: include/ndmps_hip.h).  Host arithmetic only.
extern "C" int ndmps_labelhist_plan_query(int64_t elem_bytes, int64_t n_labels, int64_t n_bins, int per_label, int64_t* h_out) {
  NDMPS_REQUIRE(h_out && (elem_bytes == 4 || elem_bytes == 8), "bad labelhist plan query (elem_bytes=%lld)", (long long)elem_bytes);
  LabelHistPlan hp;
  NDMPS_TRY(labelhist_plan_checked(elem_bytes, n_labels, n_bins, per_label != 0, &hp));
  h_out[0] = hp.window;
  h_out[1] = hp.launches;
  h_out[2] = hp.lds_bytes;
  h_out[3] = hp.table_bytes;
  return NDMPS_OK;
}

extern "C" int ndmps_labelhist_f32(int L, const int64_t* h_dims, const int64_t* h_bonds, const float* const* h_cores,
                                   const void* d_labels, int label_elem_bytes, const int64_t* d_row_off,
                                   const int64_t* d_col_off, const int32_t* d_col_perm, int64_t n_cols, int n_labels,
                                   const float* h_edges, int n_bins, int per_label, int64_t* h_counts, double* h_minmax,
                                   int64_t* h_info, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  return labelhist_run<float>(L, h_dims, h_bonds, h_cores, d_labels, label_elem_bytes, d_row_off, d_col_off, d_col_perm,
                              n_cols, n_labels, h_edges, n_bins, per_label, h_counts, h_minmax, h_info, d_ws, ws_bytes, stream);
}
extern "C" int ndmps_labelhist_f64(int L, const int64_t* h_dims, const int64_t* h_bonds, const double* const* h_cores,
                                   const void* d_labels, int label_elem_bytes, const int64_t* d_row_off,
                                   const int64_t* d_col_off, const int32_t* d_col_perm, int64_t n_cols, int n_labels,
                                   const double* h_edges, int n_bins, int per_label, int64_t* h_counts, double* h_minmax,
                                   int64_t* h_info, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  return labelhist_run<double>(L, h_dims, h_bonds, h_cores, d_labels, label_elem_bytes, d_row_off, d_col_off, d_col_perm,
                               n_cols, n_labels, h_edges, n_bins, per_label, h_counts, h_minmax, h_info, d_ws, ws_bytes, stream);
}
