// Statistics per label of an atlas or segmentation, from the cores: the moments pass of the value statistics
// (RecordEpi, valstat_device.h) and then one more epilogue of the same reducing product per window of labels, so the N
// voxels are never written.
//
//   ndmps_labelstat_*  <- NDMPS.label_stats / label_stats_many   (core/labelstat.py)
#include <vector>

#include "common.h"
#include "labelstat_device.h"
#include "typed.h"
#include "valstat_device.h"
#include "valstat_plan.h"

namespace {

// Which threads meet which label depends on the data, so no fixed tree folds the sums.  They are 64-bit fixed-point
// integers instead: q = llrint(v 2^s) into a signed sum, q2 = llrint(v v 2^s2) into an unsigned one, and integer
// addition gives the same bits in any order.  The scales follow from the extremes of the moments pass over the same
// operands (labelstat_scale_kernel), by the one rule of labelstat_device.h.
constexpr int kLabelWindow = 1024;  // labels of one launch: their LDS table (40 B each in fp64) fits beside the tiles
constexpr int kLabelSlots = 6;      // global table: sum, sum of squares, count, NaN count, min key, max key (n_labels each)
constexpr int kLabelTail = 5;       // then: outside, overflow, s, s2, non-finite flag
enum { kTailOutside = 0, kTailOverflow = 1, kTailS = 2, kTailS2 = 3, kTailFlag = 4 };

// the folded record of the moments pass -> s, s2 and the non-finite flag in the table's tail (one thread)
__global__ void labelstat_scale_kernel(const Record* __restrict__ result, int64_t numel, long long* __restrict__ tail) {
  const Record r = *result;
  double maxabs = 0.0;
  if (r.c2 > 0) maxabs = fmax(fabs(r.lo), fabs(r.hi0));  // no voxel taken (NaN only): lo = +inf, hi0 = -inf
  int s = 0, s2 = 0;
  const bool finite = maxabs <= 1.7976931348623157e308;
  if (finite) labelstat_scale_rule(maxabs, numel, &s, &s2);
  tail[kTailS] = s;
  tail[kTailS2] = s2;
  tail[kTailFlag] = finite ? 0 : 1;
}

struct LabelArgs {
  const void* lab;             // the label volume, C order
  int lab_bytes;               // 1: uint8, 2: int16, 4: int32
  const int64_t* row_off;      // [m]
  const int64_t* col_off;      // [n], in the column order of B as the kernel sees it
  int64_t numel;               // elements of lab
  unsigned long long* table;   // [kLabelSlots * n_labels + kLabelTail], cleared before the first window
  int n_labels;
  int label_base, window;      // this launch takes the labels label_base <= l < label_base + window
  int nb;                      // labelstat_bits(numel)
};

// A thread holds one run (label, counts, sums, keys) in registers while the voxels it takes share a label, and flushes
// it into the workgroup's LDS table when the label changes and at the end; padded elements, labels of another
// window and labels outside [0, n_labels) neither break nor extend a run.  Keys: the largest wins for both extremes
// (ext_key<T, true> for the minimum), key 0 is "nothing", so a cleared table is an empty one.
template <typename T>
struct LabelEpi {
  typedef LabelArgs Args;
  typedef typename KeyOf<T>::type K;
  unsigned long long *sum, *sumsq;  // LDS, [window] each
  K *kmin, *kmax;
  unsigned int *cnt, *nan, *misc;   // misc: outside, overflow
  int s, s2;
  bool dead;                        // non-finite voxels: the host refuses, nothing is accumulated
  double limit;                     // 2^(62 - nb): no |q| of a voxel the moments pass saw comes near it
  int h_label;
  unsigned int h_cnt, h_nan, outside, overflow;
  long long h_sum;
  unsigned long long h_sumsq;
  K h_min, h_max;

  __device__ __forceinline__ void begin(const Args& a) {
    const int W = a.window;
    sum = reinterpret_cast<unsigned long long*>(valstat_dyn_lds);
    sumsq = sum + W;
    kmin = reinterpret_cast<K*>(sumsq + W);
    kmax = kmin + W;
    cnt = reinterpret_cast<unsigned int*>(kmax + W);
    nan = cnt + W;
    misc = nan + W;
    for (int i = threadIdx.x; i < W; i += 256) {
      sum[i] = sumsq[i] = 0ull;
      kmin[i] = kmax[i] = (K)0;
      cnt[i] = nan[i] = 0u;
    }
    if (threadIdx.x < 2) misc[threadIdx.x] = 0u;
    const long long* tail = reinterpret_cast<const long long*>(a.table + (size_t)kLabelSlots * a.n_labels);
    s = (int)tail[kTailS];
    s2 = (int)tail[kTailS2];
    dead = tail[kTailFlag] != 0;
    limit = ldexp(1.0, 62 - a.nb);
    h_label = -1;
    h_cnt = h_nan = outside = overflow = 0u;
    h_sum = 0;
    h_sumsq = 0ull;
    h_min = h_max = (K)0;
    __syncthreads();
  }
  __device__ __forceinline__ void flush() {
    if (h_label < 0) return;
    if (h_nan) atomicAdd(&nan[h_label], h_nan);
    if (h_cnt) {
      atomicAdd(&cnt[h_label], h_cnt);
      atomicAdd(&sum[h_label], (unsigned long long)h_sum);  // two's complement: the signed sum
      atomicAdd(&sumsq[h_label], h_sumsq);
      atomicMax(&kmin[h_label], h_min);
      atomicMax(&kmax[h_label], h_max);
    }
  }
  __device__ __forceinline__ void take(const Args& a, bool valid, int64_t row, int64_t col, T v) {
    if (!valid || dead) return;
    const int64_t at = a.row_off[row] + a.col_off[col];
    if (at < 0 || at >= a.numel) return;  // the tables are not trusted: nothing is read outside lab
    int label = label_read(a.lab, a.lab_bytes, at);
    if (label < 0 || label >= a.n_labels) {
      if (a.label_base == 0) ++outside;
      return;
    }
    label -= a.label_base;
    if (label < 0 || label >= a.window) return;  // another window's launch takes it
    const bool is_nan = v != v;
    long long q = 0;
    unsigned long long q2 = 0ull;
    if (!is_nan) {
      const double d = (double)v, x = ldexp(d, s), x2 = ldexp(d * d, s2);
      if (!(fabs(x) <= limit && x2 <= limit)) {  // not a voxel of the moments pass
        ++overflow;
        return;
      }
      q = llrint(x);
      q2 = (unsigned long long)llrint(x2);
    }
    if (label != h_label) {
      flush();
      h_label = label;
      h_cnt = h_nan = 0u;
      h_sum = 0;
      h_sumsq = 0ull;
      h_min = h_max = (K)0;
    }
    if (is_nan) {
      ++h_nan;
      return;
    }
    ++h_cnt;
    h_sum += q;
    h_sumsq += q2;
    const K lo = ext_key<T, true>(v), hi = ext_key<T, false>(v);
    if (lo > h_min) h_min = lo;
    if (hi > h_max) h_max = hi;
  }
  __device__ __forceinline__ void finish(const Args& a) {
    flush();
    if (outside) atomicAdd(&misc[0], outside);
    if (overflow) atomicAdd(&misc[1], overflow);
    __syncthreads();
    const size_t L = (size_t)a.n_labels;
    for (int i = threadIdx.x; i < a.window; i += 256) {
      const size_t g = (size_t)a.label_base + i;
      if (nan[i]) atomicAdd(&a.table[3 * L + g], (unsigned long long)nan[i]);
      if (!cnt[i]) continue;
      atomicAdd(&a.table[0 * L + g], sum[i]);
      atomicAdd(&a.table[1 * L + g], sumsq[i]);
      atomicAdd(&a.table[2 * L + g], (unsigned long long)cnt[i]);
      atomicMax(&a.table[4 * L + g], (unsigned long long)kmin[i]);
      atomicMax(&a.table[5 * L + g], (unsigned long long)kmax[i]);
    }
    if (threadIdx.x < 2 && misc[threadIdx.x]) atomicAdd(&a.table[kLabelSlots * L + threadIdx.x], (unsigned long long)misc[threadIdx.x]);
  }
};

inline int64_t labelstat_table_bytes(int64_t n_labels) {
  return ndmps::chain_round_up((kLabelSlots * n_labels + kLabelTail) * 8, 256);
}

// Statistics per label.  The products before the last run once; the last runs as the moments pass, whose folded
// record becomes the scales on the device, and then once per window of labels over the same operands (the same
// gathered right operand: a voxel has the same bits in every launch).  One synchronisation, at the final copy.
template <typename T>
int labelstat_run(int L, const int64_t* h_dims, const int64_t* h_bonds, const T* const* h_cores, const void* d_labels,
                  int label_elem_bytes, const int64_t* d_row_off, const int64_t* d_col_off, const int32_t* d_col_perm,
                  int64_t n_cols, int n_labels, int64_t* h_sums, uint64_t* h_sumsq, int64_t* h_counts, double* h_minmax,
                  int64_t* h_info, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  typedef typename KeyOf<T>::type K;
  NDMPS_REQUIRE(L >= 1 && h_dims && h_bonds && h_sums && h_sumsq && h_counts && h_minmax && h_info, "bad labelstat argument");
  NDMPS_REQUIRE(n_labels >= 1 && n_labels <= kLabelMax, "label statistics take 1 to %d labels, got %d", kLabelMax, n_labels);
  NDMPS_REQUIRE(label_elem_bytes == 1 || label_elem_bytes == 2 || label_elem_bytes == 4,
                "labels are uint8, int16 or int32 (1, 2 or 4 bytes), got %d bytes", label_elem_bytes);
  const ChainStatsPlan sp = ndmps::chain_stats_plan(L, h_dims, h_bonds, sizeof(T), 0);
  const ErrorTables tables{d_labels, d_row_off, d_col_off, d_col_perm, n_cols};
  StatCall<T> c(sp, h_cores, d_ws, stream);
  NDMPS_TRY(c.check(h_dims, h_bonds, ws_bytes, &tables));
  const int64_t table_bytes = labelstat_table_bytes(n_labels);
  if (ws_bytes < sp.total_bytes + table_bytes) {
    ndmps::set_error("labelstat workspace too small: %lld < %lld", (long long)ws_bytes, (long long)(sp.total_bytes + table_bytes));
    return NDMPS_EWORKSPACE;
  }
  NDMPS_TRY(stat_counters_fit(stat_tiles(c.q), c.grid, "label statistics"));
  NDMPS_TRY(c.run(d_col_perm));
  hipStream_t s = c.s;
  Record* result = c.template result<Record>();
  unsigned long long* table = (unsigned long long*)(c.ws + sp.total_bytes);
  const int64_t numel = sp.chain.numel;

  const RecordArgs margs{c.template partials<Record>(), nullptr, nullptr, nullptr, numel, -INFINITY, INFINITY};
  NDMPS_TRY((stat_launch<T, RecordEpi<T, false>>(c.q, c.ops, margs, c.grid, 0, s)));
  NDMPS_TRY(stat_fold(margs.partials, c.grid, result, s));
  NDMPS_CHECK_HIP(hipMemsetAsync(table, 0, (size_t)table_bytes, s));
  hipLaunchKernelGGL(labelstat_scale_kernel, dim3(1), dim3(1), 0, s, result, numel,
                     (long long*)(table + (size_t)kLabelSlots * n_labels));
  NDMPS_LAUNCH_CHECK();
  for (int base = 0; base < n_labels; base += kLabelWindow) {
    const int window = std::min(kLabelWindow, n_labels - base);
    const LabelArgs args{d_labels, label_elem_bytes, d_row_off, d_col_off, numel, table, n_labels, base, window,
                         labelstat_bits(numel)};
    const size_t lds = (size_t)window * (16 + 2 * sizeof(K) + 8) + 8;
    NDMPS_TRY((stat_launch<T, LabelEpi<T>>(c.q, c.ops, args, c.grid, lds, s)));
  }
  const size_t words = (size_t)kLabelSlots * n_labels + kLabelTail;
  std::vector<unsigned long long> host(words);
  NDMPS_CHECK_HIP(hipMemcpyAsync(host.data(), table, words * 8, hipMemcpyDeviceToHost, s));
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));
  const unsigned long long* tail = host.data() + (size_t)kLabelSlots * n_labels;
  NDMPS_REQUIRE(tail[kTailFlag] == 0, "label statistics need finite voxels: the volume has an infinite one");
  if (tail[kTailOverflow] != 0) {
    ndmps::set_error("internal: %llu voxels of the labelled pass exceed the range the moments pass found",
                     tail[kTailOverflow]);
    return NDMPS_EHIP;
  }
  const size_t n = (size_t)n_labels;
  for (size_t l = 0; l < n; ++l) {
    h_sums[l] = (int64_t)host[l];
    h_sumsq[l] = host[n + l];
    h_counts[l] = (int64_t)host[2 * n + l];
    h_counts[n + l] = (int64_t)host[3 * n + l];
    h_minmax[l] = (double)ext_value<T>((K)host[4 * n + l], true);
    h_minmax[n + l] = (double)ext_value<T>((K)host[5 * n + l], false);
  }
  h_info[0] = (int64_t)tail[kTailOutside];
  h_info[1] = (int64_t)tail[kTailS];
  h_info[2] = (int64_t)tail[kTailS2];
  h_info[3] = numel;
  return NDMPS_OK;
}

}  // namespace

extern "C" int64_t ndmps_labelstat_workspace_bytes(int L, const int64_t* h_dims, const int64_t* h_bonds, int64_t elem_bytes,
                                                   int64_t n_labels) {
  if (L < 1 || !h_dims || !h_bonds || (elem_bytes != 4 && elem_bytes != 8) || n_labels < 1 || n_labels > kLabelMax) return 0;
  return ndmps::chain_stats_plan(L, h_dims, h_bonds, elem_bytes, 0).total_bytes + labelstat_table_bytes(n_labels);
}
extern "C" int ndmps_labelstat_scales(double maxabs, int64_t numel, int* s, int* s2) {
  NDMPS_REQUIRE(s && s2 && numel >= 1 && maxabs >= 0.0 && maxabs <= 1.7976931348623157e308,
                "labelstat scales: maxabs must be finite and not negative, numel positive");
  labelstat_scale_rule(maxabs, numel, s, s2);
  return NDMPS_OK;
}
extern "C" int ndmps_labelstat_f32(int L, const int64_t* h_dims, const int64_t* h_bonds, const float* const* h_cores,
                                   const void* d_labels, int label_elem_bytes, const int64_t* d_row_off,
                                   const int64_t* d_col_off, const int32_t* d_col_perm, int64_t n_cols, int n_labels,
                                   int64_t* h_sums, uint64_t* h_sumsq, int64_t* h_counts, double* h_minmax, int64_t* h_info,
                                   void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  return labelstat_run<float>(L, h_dims, h_bonds, h_cores, d_labels, label_elem_bytes, d_row_off, d_col_off, d_col_perm,
                              n_cols, n_labels, h_sums, h_sumsq, h_counts, h_minmax, h_info, d_ws, ws_bytes, stream);
}
extern "C" int ndmps_labelstat_f64(int L, const int64_t* h_dims, const int64_t* h_bonds, const double* const* h_cores,
                                   const void* d_labels, int label_elem_bytes, const int64_t* d_row_off,
                                   const int64_t* d_col_off, const int32_t* d_col_perm, int64_t n_cols, int n_labels,
                                   int64_t* h_sums, uint64_t* h_sumsq, int64_t* h_counts, double* h_minmax, int64_t* h_info,
                                   void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  return labelstat_run<double>(L, h_dims, h_bonds, h_cores, d_labels, label_elem_bytes, d_row_off, d_col_off, d_col_perm,
                               n_cols, n_labels, h_sums, h_sumsq, h_counts, h_minmax, h_info, d_ws, ws_bytes, stream);
}
