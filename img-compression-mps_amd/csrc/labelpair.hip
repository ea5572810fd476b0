// Pair statistics per label of an atlas, from the cores: two values per voxel -- the voxel of chain a and either the
// voxel of chain b or the element of an original at the voxel's address -- reduced under the label read at that
// address, with no volume written.
//
//   ndmps_labelpair_*           <- NDMPS.label_pair_stats / label_pair_stats_many   (core/labelpair.py)
//   ndmps_labelpair_original_*  <- NDMPS.label_error_to
//
// One epilogue text, LabelPairEpi, behind two front ends.  Two chains: pairstat_product_kernel (pairstat_device.h), both
// chains run with the plan's column order so that column c of either is the column col_off[c] speaks of.  One chain and
// an original: valstat_product_kernel with OriginalEpi in front, which computes the address once, reads the original
// there and hands (v, y, address) on.  A call is the moments pass over the same operands (PairRecordEpi, the epilogue of
// pair_stats), whose extremes become six power-of-two scales on the device, and then one labelled launch per window of
// 512 labels.  Sums are 64-bit fixed-point integers added with integer atomics, so the same inputs give the same bits
// whichever thread meets which label; a voxel is computed by the one text of stat_tile_accumulate, so where neither
// volume has a NaN the fields of a (and of b) are those of ndmps_labelstat_* on that chain bit for bit.
#include <vector>

#include "common.h"
#include "labelstat_device.h"
#include "pairstat_device.h"
#include "typed.h"
#include "valstat_device.h"

namespace {

constexpr int kPairWindow = 512;  // labels of one launch: 96 B each in fp64, 48 KiB beside the 8.5 KiB of staging tiles
// global table, n_labels words per slot: three signed sums, three unsigned sums, two counts, five keys
enum { kSlotSumA = 0, kSlotSumB, kSlotSumAB, kSlotSqA, kSlotSqB, kSlotSse, kSlotCount, kSlotNan,
       kSlotMinA, kSlotMaxA, kSlotMinB, kSlotMaxB, kSlotMaxDiff, kPairSlots };
static_assert(kPairSlots == 13, "table layout");
// then the tail: outside, overflow, the six exponents, the non-finite flag, and the five extremes of the whole volume
// as the moments pass found them (fp64 bit patterns)
enum { kPtOutside = 0, kPtOverflow = 1, kPtScale = 2, kPtFlag = 8, kPtWhole = 9, kPairTail = 14 };
enum { kSA = 0, kS2A, kSB, kS2B, kSAB, kS2D, kPairScales };  // order of the exponents, here and in h_info[1..6]
static_assert(kPtScale + kPairScales == kPtFlag, "tail layout");

// Six exponents from max |a|, max |b| and max |a - b| over the counted voxels (nb = labelstat_bits(numel)):
//   s_a, s2_a   labelstat_scale_rule(max |a|): every |a| 2^s_a and every fl(a a) 2^s2_a is at most 2^(61 - nb)
//   s_b, s2_b   the same from max |b|
//   s2_d        the second exponent of labelstat_scale_rule(max |a - b|): d = fl(a - b) is what the maximum was taken
//               over, so fl(d d) <= fl(max max) < 2^e2
//   s_ab        61 - nb - e with fl(max |a| max |b|) < 2^e: rounding is monotone, so every |fl(a b)| is below 2^e too;
//               e_a + e_b where that product leaves the fp64 range (|a b| < 2^(e_a + e_b) always)
// numel terms of at most 2^(61 - nb) sum to at most 2^61: no 64-bit sum overflows.
__host__ __device__ inline void labelpair_scale_rule(double max_a, double max_b, double max_d, int64_t numel, int* out) {
  int unused = 0;
  labelstat_scale_rule(max_a, numel, &out[kSA], &out[kS2A]);
  labelstat_scale_rule(max_b, numel, &out[kSB], &out[kS2B]);
  labelstat_scale_rule(max_d, numel, &unused, &out[kS2D]);
  out[kSAB] = 0;
  if (!(max_a > 0.0 && max_b > 0.0)) return;
  int e = 0, ea = 0, eb = 0;
  const double p = max_a * max_b;
  if (p > 0.0 && p <= 1.7976931348623157e308) {
    frexp(p, &e);
  } else {
    frexp(max_a, &ea);
    frexp(max_b, &eb);
    e = ea + eb;
  }
  out[kSAB] = labelstat_clamp(61 - labelstat_bits(numel) - e);
}

// the folded record of the moments pass -> the exponents, the non-finite flag and the whole volume's extremes in the
// table's tail (one thread)
__global__ void labelpair_scale_kernel(const PairSlot* __restrict__ result, int64_t numel, long long* __restrict__ tail) {
  const PairRecord r = *result;
  double max_a = 0.0, max_b = 0.0, max_d = 0.0;
  if (r.count > 0) {  // no voxel counted: the extremes are still +-inf
    max_a = fmax(fabs(r.min_a), fabs(r.max_a));
    max_b = fmax(fabs(r.min_b), fabs(r.max_b));
    max_d = r.max_abs_diff;
  }
  const double top = 1.7976931348623157e308;
  const bool finite = max_a <= top && max_b <= top && max_d <= top;
  int s[kPairScales] = {0, 0, 0, 0, 0, 0};
  if (finite) labelpair_scale_rule(max_a, max_b, max_d, numel, s);
  for (int i = 0; i < kPairScales; ++i) tail[kPtScale + i] = s[i];
  tail[kPtFlag] = finite ? 0 : 1;
  const double whole[5] = {r.min_a, r.max_a, r.min_b, r.max_b, r.max_abs_diff};
  for (int i = 0; i < 5; ++i) tail[kPtWhole + i] = __double_as_longlong(whole[i]);
}

struct LabelPairArgs {
  const void* lab;             // the label volume, C order
  int lab_bytes;               // 1: uint8, 2: int16, 4: int32
  const int64_t* row_off;      // [m]
  const int64_t* col_off;      // [n], in the column order of B as the kernel sees it
  int64_t numel;               // elements of lab
  unsigned long long* table;   // [kPairSlots * n_labels + kPairTail], cleared before the first window
  int n_labels;
  int label_base, window;      // this launch takes the labels label_base <= l < label_base + window
  int nb;                      // labelstat_bits(numel)
};

// LabelEpi (labelstat.hip) for two values: a thread holds one run (label, counts, six sums, five keys) in registers
// while the voxels it takes share a label, and flushes it into the workgroup's LDS table when the label changes and at
// the end; padded elements, labels of another window and labels outside [0, n_labels) neither break nor extend a run.
// Keys: the largest wins for every extreme (ext_key<T, true> for a minimum), key 0 is "nothing".  The key of
// |a - b| is the fp64 one in either element type: the difference of two fp32 voxels is formed in fp64, as
// PairRecordEpi forms it, and is no fp32 number.
template <typename T>
struct LabelPairEpi {
  typedef LabelPairArgs Args;
  typedef typename KeyOf<T>::type K;
  typedef unsigned long long U;
  U* sums;                          // LDS, [6][window]: sum a, sum b, sum a b (signed), sum a^2, sum b^2, sum d^2
  U* kdiff;                         // [window]
  K* keys;                          // [4][window]: min a, max a, min b, max b
  unsigned int *cnt, *nan, *misc;   // misc: outside, overflow
  int W;
  int s[kPairScales];
  bool dead;                        // non-finite voxels: the host refuses, nothing is accumulated
  double limit;                     // 2^(62 - nb): no term of a voxel the moments pass saw comes near it
  int h_label;
  unsigned int h_cnt, h_nan, outside, overflow;
  long long h_a, h_b, h_ab;
  U h_a2, h_b2, h_d2, h_diff;
  K h_min_a, h_max_a, h_min_b, h_max_b;

  static size_t lds_bytes(int window) { return (size_t)window * (7 * 8 + 4 * sizeof(K) + 2 * 4) + 8; }

  __device__ __forceinline__ void clear_run() {
    h_cnt = h_nan = 0u;
    h_a = h_b = h_ab = 0;
    h_a2 = h_b2 = h_d2 = h_diff = 0ull;
    h_min_a = h_max_a = h_min_b = h_max_b = (K)0;
  }
  __device__ __forceinline__ void begin(const Args& a) {
    W = a.window;
    sums = reinterpret_cast<U*>(valstat_dyn_lds);
    kdiff = sums + 6 * W;
    keys = reinterpret_cast<K*>(kdiff + W);
    cnt = reinterpret_cast<unsigned int*>(keys + 4 * W);
    nan = cnt + W;
    misc = nan + W;
    for (int i = threadIdx.x; i < 7 * W; i += 256) sums[i] = 0ull;  // the sums and kdiff behind them
    for (int i = threadIdx.x; i < 4 * W; i += 256) keys[i] = (K)0;
    for (int i = threadIdx.x; i < 2 * W; i += 256) cnt[i] = 0u;     // cnt and nan behind it
    if (threadIdx.x < 2) misc[threadIdx.x] = 0u;
    const long long* tail = reinterpret_cast<const long long*>(a.table + (size_t)kPairSlots * a.n_labels);
    for (int i = 0; i < kPairScales; ++i) s[i] = (int)tail[kPtScale + i];
    dead = tail[kPtFlag] != 0;
    limit = ldexp(1.0, 62 - a.nb);
    h_label = -1;
    outside = overflow = 0u;
    clear_run();
    __syncthreads();
  }
  __device__ __forceinline__ void flush() {
    if (h_label < 0) return;
    if (h_nan) atomicAdd(&nan[h_label], h_nan);
    if (h_cnt) {
      atomicAdd(&cnt[h_label], h_cnt);
      atomicAdd(&sums[0 * W + h_label], (U)h_a);  // two's complement: the signed sums
      atomicAdd(&sums[1 * W + h_label], (U)h_b);
      atomicAdd(&sums[2 * W + h_label], (U)h_ab);
      atomicAdd(&sums[3 * W + h_label], h_a2);
      atomicAdd(&sums[4 * W + h_label], h_b2);
      atomicAdd(&sums[5 * W + h_label], h_d2);
      atomicMax(&kdiff[h_label], h_diff);
      atomicMax(&keys[0 * W + h_label], h_min_a);
      atomicMax(&keys[1 * W + h_label], h_max_a);
      atomicMax(&keys[2 * W + h_label], h_min_b);
      atomicMax(&keys[3 * W + h_label], h_max_b);
    }
  }
  __device__ __forceinline__ void take(const Args& a, bool valid, int64_t row, int64_t col, T va, T vb) {
    if (!valid) return;
    const int64_t at = a.row_off[row] + a.col_off[col];
    if (at < 0 || at >= a.numel) return;  // the tables are not trusted: nothing is read outside lab
    take_at(a, at, va, vb);
  }
  // a valid pair whose address 0 <= at < numel is known
  __device__ __forceinline__ void take_at(const Args& a, int64_t at, T va, T vb) {
    if (dead) return;
    int label = label_read(a.lab, a.lab_bytes, at);
    if (label < 0 || label >= a.n_labels) {
      if (a.label_base == 0) ++outside;
      return;
    }
    label -= a.label_base;
    if (label < 0 || label >= a.window) return;  // another window's launch takes it
    const bool is_nan = va != va || vb != vb;
    long long q_a = 0, q_b = 0, q_ab = 0;
    U q_a2 = 0ull, q_b2 = 0ull, q_d2 = 0ull;
    double d = 0.0;
    if (!is_nan) {
      const double x = (double)va, y = (double)vb;
      d = x - y;
      const double t_a = ldexp(x, s[kSA]), t_b = ldexp(y, s[kSB]), t_ab = ldexp(x * y, s[kSAB]);
      const double t_a2 = ldexp(x * x, s[kS2A]), t_b2 = ldexp(y * y, s[kS2B]), t_d2 = ldexp(d * d, s[kS2D]);
      if (!(fabs(t_a) <= limit && fabs(t_b) <= limit && fabs(t_ab) <= limit && t_a2 <= limit && t_b2 <= limit &&
            t_d2 <= limit)) {  // not a voxel of the moments pass
        ++overflow;
        return;
      }
      q_a = llrint(t_a), q_b = llrint(t_b), q_ab = llrint(t_ab);
      q_a2 = (U)llrint(t_a2), q_b2 = (U)llrint(t_b2), q_d2 = (U)llrint(t_d2);
    }
    if (label != h_label) {
      flush();
      h_label = label;
      clear_run();
    }
    if (is_nan) {
      ++h_nan;
      return;
    }
    ++h_cnt;
    h_a += q_a, h_b += q_b, h_ab += q_ab;
    h_a2 += q_a2, h_b2 += q_b2, h_d2 += q_d2;
    const K lo_a = ext_key<T, true>(va), hi_a = ext_key<T, false>(va);
    const K lo_b = ext_key<T, true>(vb), hi_b = ext_key<T, false>(vb);
    const U diff = ext_key<double, false>(fabs(d));
    if (lo_a > h_min_a) h_min_a = lo_a;
    if (hi_a > h_max_a) h_max_a = hi_a;
    if (lo_b > h_min_b) h_min_b = lo_b;
    if (hi_b > h_max_b) h_max_b = hi_b;
    if (diff > h_diff) h_diff = diff;
  }
  __device__ __forceinline__ void finish(const Args& a) {
    flush();
    if (outside) atomicAdd(&misc[0], outside);
    if (overflow) atomicAdd(&misc[1], overflow);
    __syncthreads();
    const size_t L = (size_t)a.n_labels;
    for (int i = threadIdx.x; i < W; i += 256) {
      const size_t g = (size_t)a.label_base + i;
      if (nan[i]) atomicAdd(&a.table[kSlotNan * L + g], (U)nan[i]);
      if (!cnt[i]) continue;
      atomicAdd(&a.table[kSlotCount * L + g], (U)cnt[i]);
      for (int k = 0; k < 6; ++k) atomicAdd(&a.table[(kSlotSumA + k) * L + g], sums[k * W + i]);
      for (int k = 0; k < 4; ++k) atomicMax(&a.table[(kSlotMinA + k) * L + g], (U)keys[k * W + i]);
      atomicMax(&a.table[kSlotMaxDiff * L + g], kdiff[i]);
    }
    if (threadIdx.x < 2 && misc[threadIdx.x]) atomicAdd(&a.table[kPairSlots * L + threadIdx.x], (U)misc[threadIdx.x]);
  }
};

// In front of a pair epilogue Inner on valstat_product_kernel: the second value of a voxel is the element of an
// original at the voxel's C-order address (RecordEpi<T, true>'s read and range check).  The address is computed once
// and handed on, so a labelled Inner reads its label where the original was read.
template <typename InnerArgs>
struct OriginalArgs {
  InnerArgs inner;
  const void* ref;         // the original, C order, in the element type
  const int64_t* row_off;  // [m]
  const int64_t* col_off;  // [n], in the column order of B as the kernel sees it
  int64_t numel;           // elements of ref
};

template <typename T, typename Inner>
struct OriginalEpi {
  typedef OriginalArgs<typename Inner::Args> Args;
  Inner inner;
  __device__ __forceinline__ void begin(const Args& a) { inner.begin(a.inner); }
  __device__ __forceinline__ void take(const Args& a, bool valid, int64_t row, int64_t col, T v) {
    if (!valid) return;
    const int64_t at = a.row_off[row] + a.col_off[col];
    if (at < 0 || at >= a.numel) return;  // the tables are not trusted: nothing is read outside ref
    inner.take_at(a.inner, at, v, static_cast<const T*>(a.ref)[at]);
  }
  __device__ __forceinline__ void finish(const Args& a) { inner.finish(a.inner); }
};

inline int64_t labelpair_table_bytes(int64_t n_labels) {
  return ndmps::chain_round_up((kPairSlots * n_labels + kPairTail) * 8, 256);
}

// the moments pass of the original front end keeps its partial pair records in the single plan's record slots
constexpr int kOriginalMomentGroups = (int)(ndmps::kValstatMaxGroups * ndmps::kValstatRecordBytes / sizeof(PairSlot));
static_assert(kOriginalMomentGroups >= 1 && sizeof(PairSlot) <= 256, "the single plan's record slots hold pair records");

struct LabelPairOut {
  int64_t* sums;    // [3][n_labels]: sum a, sum b, sum a b
  uint64_t* sumsq;  // [3][n_labels]: sum a^2, sum b^2, sum (a - b)^2
  int64_t* counts;  // [2][n_labels]: count, n_nan
  double* ext;      // [5][n_labels]: min a, max a, min b, max b, max |a - b|
  int64_t* info;    // [NDMPS_LABELPAIR_INFO_SLOTS]: outside, the six exponents, numel
  double* whole;    // [5]: the five extremes over all counted voxels, labelled or not
  bool ok() const { return sums && sumsq && counts && ext && info && whole; }
};

template <typename T>
int labelpair_args_ok(int n_labels, int label_elem_bytes, const LabelPairOut& out) {
  NDMPS_REQUIRE(out.ok(), "bad labelpair argument");
  NDMPS_REQUIRE(n_labels >= 1 && n_labels <= kLabelMax, "label statistics take 1 to %d labels, got %d", kLabelMax, n_labels);
  NDMPS_REQUIRE(label_elem_bytes == 1 || label_elem_bytes == 2 || label_elem_bytes == 4,
                "labels are uint8, int16 or int32 (1, 2 or 4 bytes), got %d bytes", label_elem_bytes);
  constexpr size_t kStatic = sizeof(typename StatTile<T>::StageA) + sizeof(typename StatTile<T>::StageB);
  NDMPS_REQUIRE(LabelPairEpi<T>::lds_bytes(kPairWindow) + kStatic <= 65536, "internal: the label window does not fit in 64 KiB of LDS");
  return NDMPS_OK;
}

// After the products before the last: the moments pass (moments(): its launch into `partials`), fold, memset of the
// table, the scale kernel, one labelled launch per window (labelled(args, lds)), one copy, one synchronisation.
template <typename T, typename Moments, typename Labelled>
int labelpair_passes(const LabelPairArgs& base, PairSlot* partials, int moment_groups, PairSlot* result, hipStream_t s,
                     const LabelPairOut& out, Moments&& moments, Labelled&& labelled) {
  typedef typename KeyOf<T>::type K;
  const int n_labels = base.n_labels;
  unsigned long long* table = base.table;
  NDMPS_TRY(moments());
  NDMPS_TRY((stat_fold<PairRecord>(partials, moment_groups, static_cast<PairRecord*>(result), s)));
  NDMPS_CHECK_HIP(hipMemsetAsync(table, 0, (size_t)labelpair_table_bytes(n_labels), s));
  hipLaunchKernelGGL(labelpair_scale_kernel, dim3(1), dim3(1), 0, s, result, base.numel,
                     (long long*)(table + (size_t)kPairSlots * n_labels));
  NDMPS_LAUNCH_CHECK();
  for (int at = 0; at < n_labels; at += kPairWindow) {
    LabelPairArgs args = base;
    args.label_base = at;
    args.window = std::min(kPairWindow, n_labels - at);
    NDMPS_TRY(labelled(args, LabelPairEpi<T>::lds_bytes(args.window)));
  }
  const size_t n = (size_t)n_labels, words = kPairSlots * n + kPairTail;
  std::vector<unsigned long long> host(words);
  NDMPS_CHECK_HIP(hipMemcpyAsync(host.data(), table, words * 8, hipMemcpyDeviceToHost, s));
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));
  const unsigned long long* tail = host.data() + kPairSlots * n;
  NDMPS_REQUIRE(tail[kPtFlag] == 0, "label pair statistics need finite voxels: one of the two volumes has an infinite one");
  if (tail[kPtOverflow] != 0) {
    ndmps::set_error("internal: %llu voxels of the labelled pass exceed the range the moments pass found", tail[kPtOverflow]);
    return NDMPS_EHIP;
  }
  for (size_t l = 0; l < n; ++l) {
    for (int k = 0; k < 3; ++k) {
      out.sums[k * n + l] = (int64_t)host[(kSlotSumA + k) * n + l];
      out.sumsq[k * n + l] = host[(kSlotSqA + k) * n + l];
    }
    out.counts[l] = (int64_t)host[kSlotCount * n + l];
    out.counts[n + l] = (int64_t)host[kSlotNan * n + l];
    for (int k = 0; k < 4; ++k) out.ext[k * n + l] = (double)ext_value<T>((K)host[(kSlotMinA + k) * n + l], k % 2 == 0);
    out.ext[4 * n + l] = ext_value<double>(host[kSlotMaxDiff * n + l], false);
  }
  out.info[0] = (int64_t)tail[kPtOutside];
  for (int i = 0; i < kPairScales; ++i) out.info[1 + i] = (int64_t)tail[kPtScale + i];
  out.info[1 + kPairScales] = base.numel;
  for (int i = 0; i < 5; ++i) __builtin_memcpy(&out.whole[i], &tail[kPtWhole + i], 8);
  return NDMPS_OK;
}

// two chains
template <typename T>
int labelpair_run(int L, const int64_t* h_dims, const int64_t* h_bonds_a, const int64_t* h_bonds_b, const T* const* h_cores_a,
                  const T* const* h_cores_b, const void* d_labels, int label_elem_bytes, const int64_t* d_row_off,
                  const int64_t* d_col_off, const int32_t* d_col_perm, int64_t n_cols, int n_labels, const LabelPairOut& out,
                  void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  NDMPS_REQUIRE(L >= 1 && h_dims && h_bonds_a && h_bonds_b, "bad labelpair argument");
  NDMPS_TRY(labelpair_args_ok<T>(n_labels, label_elem_bytes, out));
  const ChainPairPlan pp = ndmps::chain_pair_plan(L, h_dims, h_bonds_a, h_bonds_b, sizeof(T));
  const ErrorTables tables{d_labels, d_row_off, d_col_off, d_col_perm, n_cols};
  StatCall<T> a(pp.a, h_cores_a, d_ws, stream), b(pp.b, h_cores_b, (char*)d_ws + pp.off_b, stream);
  NDMPS_TRY(pairstat_check(pp, a, b, h_dims, h_bonds_a, h_bonds_b, ws_bytes, &tables));
  const int64_t need = pp.total_bytes + labelpair_table_bytes(n_labels);
  if (ws_bytes < need) {
    ndmps::set_error("labelpair workspace too small: %lld < %lld", (long long)ws_bytes, (long long)need);
    return NDMPS_EWORKSPACE;
  }
  NDMPS_TRY(stat_counters_fit(stat_tiles(a.q), a.grid, "label pair statistics"));
  NDMPS_TRY(a.run(d_col_perm));
  NDMPS_TRY(b.run(d_col_perm));
  PairSlot* partials = (PairSlot*)(a.ws + pp.off_partials);
  PairSlot* result = (PairSlot*)(a.ws + pp.off_result);
  const int64_t numel = pp.a.chain.numel;
  const LabelPairArgs base{d_labels, label_elem_bytes, d_row_off, d_col_off, numel, (unsigned long long*)(a.ws + pp.total_bytes),
                           n_labels, 0, 0, labelstat_bits(numel)};
  return labelpair_passes<T>(
      base, partials, a.grid, result, a.s, out,
      [&] { return pairstat_launch<T, PairRecordEpi<T>>(a, b, PairRecordArgs{partials}, a.grid, 0); },
      [&](const LabelPairArgs& args, size_t lds) { return pairstat_launch<T, LabelPairEpi<T>>(a, b, args, a.grid, lds); });
}

// one chain and an original
template <typename T>
int labelpair_original_run(int L, const int64_t* h_dims, const int64_t* h_bonds, const T* const* h_cores, const T* d_ref,
                           const void* d_labels, int label_elem_bytes, const int64_t* d_row_off, const int64_t* d_col_off,
                           const int32_t* d_col_perm, int64_t n_cols, int n_labels, const LabelPairOut& out, void* d_ws,
                           int64_t ws_bytes, ndmps_stream_t stream) {
  NDMPS_REQUIRE(L >= 1 && h_dims && h_bonds && d_labels, "bad labelpair argument");
  NDMPS_TRY(labelpair_args_ok<T>(n_labels, label_elem_bytes, out));
  const ChainStatsPlan sp = ndmps::chain_stats_plan(L, h_dims, h_bonds, sizeof(T), 0);
  const ErrorTables tables{d_ref, d_row_off, d_col_off, d_col_perm, n_cols};
  StatCall<T> c(sp, h_cores, d_ws, stream);
  NDMPS_TRY(c.check(h_dims, h_bonds, ws_bytes, &tables));
  const int64_t need = sp.total_bytes + labelpair_table_bytes(n_labels);
  if (ws_bytes < need) {
    ndmps::set_error("labelpair workspace too small: %lld < %lld", (long long)ws_bytes, (long long)need);
    return NDMPS_EWORKSPACE;
  }
  NDMPS_TRY(stat_counters_fit(stat_tiles(c.q), c.grid, "label pair statistics"));
  NDMPS_TRY(c.run(d_col_perm));
  PairSlot* partials = c.template partials<PairSlot>();
  PairSlot* result = c.template result<PairSlot>();
  const int moment_groups = std::min(c.grid, kOriginalMomentGroups);  // the extremes do not depend on the grid
  const int64_t numel = sp.chain.numel;
  const LabelPairArgs base{d_labels, label_elem_bytes, d_row_off, d_col_off, numel, (unsigned long long*)(c.ws + sp.total_bytes),
                           n_labels, 0, 0, labelstat_bits(numel)};
  typedef OriginalEpi<T, PairRecordEpi<T>> MomentsEpi;
  typedef OriginalEpi<T, LabelPairEpi<T>> LabelledEpi;
  return labelpair_passes<T>(
      base, partials, moment_groups, result, c.s, out,
      [&] {
        const typename MomentsEpi::Args args{PairRecordArgs{partials}, d_ref, d_row_off, d_col_off, numel};
        return stat_launch<T, MomentsEpi>(c.q, c.ops, args, moment_groups, 0, c.s);
      },
      [&](const LabelPairArgs& largs, size_t lds) {
        const typename LabelledEpi::Args args{largs, d_ref, d_row_off, d_col_off, numel};
        return stat_launch<T, LabelledEpi>(c.q, c.ops, args, c.grid, lds, c.s);
      });
}

}  // namespace

// h_bonds_b == NULL: the call on one chain and an original
extern "C" int64_t ndmps_labelpair_workspace_bytes(int L, const int64_t* h_dims, const int64_t* h_bonds_a,
                                                   const int64_t* h_bonds_b, int64_t elem_bytes, int64_t n_labels) {
  if (L < 1 || !h_dims || !h_bonds_a || (elem_bytes != 4 && elem_bytes != 8) || n_labels < 1 || n_labels > kLabelMax) return 0;
  if (!h_bonds_b) return ndmps::chain_stats_plan(L, h_dims, h_bonds_a, elem_bytes, 0).total_bytes + labelpair_table_bytes(n_labels);
  const ChainPairPlan pp = ndmps::chain_pair_plan(L, h_dims, h_bonds_a, h_bonds_b, elem_bytes);
  return pp.error ? 0 : pp.total_bytes + labelpair_table_bytes(n_labels);
}
extern "C" int ndmps_labelpair_scales(double maxabs_a, double maxabs_b, double max_abs_diff, int64_t numel, int* h_scales) {
  const double top = 1.7976931348623157e308;
  NDMPS_REQUIRE(h_scales && numel >= 1 && maxabs_a >= 0.0 && maxabs_a <= top && maxabs_b >= 0.0 && maxabs_b <= top &&
                    max_abs_diff >= 0.0 && max_abs_diff <= top,
                "labelpair scales: the three magnitudes must be finite and not negative, numel positive");
  labelpair_scale_rule(maxabs_a, maxabs_b, max_abs_diff, numel, h_scales);
  return NDMPS_OK;
}

#define NDMPS_LABELPAIR_ENTRIES(SUFFIX, T)                                                                                      \
  extern "C" int ndmps_labelpair_##SUFFIX(int L, const int64_t* h_dims, const int64_t* h_bonds_a, const int64_t* h_bonds_b,    \
                                          const T* const* h_cores_a, const T* const* h_cores_b, const void* d_labels,          \
                                          int label_elem_bytes, const int64_t* d_row_off, const int64_t* d_col_off,            \
                                          const int32_t* d_col_perm, int64_t n_cols, int n_labels, int64_t* h_sums,            \
                                          uint64_t* h_sumsq, int64_t* h_counts, double* h_ext, int64_t* h_info,                \
                                          double* h_whole, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {              \
    return labelpair_run<T>(L, h_dims, h_bonds_a, h_bonds_b, h_cores_a, h_cores_b, d_labels, label_elem_bytes, d_row_off,      \
                            d_col_off, d_col_perm, n_cols, n_labels,                                                           \
                            LabelPairOut{h_sums, h_sumsq, h_counts, h_ext, h_info, h_whole}, d_ws, ws_bytes, stream);          \
  }                                                                                                                             \
  extern "C" int ndmps_labelpair_original_##SUFFIX(int L, const int64_t* h_dims, const int64_t* h_bonds,                        \
                                                   const T* const* h_cores, const T* d_ref, const void* d_labels,              \
                                                   int label_elem_bytes, const int64_t* d_row_off, const int64_t* d_col_off,   \
                                                   const int32_t* d_col_perm, int64_t n_cols, int n_labels, int64_t* h_sums,   \
                                                   uint64_t* h_sumsq, int64_t* h_counts, double* h_ext, int64_t* h_info,       \
                                                   double* h_whole, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {     \
    return labelpair_original_run<T>(L, h_dims, h_bonds, h_cores, d_ref, d_labels, label_elem_bytes, d_row_off, d_col_off,     \
                                     d_col_perm, n_cols, n_labels,                                                             \
                                     LabelPairOut{h_sums, h_sumsq, h_counts, h_ext, h_info, h_whole}, d_ws, ws_bytes, stream); \
  }
NDMPS_LABELPAIR_ENTRIES(f32, float)
NDMPS_LABELPAIR_ENTRIES(f64, double)
#undef NDMPS_LABELPAIR_ENTRIES
