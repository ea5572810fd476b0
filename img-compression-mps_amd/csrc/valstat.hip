// Value statistics and the error against an original, from the cores: the chain contraction whose last product is
// reduced in registers and LDS instead of stored, so the N voxels are never written.
//
//   ndmps_valstat_moments_*    <- NDMPS.value_stats / min / max      (core/valstat.py)
//   ndmps_valstat_histogram_*  <- NDMPS.histogram / quantile
//   ndmps_valstat_error_*      <- NDMPS.error_to / psnr_to
//   ndmps_axisext_*            <- NDMPS.amax / amin / argmax / argmin along axes   (core/axisext.py)
//   ndmps_argext_*             <- NDMPS.argmax / argmin of the whole volume
//   ndmps_labelstat_*          <- NDMPS.label_stats / label_stats_many             (core/labelstat.py)
//
// chain_stats_plan (valstat_plan.h) is chain_plan with the last product's destination removed and the output's
// role as second cumulative buffer taken by ws_left2.  Every product before the last runs through ndmps_sgemm /
// ndmps_dgemm exactly as run_chain issues them (chain.hip); the last one is valstat_product_kernel, a tiled MFMA
// product (v_mfma_f32_32x32x2_f32 / v_mfma_f64_16x16x4_f64, lane maps as in gemm.hip) on a persistent grid whose
// accumulator tiles are handed, element by element, to an epilogue: the three below, the two of the extremes and the
// one of the label statistics (AxisEpi, ArgEpi, LabelEpi: described where they stand):
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
// workgroup folds its threads by a fixed shuffle tree and writes one partial record, and valstat_fold_kernel folds
// the records in index order: the same inputs give the same bits.  The histogram adds integers, the extremes
// along axes take integer maxima of order-preserving keys, and the label statistics do both on fixed-point sums:
// all associative and commutative.
#include <math.h>

#include <type_traits>
#include <vector>

#include "common.h"
#include "typed.h"
#include "valstat_device.h"  // what pairstat.hip shares: the chain's check and products, the tile, the bin search
#include "valstat_plan.h"

using ndmps::ChainKind;

namespace {

// a partial or the result of the two record epilogues (ndmps::kValstatRecordBytes)
struct Record {
  double s0, s1;     // moments: sum v, sum v^2            error: sum (v - y)^2, sum y^2
  double lo;         // moments: min                       error: unused
  double hi0, hi1;   // moments: max, unused               error: max |v - y|, max y
  long long c0, c1;  // voxels, NaN among them (moments: v; error: v - y)
  long long c2;      // moments: voxels inside the clip range (the ones behind the four statistics)
};
static_assert(sizeof(Record) == ndmps::kValstatRecordBytes, "record layout");

__device__ __forceinline__ void record_clear(Record& r) {
  r.s0 = r.s1 = 0.0;
  r.lo = INFINITY;
  r.hi0 = r.hi1 = -INFINITY;
  r.c0 = r.c1 = r.c2 = 0;
}
__device__ __forceinline__ void record_fold(Record& a, const Record& b) {
  a.s0 += b.s0;
  a.s1 += b.s1;
  a.lo = fmin(a.lo, b.lo);
  a.hi0 = fmax(a.hi0, b.hi0);
  a.hi1 = fmax(a.hi1, b.hi1);
  a.c0 += b.c0;
  a.c1 += b.c1;
  a.c2 += b.c2;
}
// lane 0 <- the wavefront's 64 records, folded by a fixed tree
__device__ __forceinline__ void record_fold_wave(Record& r) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    Record o;
    o.s0 = __shfl_down(r.s0, off);
    o.s1 = __shfl_down(r.s1, off);
    o.lo = __shfl_down(r.lo, off);
    o.hi0 = __shfl_down(r.hi0, off);
    o.hi1 = __shfl_down(r.hi1, off);
    o.c0 = __shfl_down(r.c0, off);
    o.c1 = __shfl_down(r.c1, off);
    o.c2 = __shfl_down(r.c2, off);
    record_fold(r, o);
  }
}

// ------------------------------------------------------------------------------------------------ epilogues
// take() is called by every lane of every wavefront the same number of times (valid == false: a padded row or
// column, which contributes nothing); finish() once per workgroup.
struct RecordArgs {
  Record* partials;         // one per workgroup
  const void* ref;          // error: the original, C order
  const int64_t* row_off;   // error: [m]
  const int64_t* col_off;   // error: [n], in the column order of B as the kernel sees it
  int64_t numel;            // error: elements of ref
  double clip_lo, clip_hi;  // moments: only clip_lo <= v <= clip_hi enters the four statistics
};

template <typename T, bool ERR>
struct RecordEpi {
  typedef RecordArgs Args;
  Record r;
  __device__ __forceinline__ void begin(const Args&) { record_clear(r); }
  __device__ __forceinline__ void take(const Args& a, bool valid, int64_t row, int64_t col, T v) {
    if (!valid) return;
    if constexpr (ERR) {
      const int64_t at = a.row_off[row] + a.col_off[col];
      if (at < 0 || at >= a.numel) return;  // the tables are not trusted: nothing is read outside ref
      const double y = (double)static_cast<const T*>(a.ref)[at];
      const double d = (double)v - y;
      ++r.c0;
      if (d != d) {
        ++r.c1;
        return;
      }
      r.s0 += d * d;
      r.s1 += y * y;
      r.hi0 = fmax(r.hi0, fabs(d));
      r.hi1 = fmax(r.hi1, y);
    } else {
      ++r.c0;
      if (v != v) {
        ++r.c1;
        return;
      }
      const double d = (double)v;
      if (!(d >= a.clip_lo && d <= a.clip_hi)) return;
      ++r.c2;
      r.s0 += d;
      r.s1 += d * d;
      r.lo = fmin(r.lo, d);
      r.hi0 = fmax(r.hi0, d);
    }
  }
  __device__ __forceinline__ void finish(const Args& a) {
    __shared__ Record waves[4];
    record_fold_wave(r);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
      Record t = waves[0];
      for (int w = 1; w < 4; ++w) record_fold(t, waves[w]);
      a.partials[blockIdx.x] = t;
    }
  }
};

struct HistArgs {
  const void* edges;              // [bins + 1] in the element type, ascending
  unsigned long long* counts;     // [bins + 3]: the bins, then below, above, NaN
  int bins;
};

extern __shared__ double valstat_dyn_lds[];  // histogram: the edges, then the 32-bit counters

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

// ---- extremes along axes, and the place of the global extreme (core/axisext.py)
// A voxel becomes an unsigned key whose integer order is the order of the values: the bits with the sign bit set for
// v >= 0 and all bits flipped for v < 0, complemented once more when the minimum is wanted, so that "the extreme" is
// always the largest key.  -0 is made +0 first (v + 0), so the two compare equal.  NaN takes no part and gets key 0,
// which no other value maps to (-inf maps to 0x007F..., and so does +inf after the complement).
template <typename T>
struct KeyOf {
  typedef typename std::conditional<sizeof(T) == 4, unsigned int, unsigned long long>::type type;
};
template <typename T, bool MIN>
__host__ __device__ __forceinline__ typename KeyOf<T>::type ext_key(T v) {
  typedef typename KeyOf<T>::type K;
  if (v != v) return (K)0;
  v = v + (T)0;
  K b;
  __builtin_memcpy(&b, &v, sizeof(T));
  const K sign = (K)1 << (8 * sizeof(T) - 1);
  b ^= (b & sign) ? ~(K)0 : sign;
  return MIN ? (K)~b : b;
}
// the value of a key; key 0 (nothing taken) is NaN
template <typename T>
__host__ __device__ __forceinline__ T ext_value(typename KeyOf<T>::type key, bool min) {
  typedef typename KeyOf<T>::type K;
  if (key == 0) return (T)NAN;
  if (min) key = (K)~key;
  const K sign = (K)1 << (8 * sizeof(T) - 1);
  key ^= (key & sign) ? sign : ~(K)0;
  T v;
  __builtin_memcpy(&v, &key, sizeof(T));
  return v;
}

struct AxisArgs {
  const int64_t* row_out;    // [m]  offset into the projected array = row_out[r] + col_out[c]
  const int64_t* col_out;    // [n]  in the column order of B as the kernel sees it: equal entries are adjacent
  const int32_t* row_idx;    // [m]  coordinate along the reduced axis = row_idx[r] + col_idx[c] (index modes only)
  const int32_t* col_idx;    // [n]
  void* keys;                // [out_numel] KEYS: keys of the element type's width.  PACKED: 64-bit (key << 32 | ~index)
                             //             MATCH: the finished 64-bit keys of the first pass, read only
  unsigned long long* index; // [out_numel] MATCH: the smallest index whose key equals the stored one
  int64_t out_numel;
};

enum { kAxisKeys = 0, kAxisPacked = 1, kAxisMatch = 2 };

// Every cell of the projected array is the integer maximum of the scores sent to it, so the result does not depend
// on the order of arrival.  KEYS: score = key.  PACKED (fp32): score = key << 32 | (0xFFFFFFFF - index), the larger
// value and among equal values the smaller index.  MATCH (fp64, second pass of the same product): score =
// UINT64_MAX - index where the element's key equals the finished key of its cell, and the cell takes the minimum
// index.  Score 0 is "nothing".  Before the atomic, the lanes of one row that share a cell (their columns are
// adjacent: the planner sorts them so) fold by a segmented shuffle, only the first lane of a segment goes on, and it
// holds its score back while the next elements it takes have the same cell.
template <typename T, bool MIN, int MODE>
struct AxisEpi {
  typedef AxisArgs Args;
  typedef typename KeyOf<T>::type K;
  typedef typename std::conditional<MODE == kAxisKeys, K, unsigned long long>::type S;
  static constexpr int W = sizeof(T) == 4 ? 32 : 16;  // lanes of one row of an accumulator tile
  int64_t held_at;
  S held;

  __device__ __forceinline__ void begin(const Args&) {
    held_at = -1;
    held = 0;
  }
  __device__ __forceinline__ void send(const Args& a, int64_t at, S score) {
    if constexpr (MODE == kAxisKeys) {
      atomicMax(static_cast<K*>(a.keys) + at, score);
    } else if constexpr (MODE == kAxisPacked) {
      atomicMax(static_cast<unsigned long long*>(a.keys) + at, score);
    } else {
      atomicMin(a.index + at, ~score);
    }
  }
  __device__ __forceinline__ void take(const Args& a, bool valid, int64_t row, int64_t col, T v) {
    // a padded element has cell -1 and score 0: it shares a segment with padding only, and sends nothing
    int64_t at = -1;
    S score = 0;
    if (valid) {
      at = a.row_out[row] + a.col_out[col];
      if (at < 0 || at >= a.out_numel) at = -1;  // the tables are not trusted: nothing is touched outside the result
    }
    if (at >= 0) {
      const K key = ext_key<T, MIN>(v);
      if constexpr (MODE == kAxisKeys) {
        score = key;
      } else {
        const unsigned int idx = (unsigned int)(a.row_idx[row] + a.col_idx[col]);
        if constexpr (MODE == kAxisPacked)
          score = key ? ((unsigned long long)key << 32) | (0xFFFFFFFFu - idx) : 0ull;
        else
          score = (key && key == static_cast<const K*>(a.keys)[at]) ? ~(unsigned long long)idx : 0ull;
      }
    }
    // the W lanes of one row: segments of equal cells are contiguous, so doubling over "the lane `off` further on has
    // my cell" folds each segment into its first lane
    const int pos = (int)(threadIdx.x & (W - 1));
#pragma unroll
    for (int off = 1; off < W; off <<= 1) {
      const int64_t o_at = __shfl_down((long long)at, off, W);
      const S o_score = __shfl_down(score, off, W);
      if (pos + off < W && o_at == at && o_score > score) score = o_score;
    }
    const int64_t before = __shfl_up((long long)at, 1, W);
    const bool head = pos == 0 || before != at;
    if (!head || at < 0 || score == 0) return;
    if (at == held_at) {
      if (score > held) held = score;
      return;
    }
    if (held_at >= 0) send(a, held_at, held);
    held_at = at;
    held = score;
  }
  __device__ __forceinline__ void finish(const Args& a) {
    if (held_at >= 0) send(a, held_at, held);
  }
};

// the place of the global extreme: one (key, offset) per thread, the smaller offset on equal keys, no atomics
struct ArgRec {
  unsigned long long key;  // 0: nothing taken
  long long at;            // row_off[r] + col_off[c], the flat C-order index
};
__device__ __forceinline__ void argrec_fold(ArgRec& a, const ArgRec& b) {
  if (b.key > a.key || (b.key == a.key && b.key != 0 && b.at < a.at)) a = b;
}
__device__ __forceinline__ void argrec_fold_wave(ArgRec& r) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    ArgRec o;
    o.key = __shfl_down(r.key, off);
    o.at = __shfl_down(r.at, off);
    argrec_fold(r, o);
  }
}

struct ArgArgs {
  ArgRec* partials;        // one per workgroup
  const int64_t* row_off;  // [m]
  const int64_t* col_off;  // [n], in the column order of B as the kernel sees it
};

template <typename T, bool MIN>
struct ArgEpi {
  typedef ArgArgs Args;
  ArgRec r;
  __device__ __forceinline__ void begin(const Args&) { r.key = 0, r.at = -1; }
  __device__ __forceinline__ void take(const Args& a, bool valid, int64_t row, int64_t col, T v) {
    if (!valid) return;
    const ArgRec mine{(unsigned long long)ext_key<T, MIN>(v), (long long)(a.row_off[row] + a.col_off[col])};
    argrec_fold(r, mine);
  }
  __device__ __forceinline__ void finish(const Args& a) {
    __shared__ ArgRec waves[4];
    argrec_fold_wave(r);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
      ArgRec t = waves[0];
      for (int w = 1; w < 4; ++w) argrec_fold(t, waves[w]);
      a.partials[blockIdx.x] = t;
    }
  }
};

// ---- statistics per label of an atlas (core/labelstat.py)
// Which threads meet which label depends on the data, so no fixed tree folds the sums.  They are 64-bit fixed-point
// integers instead: q = llrint(v 2^s) into a signed sum, q2 = llrint(v v 2^s2) into an unsigned one, and integer
// addition gives the same bits in any order.  The scales follow from the extremes of the moments pass over the same
// operands (labelstat_scale_kernel), by the one rule below.
constexpr int kLabelWindow = 1024;  // labels of one launch: their LDS table (40 B each in fp64) fits beside the tiles
constexpr int kLabelMax = 4096;
constexpr int kLabelSlots = 6;      // global table: sum, sum of squares, count, NaN count, min key, max key (n_labels each)
constexpr int kLabelTail = 5;       // then: outside, overflow, s, s2, non-finite flag
enum { kTailOutside = 0, kTailOverflow = 1, kTailS = 2, kTailS2 = 3, kTailFlag = 4 };

// nb = ceil(log2 numel)
__host__ __device__ inline int labelstat_bits(int64_t numel) {
  int nb = 0;
  while (nb < 62 && ((int64_t)1 << nb) < numel) ++nb;
  return nb;
}
// maxabs < 2^e (frexp), s = 61 - nb - e, so that numel * |v| 2^s <= 2^61; s2 likewise from the fp64 product
// maxabs * maxabs, which bounds every fl(v * v) (2 e where the product leaves the fp64 range)
__host__ __device__ inline void labelstat_scale_rule(double maxabs, int64_t numel, int* s, int* s2) {
  *s = *s2 = 0;
  if (!(maxabs > 0.0)) return;
  const int nb = labelstat_bits(numel);
  int e = 0, e2 = 0;
  frexp(maxabs, &e);
  const double sq = maxabs * maxabs;
  if (sq > 0.0 && sq <= 1.7976931348623157e308) frexp(sq, &e2); else e2 = 2 * e;
  const int a = 61 - nb - e, b = 61 - nb - e2;
  *s = a < -1000 ? -1000 : (a > 1000 ? 1000 : a);
  *s2 = b < -1000 ? -1000 : (b > 1000 ? 1000 : b);
}

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
    int label;
    switch (a.lab_bytes) {  // uniform over the launch
      case 1: label = static_cast<const uint8_t*>(a.lab)[at]; break;
      case 2: label = static_cast<const int16_t*>(a.lab)[at]; break;
      default: label = static_cast<const int32_t*>(a.lab)[at]; break;
    }
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

// ------------------------------------------------------------------------------------------------ the product
// C = A (m x k) B (k x n), dense row-major, tile by tile on a persistent grid; column c of B is B[:, perm[c]] when
// perm is given (the columns in memory order of the volume, for a chain whose decode has no gather buffer).  Rows
// and columns beyond m and n are staged as zeros and handed to the epilogue as invalid.
template <typename T, typename Epi>
__global__ void __launch_bounds__(256)
valstat_product_kernel(const T* __restrict__ A, const T* __restrict__ B, const int32_t* __restrict__ perm, int64_t m,
                       int64_t n, int64_t k, const typename Epi::Args args) {
  constexpr int BK = sizeof(T) == 4 ? 16 : 8;
  constexpr int PAD = 4;
  __shared__ T As[BK][kBM + PAD];  // k-major, as gemm.hip stages them: a fragment read is consecutive words
  __shared__ T Bs[BK][kBN + PAD];

  Epi epi;
  epi.begin(args);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int64_t tiles_n = (n + kBN - 1) / kBN, tiles = (m + kBM - 1) / kBM * tiles_n;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t m0 = (t / tiles_n) * kBM, n0 = (t % tiles_n) * kBN;
    typename std::conditional<sizeof(T) == 4, f32x16, f64x4>::type acc[sizeof(T) == 4 ? 1 : 4];
    for (auto& a : acc)
      for (int r = 0; r < (sizeof(T) == 4 ? 16 : 4); ++r) a[r] = (T)0;

    for (int64_t k0 = 0; k0 < k; k0 += BK) {
      for (int e = tid; e < kBM * BK; e += 256) {
        const int r = e / BK, kk = e % BK;
        const int64_t gr = m0 + r, gk = k0 + kk;
        As[kk][r] = (gr < m && gk < k) ? A[gr * k + gk] : (T)0;
      }
      for (int e = tid; e < BK * kBN; e += 256) {
        const int kk = e / kBN, c = e % kBN;
        const int64_t gk = k0 + kk;
        int64_t gc = n0 + c;
        bool ok = gc < n && gk < k;
        if (ok && perm) {
          gc = perm[gc];
          ok = gc >= 0 && gc < n;
        }
        Bs[kk][c] = ok ? B[gk * n + gc] : (T)0;
      }
      __syncthreads();
      if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2)
          acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + (lane >> 5)][wm + (lane & 31)],
                                                        Bs[kk + (lane >> 5)][wn + (lane & 31)], acc[0], 0, 0, 0);
      } else {
#pragma unroll
        for (int kk = 0; kk < BK; kk += 4) {
          double a[2], b[2];
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            a[i] = As[kk + (lane >> 4)][wm + 16 * i + (lane & 15)];
            b[i] = Bs[kk + (lane >> 4)][wn + 16 * i + (lane & 15)];
          }
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[2 * i + j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[2 * i + j], 0, 0, 0);
        }
      }
      __syncthreads();
    }

    if constexpr (sizeof(T) == 4) {
      const int64_t col = n0 + wn + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t row = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        epi.take(args, row < m && col < n, row, col, acc[0][r]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int64_t col = n0 + wn + 16 * j + (lane & 15);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int64_t row = m0 + wm + 16 * i + (lane >> 4) + 4 * r;
            epi.take(args, row < m && col < n, row, col, acc[2 * i + j][r]);
          }
        }
    }
  }
  epi.finish(args);
}

// result <- the partial records folded in index order (one wavefront)
__global__ void __launch_bounds__(64) valstat_fold_kernel(const Record* __restrict__ partials, int count, Record* result) {
  Record r;
  record_clear(r);
  for (int i = threadIdx.x; i < count; i += 64) record_fold(r, partials[i]);
  record_fold_wave(r);
  if (threadIdx.x == 0) *result = r;
}

template <typename K>
__global__ void __launch_bounds__(256) axisext_fill_kernel(K* __restrict__ p, int64_t count, K value) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < count; e += (int64_t)gridDim.x * 256) p[e] = value;
}

// keys -> values, in place (the key buffer is the result buffer); an untouched cell becomes NaN.  index (may be
// NULL, fp64 with indices): a cell no pass touched still holds INT64_MAX and becomes -1.
template <typename T>
__global__ void __launch_bounds__(256)
axisext_decode_kernel(void* __restrict__ values, long long* __restrict__ index, int64_t count, bool min) {
  typedef typename KeyOf<T>::type K;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < count; e += (int64_t)gridDim.x * 256) {
    const K key = static_cast<const K*>(values)[e];
    static_cast<T*>(values)[e] = ext_value<T>(key, min);
    if (index && index[e] == INT64_MAX) index[e] = -1;
  }
}

// fp32 with indices: packed[e] = key << 32 | (0xFFFFFFFF - index) -> values[e] and, in place, the int64 index
__global__ void __launch_bounds__(256)
axisext_unpack_kernel(unsigned long long* __restrict__ packed, float* __restrict__ values, int64_t count, bool min) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < count; e += (int64_t)gridDim.x * 256) {
    const unsigned long long p = packed[e];
    values[e] = ext_value<float>((unsigned int)(p >> 32), min);
    reinterpret_cast<long long*>(packed)[e] = p ? (long long)(0xFFFFFFFFu - (unsigned int)p) : -1ll;
  }
}

// result <- the partial places folded in index order (one wavefront)
__global__ void __launch_bounds__(64) argext_fold_kernel(const ArgRec* __restrict__ partials, int count, ArgRec* result) {
  ArgRec r{0ull, -1ll};
  for (int i = threadIdx.x; i < count; i += 64) argrec_fold(r, partials[i]);
  argrec_fold_wave(r);
  if (threadIdx.x == 0) *result = r;
}

// ------------------------------------------------------------------------------------------------ host
// (ErrorTables, valstat_check, Operands, valstat_run_chain, valstat_grid: valstat_device.h)

// moments (err == NULL) or the error against an original: h_stats[4], h_counts[3]
template <typename T>
int valstat_record(int L, const int64_t* h_dims, const int64_t* h_bonds, const T* const* h_cores, const ErrorTables* err,
                   double clip_lo, double clip_hi, double* h_stats, int64_t* h_counts, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  NDMPS_REQUIRE(L >= 1 && h_dims && h_bonds && h_stats && h_counts, "bad valstat argument");
  NDMPS_REQUIRE(clip_lo == clip_lo && clip_hi == clip_hi, "moments: the clip range must not be NaN");
  const ChainStatsPlan sp = ndmps::chain_stats_plan(L, h_dims, h_bonds, sizeof(T), 0);
  NDMPS_TRY(valstat_check(sp, h_dims, h_bonds, h_cores, d_ws, ws_bytes, err));
  hipStream_t s = (hipStream_t)stream;
  Operands ops;
  NDMPS_TRY(valstat_run_chain(sp, h_cores, d_ws, err ? err->col_perm : nullptr, s, &ops));
  const ChainProduct& q = sp.reduced;
  const int grid = valstat_grid(q);
  Record* partials = (Record*)((char*)d_ws + sp.off_partials);
  Record* result = (Record*)((char*)d_ws + sp.off_result);
  RecordArgs args{partials, nullptr, nullptr, nullptr, sp.chain.numel, clip_lo, clip_hi};
  if (err) {
    args.ref = err->ref;
    args.row_off = err->row_off;
    args.col_off = err->col_off;
    hipLaunchKernelGGL((valstat_product_kernel<T, RecordEpi<T, true>>), dim3(grid), dim3(256), 0, s, (const T*)ops.A,
                       (const T*)ops.B, ops.perm, q.m, q.n, q.k, args);
  } else {
    hipLaunchKernelGGL((valstat_product_kernel<T, RecordEpi<T, false>>), dim3(grid), dim3(256), 0, s, (const T*)ops.A,
                       (const T*)ops.B, ops.perm, q.m, q.n, q.k, args);
  }
  NDMPS_LAUNCH_CHECK();
  hipLaunchKernelGGL(valstat_fold_kernel, dim3(1), dim3(64), 0, s, partials, grid, result);
  NDMPS_LAUNCH_CHECK();
  Record host;
  NDMPS_CHECK_HIP(hipMemcpyAsync(&host, result, sizeof(Record), hipMemcpyDeviceToHost, s));
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));
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
  for (int i = 0; i <= n_bins; ++i)
    NDMPS_REQUIRE(h_edges[i] == h_edges[i] && (i == 0 || h_edges[i] >= h_edges[i - 1]),
                  "histogram: edges must be ascending and not NaN (edge %d)", i);
  const ChainStatsPlan sp = ndmps::chain_stats_plan(L, h_dims, h_bonds, sizeof(T), n_bins);
  NDMPS_TRY(valstat_check(sp, h_dims, h_bonds, h_cores, d_ws, ws_bytes, nullptr));
  const ChainProduct& q = sp.reduced;
  const int grid = valstat_grid(q);
  // a workgroup counts in 32 bits until its one flush
  NDMPS_REQUIRE(ceil_div(ceil_div(q.m, kBM) * ceil_div(q.n, kBN), grid) * kBM * kBN < (int64_t)UINT32_MAX,
                "histogram: volume too large for 32-bit counters per workgroup");
  hipStream_t s = (hipStream_t)stream;
  Operands ops;
  NDMPS_TRY(valstat_run_chain(sp, h_cores, d_ws, nullptr, s, &ops));
  unsigned long long* counts = (unsigned long long*)((char*)d_ws + sp.off_hist);
  T* edges = (T*)((char*)d_ws + sp.off_edges);
  NDMPS_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)(n_bins + 3) * 8, s));
  NDMPS_CHECK_HIP(hipMemcpyAsync(edges, h_edges, (size_t)(n_bins + 1) * sizeof(T), hipMemcpyHostToDevice, s));
  const HistArgs args{edges, counts, n_bins};
  const size_t lds = ((size_t)(n_bins + 1) * sizeof(T) + 7) / 8 * 8 + (size_t)(n_bins + 3) * 4;
  hipLaunchKernelGGL((valstat_product_kernel<T, HistEpi<T>>), dim3(grid), dim3(256), lds, s, (const T*)ops.A,
                     (const T*)ops.B, ops.perm, q.m, q.n, q.k, args);
  NDMPS_LAUNCH_CHECK();
  static_assert(sizeof(int64_t) == sizeof(unsigned long long), "counter width");
  NDMPS_CHECK_HIP(hipMemcpyAsync(h_counts, counts, (size_t)(n_bins + 3) * 8, hipMemcpyDeviceToHost, s));
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));
  return NDMPS_OK;
}

template <typename T, typename Epi>
int axisext_product(const ChainProduct& q, const Operands& ops, const typename Epi::Args& args, hipStream_t s) {
  hipLaunchKernelGGL((valstat_product_kernel<T, Epi>), dim3(valstat_grid(q)), dim3(256), 0, s, (const T*)ops.A,
                     (const T*)ops.B, ops.perm, q.m, q.n, q.k, args);
  NDMPS_LAUNCH_CHECK();
  return NDMPS_OK;
}

// the extreme (op 0: max, 1: min) of every cell of the projected array, and with the index tables its place along
// the one reduced axis
template <typename T>
int axisext_run(int L, const int64_t* h_dims, const int64_t* h_bonds, const T* const* h_cores, int op,
                const int64_t* d_row_out, const int64_t* d_col_out, const int32_t* d_col_perm, int64_t n_cols,
                const int32_t* d_row_idx, const int32_t* d_col_idx, int64_t out_numel, T* d_values, int64_t* d_index,
                void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  typedef typename KeyOf<T>::type K;
  NDMPS_REQUIRE(L >= 1 && h_dims && h_bonds, "bad axisext argument");
  NDMPS_REQUIRE(op == 0 || op == 1, "axisext: op %d is neither 0 (max) nor 1 (min)", op);
  NDMPS_REQUIRE(d_row_out && d_col_out && d_col_perm && d_values && out_numel >= 1, "axisext: NULL table or result");
  const bool index = d_index != nullptr;
  NDMPS_REQUIRE((d_row_idx != nullptr) == index && (d_col_idx != nullptr) == index,
                "axisext: the index tables and d_index are given together or not at all");
  const ChainStatsPlan sp = ndmps::chain_stats_plan(L, h_dims, h_bonds, sizeof(T), 0);
  // valstat_check's table conditions (none NULL, n_cols is the last product's); the result stands where the original does
  const ErrorTables tables{d_values, d_row_out, d_col_out, d_col_perm, n_cols};
  NDMPS_TRY(valstat_check(sp, h_dims, h_bonds, h_cores, d_ws, ws_bytes, &tables));
  hipStream_t s = (hipStream_t)stream;
  Operands ops;
  NDMPS_TRY(valstat_run_chain(sp, h_cores, d_ws, d_col_perm, s, &ops));
  const ChainProduct& q = sp.reduced;
  const bool min = op == 1;
  const dim3 flat(grid1d(out_numel)), threads(256);
  AxisArgs args{d_row_out, d_col_out, d_row_idx, d_col_idx, d_values, (unsigned long long*)d_index, out_numel};
  if constexpr (sizeof(T) == 4) {
    if (index) {  // one pass, the packed keys in d_index
      args.keys = d_index;
      hipLaunchKernelGGL(axisext_fill_kernel<unsigned long long>, flat, threads, 0, s, (unsigned long long*)d_index, out_numel, 0ull);
      NDMPS_LAUNCH_CHECK();
      NDMPS_TRY(min ? (axisext_product<T, AxisEpi<T, true, kAxisPacked>>(q, ops, args, s))
                    : (axisext_product<T, AxisEpi<T, false, kAxisPacked>>(q, ops, args, s)));
      hipLaunchKernelGGL(axisext_unpack_kernel, flat, threads, 0, s, (unsigned long long*)d_index, (float*)d_values, out_numel, min);
      NDMPS_LAUNCH_CHECK();
      return NDMPS_OK;
    }
  }
  hipLaunchKernelGGL(axisext_fill_kernel<K>, flat, threads, 0, s, (K*)d_values, out_numel, (K)0);
  NDMPS_LAUNCH_CHECK();
  NDMPS_TRY(min ? (axisext_product<T, AxisEpi<T, true, kAxisKeys>>(q, ops, args, s))
                : (axisext_product<T, AxisEpi<T, false, kAxisKeys>>(q, ops, args, s)));
  if constexpr (sizeof(T) == 8) {
    if (index) {  // the same product again: an element whose key is its cell's finished key offers its index
      hipLaunchKernelGGL(axisext_fill_kernel<unsigned long long>, flat, threads, 0, s, (unsigned long long*)d_index, out_numel,
                         (unsigned long long)INT64_MAX);
      NDMPS_LAUNCH_CHECK();
      NDMPS_TRY(min ? (axisext_product<T, AxisEpi<T, true, kAxisMatch>>(q, ops, args, s))
                    : (axisext_product<T, AxisEpi<T, false, kAxisMatch>>(q, ops, args, s)));
    }
  }
  hipLaunchKernelGGL(axisext_decode_kernel<T>, flat, threads, 0, s, (void*)d_values, (long long*)d_index, out_numel, min);
  NDMPS_LAUNCH_CHECK();
  return NDMPS_OK;
}

// the global extreme and its flat C-order index (-1 and NaN for a volume of NaN only)
template <typename T>
int argext_run(int L, const int64_t* h_dims, const int64_t* h_bonds, const T* const* h_cores, int op,
               const int64_t* d_row_off, const int64_t* d_col_off, const int32_t* d_col_perm, int64_t n_cols,
               double* h_value, int64_t* h_flat_index, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  typedef typename KeyOf<T>::type K;
  NDMPS_REQUIRE(L >= 1 && h_dims && h_bonds && h_value && h_flat_index, "bad argext argument");
  NDMPS_REQUIRE(op == 0 || op == 1, "argext: op %d is neither 0 (max) nor 1 (min)", op);
  const ChainStatsPlan sp = ndmps::chain_stats_plan(L, h_dims, h_bonds, sizeof(T), 0);
  const ErrorTables tables{d_row_off, d_row_off, d_col_off, d_col_perm, n_cols};  // no original: the row table stands in
  NDMPS_TRY(valstat_check(sp, h_dims, h_bonds, h_cores, d_ws, ws_bytes, &tables));
  hipStream_t s = (hipStream_t)stream;
  Operands ops;
  NDMPS_TRY(valstat_run_chain(sp, h_cores, d_ws, d_col_perm, s, &ops));
  const ChainProduct& q = sp.reduced;
  static_assert(sizeof(ArgRec) <= ndmps::kValstatRecordBytes, "a place fits a record slot");
  ArgRec* partials = (ArgRec*)((char*)d_ws + sp.off_partials);
  ArgRec* result = (ArgRec*)((char*)d_ws + sp.off_result);
  const ArgArgs args{partials, d_row_off, d_col_off};
  NDMPS_TRY(op == 1 ? (axisext_product<T, ArgEpi<T, true>>(q, ops, args, s))
                    : (axisext_product<T, ArgEpi<T, false>>(q, ops, args, s)));
  hipLaunchKernelGGL(argext_fold_kernel, dim3(1), dim3(64), 0, s, partials, valstat_grid(q), result);
  NDMPS_LAUNCH_CHECK();
  ArgRec host;
  NDMPS_CHECK_HIP(hipMemcpyAsync(&host, result, sizeof(ArgRec), hipMemcpyDeviceToHost, s));
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));
  *h_value = (double)ext_value<T>((K)host.key, op == 1);
  *h_flat_index = host.key ? (int64_t)host.at : -1;
  return NDMPS_OK;
}

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
  NDMPS_TRY(valstat_check(sp, h_dims, h_bonds, h_cores, d_ws, ws_bytes, &tables));
  const int64_t table_bytes = labelstat_table_bytes(n_labels);
  if (ws_bytes < sp.total_bytes + table_bytes) {
    ndmps::set_error("labelstat workspace too small: %lld < %lld", (long long)ws_bytes, (long long)(sp.total_bytes + table_bytes));
    return NDMPS_EWORKSPACE;
  }
  const ChainProduct& q = sp.reduced;
  const int grid = valstat_grid(q);
  // a workgroup counts in 32 bits until its one flush
  NDMPS_REQUIRE(ceil_div(ceil_div(q.m, kBM) * ceil_div(q.n, kBN), grid) * kBM * kBN < (int64_t)UINT32_MAX,
                "label statistics: volume too large for 32-bit counters per workgroup");
  hipStream_t s = (hipStream_t)stream;
  Operands ops;
  NDMPS_TRY(valstat_run_chain(sp, h_cores, d_ws, d_col_perm, s, &ops));
  Record* partials = (Record*)((char*)d_ws + sp.off_partials);
  Record* result = (Record*)((char*)d_ws + sp.off_result);
  unsigned long long* table = (unsigned long long*)((char*)d_ws + sp.total_bytes);
  const int64_t numel = sp.chain.numel;

  const RecordArgs margs{partials, nullptr, nullptr, nullptr, numel, -INFINITY, INFINITY};
  hipLaunchKernelGGL((valstat_product_kernel<T, RecordEpi<T, false>>), dim3(grid), dim3(256), 0, s, (const T*)ops.A,
                     (const T*)ops.B, ops.perm, q.m, q.n, q.k, margs);
  NDMPS_LAUNCH_CHECK();
  hipLaunchKernelGGL(valstat_fold_kernel, dim3(1), dim3(64), 0, s, partials, grid, result);
  NDMPS_LAUNCH_CHECK();
  NDMPS_CHECK_HIP(hipMemsetAsync(table, 0, (size_t)table_bytes, s));
  hipLaunchKernelGGL(labelstat_scale_kernel, dim3(1), dim3(1), 0, s, result, numel,
                     (long long*)(table + (size_t)kLabelSlots * n_labels));
  NDMPS_LAUNCH_CHECK();
  for (int base = 0; base < n_labels; base += kLabelWindow) {
    const int window = std::min(kLabelWindow, n_labels - base);
    const LabelArgs args{d_labels, label_elem_bytes, d_row_off, d_col_off, numel, table, n_labels, base, window,
                         labelstat_bits(numel)};
    const size_t lds = (size_t)window * (16 + 2 * sizeof(K) + 8) + 8;
    hipLaunchKernelGGL((valstat_product_kernel<T, LabelEpi<T>>), dim3(grid), dim3(256), lds, s, (const T*)ops.A,
                       (const T*)ops.B, ops.perm, q.m, q.n, q.k, args);
    NDMPS_LAUNCH_CHECK();
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

extern "C" int ndmps_axisext_f32(int L, const int64_t* h_dims, const int64_t* h_bonds, const float* const* h_cores, int op,
                                 const int64_t* d_row_out, const int64_t* d_col_out, const int32_t* d_col_perm,
                                 int64_t n_cols, const int32_t* d_row_idx, const int32_t* d_col_idx, int64_t out_numel,
                                 float* d_values, int64_t* d_index, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  return axisext_run<float>(L, h_dims, h_bonds, h_cores, op, d_row_out, d_col_out, d_col_perm, n_cols, d_row_idx, d_col_idx,
                            out_numel, d_values, d_index, d_ws, ws_bytes, stream);
}
extern "C" int ndmps_axisext_f64(int L, const int64_t* h_dims, const int64_t* h_bonds, const double* const* h_cores, int op,
                                 const int64_t* d_row_out, const int64_t* d_col_out, const int32_t* d_col_perm,
                                 int64_t n_cols, const int32_t* d_row_idx, const int32_t* d_col_idx, int64_t out_numel,
                                 double* d_values, int64_t* d_index, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  return axisext_run<double>(L, h_dims, h_bonds, h_cores, op, d_row_out, d_col_out, d_col_perm, n_cols, d_row_idx, d_col_idx,
                             out_numel, d_values, d_index, d_ws, ws_bytes, stream);
}
extern "C" int ndmps_argext_f32(int L, const int64_t* h_dims, const int64_t* h_bonds, const float* const* h_cores, int op,
                                const int64_t* d_row_off, const int64_t* d_col_off, const int32_t* d_col_perm,
                                int64_t n_cols, double* h_value, int64_t* h_flat_index, void* d_ws, int64_t ws_bytes,
                                ndmps_stream_t stream) {
  return argext_run<float>(L, h_dims, h_bonds, h_cores, op, d_row_off, d_col_off, d_col_perm, n_cols, h_value, h_flat_index,
                           d_ws, ws_bytes, stream);
}
extern "C" int ndmps_argext_f64(int L, const int64_t* h_dims, const int64_t* h_bonds, const double* const* h_cores, int op,
                                const int64_t* d_row_off, const int64_t* d_col_off, const int32_t* d_col_perm,
                                int64_t n_cols, double* h_value, int64_t* h_flat_index, void* d_ws, int64_t ws_bytes,
                                ndmps_stream_t stream) {
  return argext_run<double>(L, h_dims, h_bonds, h_cores, op, d_row_off, d_col_off, d_col_perm, n_cols, h_value, h_flat_index,
                            d_ws, ws_bytes, stream);
}

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
