// Extremes of the volume a chain decodes to along axes, and the place of the global extreme, from the cores: two
// epilogues of the reducing product of the value statistics (valstat.hip, valstat_device.h), so the N voxels are never
// written.
//
//   ndmps_axisext_*  <- NDMPS.amax / amin / argmax / argmin along axes   (core/axisext.py)
//   ndmps_argext_*   <- NDMPS.argmax / argmin of the whole volume
//
// The extremes along axes take integer maxima of order-preserving keys (ext_key, valstat_device.h) with integer
// atomics; the place of the global extreme is a record folded by the fixed tree of the moments: the same inputs give
// the same bits.
#include "common.h"
#include "typed.h"
#include "valstat_device.h"
#include "valstat_plan.h"

namespace {

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

  __device__ __forceinline__ void clear() { key = 0, at = -1; }
  __device__ __forceinline__ void fold(const ArgRec& b) {
    if (b.key > key || (b.key == key && b.key != 0 && b.at < at)) *this = b;
  }
};

struct ArgArgs {
  ArgRec* partials;        // one per workgroup
  const int64_t* row_off;  // [m]
  const int64_t* col_off;  // [n], in the column order of B as the kernel sees it
};

template <typename T, bool MIN>
struct ArgEpi {
  typedef ArgArgs Args;
  ArgRec r;
  __device__ __forceinline__ void begin(const Args&) { r.clear(); }
  __device__ __forceinline__ void take(const Args& a, bool valid, int64_t row, int64_t col, T v) {
    if (!valid) return;
    const ArgRec mine{(unsigned long long)ext_key<T, MIN>(v), (long long)(a.row_off[row] + a.col_off[col])};
    r.fold(mine);
  }
  __device__ __forceinline__ void finish(const Args& a) { stat_fold_group(r, &a.partials[blockIdx.x]); }
};

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
  StatCall<T> c(sp, h_cores, d_ws, stream);
  NDMPS_TRY(c.check(h_dims, h_bonds, ws_bytes, &tables));
  NDMPS_TRY(c.run(d_col_perm));
  hipStream_t s = c.s;
  const bool min = op == 1;
  const dim3 flat(grid1d(out_numel)), threads(256);
  AxisArgs args{d_row_out, d_col_out, d_row_idx, d_col_idx, d_values, (unsigned long long*)d_index, out_numel};
  if constexpr (sizeof(T) == 4) {
    if (index) {  // one pass, the packed keys in d_index
      args.keys = d_index;
      hipLaunchKernelGGL(axisext_fill_kernel<unsigned long long>, flat, threads, 0, s, (unsigned long long*)d_index, out_numel, 0ull);
      NDMPS_LAUNCH_CHECK();
      NDMPS_TRY(min ? (stat_launch<T, AxisEpi<T, true, kAxisPacked>>(c.q, c.ops, args, c.grid, 0, s))
                    : (stat_launch<T, AxisEpi<T, false, kAxisPacked>>(c.q, c.ops, args, c.grid, 0, s)));
      hipLaunchKernelGGL(axisext_unpack_kernel, flat, threads, 0, s, (unsigned long long*)d_index, (float*)d_values, out_numel, min);
      NDMPS_LAUNCH_CHECK();
      return NDMPS_OK;
    }
  }
  hipLaunchKernelGGL(axisext_fill_kernel<K>, flat, threads, 0, s, (K*)d_values, out_numel, (K)0);
  NDMPS_LAUNCH_CHECK();
  NDMPS_TRY(min ? (stat_launch<T, AxisEpi<T, true, kAxisKeys>>(c.q, c.ops, args, c.grid, 0, s))
                : (stat_launch<T, AxisEpi<T, false, kAxisKeys>>(c.q, c.ops, args, c.grid, 0, s)));
  if constexpr (sizeof(T) == 8) {
    if (index) {  // the same product again: an element whose key is its cell's finished key offers its index
      hipLaunchKernelGGL(axisext_fill_kernel<unsigned long long>, flat, threads, 0, s, (unsigned long long*)d_index, out_numel,
                         (unsigned long long)INT64_MAX);
      NDMPS_LAUNCH_CHECK();
      NDMPS_TRY(min ? (stat_launch<T, AxisEpi<T, true, kAxisMatch>>(c.q, c.ops, args, c.grid, 0, s))
                    : (stat_launch<T, AxisEpi<T, false, kAxisMatch>>(c.q, c.ops, args, c.grid, 0, s)));
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
  StatCall<T> c(sp, h_cores, d_ws, stream);
  NDMPS_TRY(c.check(h_dims, h_bonds, ws_bytes, &tables));
  NDMPS_TRY(c.run(d_col_perm));
  static_assert(sizeof(ArgRec) <= ndmps::kValstatRecordBytes, "a place fits a record slot");
  const ArgArgs args{c.template partials<ArgRec>(), d_row_off, d_col_off};
  NDMPS_TRY(op == 1 ? (stat_launch<T, ArgEpi<T, true>>(c.q, c.ops, args, c.grid, 0, c.s))
                    : (stat_launch<T, ArgEpi<T, false>>(c.q, c.ops, args, c.grid, 0, c.s)));
  ArgRec host;
  NDMPS_TRY(stat_fetch_record(args.partials, c.grid, c.template result<ArgRec>(), &host, c.s));
  *h_value = (double)ext_value<T>((K)host.key, op == 1);
  *h_flat_index = host.key ? (int64_t)host.at : -1;
  return NDMPS_OK;
}

}  // namespace

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
