// The voxels of the volume a chain decodes to that lie inside or outside an interval, or are NaN, from the cores: the
// one epilogue of the reducing product of the value statistics (valstat_device.h) whose output is a list.  The N
// voxels are never written; the caller counts first (the clipped moments pass) and gives exactly that many slots.
//
//   ndmps_select_*  <- NDMPS.find / find_nan / topk   (core/select.py)
//
// The slots are handed out by one 64-bit integer cursor, so the order of the list depends on the order of arrival;
// the host sorts the K pairs by their (unique) flat index, after which the same inputs give the same bytes.  The only
// atomic of this file is that integer add.
#include "common.h"
#include "typed.h"
#include "valstat_device.h"
#include "valstat_plan.h"

namespace {

enum { kSelectInside = 0, kSelectOutside = 1, kSelectNaN = 2 };

template <typename T>
struct SelectArgs {
  const int64_t* row_off;      // [m]  flat C-order index = row_off[r] + col_off[c]
  const int64_t* col_off;      // [n]  in the column order of B as the kernel sees it
  int64_t numel;               // voxels of the volume
  int mode;                    // kSelectInside: lo <= v <= hi; kSelectOutside: not NaN and not inside; kSelectNaN
  T lo, hi;
  unsigned long long* cursor;  // matches seen so far, those beyond capacity included
  int64_t capacity;            // slots of index and values
  int64_t* index;
  T* values;
};

// Every lane of a wavefront reaches take() the same number of times (the epilogue contract), so the ballot sees all
// 64 lanes.  A wavefront with matches makes one add of their number and every matching lane takes the slot
// base + (matches in the lanes below it); a slot at or beyond capacity is counted and not written.
template <typename T>
struct SelectEpi {
  typedef SelectArgs<T> Args;
  __device__ __forceinline__ void begin(const Args&) {}
  __device__ __forceinline__ void take(const Args& a, bool valid, int64_t row, int64_t col, T v) {
    int64_t at = -1;
    bool match = false;
    if (valid) {
      at = a.row_off[row] + a.col_off[col];
      if (at >= 0 && at < a.numel) {  // the tables are not trusted: an element outside the volume is dropped
        const bool nan = v != v, inside = v >= a.lo && v <= a.hi;
        match = a.mode == kSelectNaN ? nan : a.mode == kSelectInside ? inside : (!nan && !inside);
      }
    }
    const unsigned long long mask = __ballot(match);
    if (mask == 0) return;
    const int lane = (int)(threadIdx.x & 63);
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(a.cursor, (unsigned long long)__popcll(mask));
    base = __shfl(base, 0);
    if (!match) return;
    const int64_t slot = (int64_t)base + __popcll(mask & ((1ull << lane) - 1ull));
    if (slot < a.capacity) {
      a.index[slot] = at;
      a.values[slot] = v;
    }
  }
  __device__ __forceinline__ void finish(const Args&) {}
};

__global__ void select_zero_kernel(unsigned long long* cursor) { *cursor = 0ull; }

template <typename T>
int select_run(int L, const int64_t* h_dims, const int64_t* h_bonds, const T* const* h_cores, int mode, double lo, double hi,
               const int64_t* d_row_off, const int64_t* d_col_off, const int32_t* d_col_perm, int64_t n_cols,
               int64_t capacity, int64_t* d_index, T* d_values, int64_t* h_total, void* d_ws, int64_t ws_bytes,
               ndmps_stream_t stream) {
  NDMPS_REQUIRE(L >= 1 && h_dims && h_bonds && h_total, "bad select argument");
  NDMPS_REQUIRE(mode == kSelectInside || mode == kSelectOutside || mode == kSelectNaN,
                "select: mode %d is neither 0 (inside), 1 (outside) nor 2 (NaN)", mode);
  NDMPS_REQUIRE(mode == kSelectNaN || lo <= hi, "select: the bounds must not be NaN, and lo <= hi");
  NDMPS_REQUIRE(capacity >= 0 && (capacity == 0 || (d_index && d_values)), "select: %lld slots and a NULL result",
                (long long)capacity);
  const ChainStatsPlan sp = ndmps::chain_stats_plan(L, h_dims, h_bonds, sizeof(T), 0);
  const ErrorTables tables{d_row_off, d_row_off, d_col_off, d_col_perm, n_cols};  // no original: the row table stands in
  StatCall<T> c(sp, h_cores, d_ws, stream);
  NDMPS_TRY(c.check(h_dims, h_bonds, ws_bytes, &tables));
  NDMPS_TRY(c.run(d_col_perm));
  unsigned long long* cursor = c.template result<unsigned long long>();
  hipLaunchKernelGGL(select_zero_kernel, dim3(1), dim3(1), 0, c.s, cursor);
  NDMPS_LAUNCH_CHECK();
  const SelectArgs<T> args{d_row_off, d_col_off, sp.chain.numel, mode, (T)lo, (T)hi, cursor, capacity, d_index, d_values};
  NDMPS_TRY((stat_launch<T, SelectEpi<T>>(c.q, c.ops, args, c.grid, 0, c.s)));
  unsigned long long total = 0;
  NDMPS_CHECK_HIP(hipMemcpyAsync(&total, cursor, sizeof(total), hipMemcpyDeviceToHost, c.s));
  NDMPS_CHECK_HIP(hipStreamSynchronize(c.s));
  *h_total = (int64_t)total;
  return NDMPS_OK;
}

}  // namespace

extern "C" int ndmps_select_f32(int L, const int64_t* h_dims, const int64_t* h_bonds, const float* const* h_cores, int mode,
                                double lo, double hi, const int64_t* d_row_off, const int64_t* d_col_off,
                                const int32_t* d_col_perm, int64_t n_cols, int64_t capacity, int64_t* d_index,
                                float* d_values, int64_t* h_total, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  return select_run<float>(L, h_dims, h_bonds, h_cores, mode, lo, hi, d_row_off, d_col_off, d_col_perm, n_cols, capacity,
                           d_index, d_values, h_total, d_ws, ws_bytes, stream);
}
extern "C" int ndmps_select_f64(int L, const int64_t* h_dims, const int64_t* h_bonds, const double* const* h_cores, int mode,
                                double lo, double hi, const int64_t* d_row_off, const int64_t* d_col_off,
                                const int32_t* d_col_perm, int64_t n_cols, int64_t capacity, int64_t* d_index,
                                double* d_values, int64_t* h_total, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  return select_run<double>(L, h_dims, h_bonds, h_cores, mode, lo, hi, d_row_off, d_col_off, d_col_perm, n_cols, capacity,
                            d_index, d_values, h_total, d_ws, ws_bytes, stream);
}
