// The device layer and the host prologue of the statistics family: valstat.hip (moments, histogram, error),
// axisext.hip (extremes along axes, the place of the global extreme), labelstat.hip (statistics per label), each one
// chain reduced, pairstat.hip (two chains reduced together) and labelpair.hip (two values per voxel under a label; the
// pair layer on top of this one is pairstat_device.h, the label read and the scale rule labelstat_device.h).  One text
// each of
//
//   the tile       StatTile, stat_tile_accumulate (staging and MFMA k-loop), stat_tile_for_each (the walk over a
//                  wavefront's accumulator slots), and valstat_product_kernel, the single-chain product on them
//   the records    stat_fold_wave / stat_fold_group / stat_fold_kernel over any record with clear() and fold()
//   the moments    Record, RecordEpi (labelstat.hip runs the moments pass too), the order-preserving keys
//   the histogram  the bin search and the fold of the lanes that share the first lane's bin
//   the host       the argument check of a chain, the products before the last one, StatCall (plan, check, run-chain,
//                  grid), stat_launch, stat_counters_fit, stat_edges_ok, stat_fold, stat_fetch_record
//
// Internal linkage, as typed.h: each translation unit gets its own copy of what it uses.
#pragma once
#include <math.h>

#include <algorithm>
#include <type_traits>

#include "common.h"
#include "typed.h"
#include "valstat_plan.h"

namespace {

using ndmps::ceil_div;
using ndmps::ChainProduct;
using ndmps::ChainStatsPlan;
using ndmps::f64x4;
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBM = 64, kBN = 64;  // tile of a workgroup: 2 x 2 wavefronts of 32 x 32

extern __shared__ double valstat_dyn_lds[];  // the dynamic LDS of a single-chain epilogue (histogram, label statistics)

// ------------------------------------------------------------------------------------------------ the epilogue contract
// A product kernel hands the elements of its accumulator tiles to an epilogue Epi with a plain-data Epi::Args:
//   begin(args)   once per thread before the first tile (it may __syncthreads(): every thread calls it)
//   take(args, valid, row, col, v)  or, for a pair,  take(args, valid, row, col, va, vb)
//                 by every lane of every wavefront the same number of times; valid == false: a padded row or column,
//                 which contributes nothing
//   finish(args)  once per thread after the last tile (it may __syncthreads())

// ------------------------------------------------------------------------------------------------ the tile
template <typename T>
struct StatTile {
  static constexpr int BK = sizeof(T) == 4 ? 16 : 8;
  static constexpr int PAD = 4;
  typedef typename std::conditional<sizeof(T) == 4, f32x16, f64x4>::type Frag;
  static constexpr int kFrags = sizeof(T) == 4 ? 1 : 4, kPerFrag = sizeof(T) == 4 ? 16 : 4;
  typedef T StageA[BK][kBM + PAD];  // k-major, as gemm.hip stages them: a fragment read is consecutive words
  typedef T StageB[BK][kBN + PAD];
};

// acc <- the tile (m0, n0) of A (m x k) B (k x n), dense row-major, through the caller's LDS buffers
// (v_mfma_f32_32x32x2_f32 / v_mfma_f64_16x16x4_f64, lane maps as in gemm.hip); column c of B is B[:, perm[c]] when perm
// is given (the columns in memory order of the volume, for a chain whose decode has no gather buffer).  Rows and
// columns beyond m and n, and columns whose perm entry is out of range, are staged as zeros.
template <typename T>
__device__ __forceinline__ void stat_tile_accumulate(const T* __restrict__ A, const T* __restrict__ B,
                                                     const int32_t* __restrict__ perm, int64_t m, int64_t n, int64_t k,
                                                     int64_t m0, int64_t n0, typename StatTile<T>::StageA& As,
                                                     typename StatTile<T>::StageB& Bs,
                                                     typename StatTile<T>::Frag (&acc)[StatTile<T>::kFrags]) {
  constexpr int BK = StatTile<T>::BK;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  for (auto& a : acc)
    for (int r = 0; r < StatTile<T>::kPerFrag; ++r) a[r] = (T)0;

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
}

// f(valid, row, col, frag, slot) for every accumulator slot acc[frag][slot] this lane holds of the tile (m0, n0), in
// the one order every epilogue sees; valid: the element lies inside m x n
template <typename T, typename F>
__device__ __forceinline__ void stat_tile_for_each(int64_t m0, int64_t n0, int64_t m, int64_t n, F&& f) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  if constexpr (sizeof(T) == 4) {
    const int64_t col = n0 + wn + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      f(row < m && col < n, row, col, 0, r);
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
          f(row < m && col < n, row, col, 2 * i + j, r);
        }
      }
  }
}

// C = A (m x k) B (k x n) tile by tile on a persistent grid (tile t goes to workgroup t mod grid), every element
// handed to the epilogue and nothing stored
template <typename T, typename Epi>
__global__ void __launch_bounds__(256)
valstat_product_kernel(const T* __restrict__ A, const T* __restrict__ B, const int32_t* __restrict__ perm, int64_t m,
                       int64_t n, int64_t k, const typename Epi::Args args) {
  __shared__ typename StatTile<T>::StageA As;
  __shared__ typename StatTile<T>::StageB Bs;

  Epi epi;
  epi.begin(args);

  const int64_t tiles_n = (n + kBN - 1) / kBN, tiles = (m + kBM - 1) / kBM * tiles_n;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t m0 = (t / tiles_n) * kBM, n0 = (t % tiles_n) * kBN;
    typename StatTile<T>::Frag acc[StatTile<T>::kFrags];
    stat_tile_accumulate<T>(A, B, perm, m, n, k, m0, n0, As, Bs, acc);
    stat_tile_for_each<T>(m0, n0, m, n, [&](bool valid, int64_t row, int64_t col, int i, int r) {
      epi.take(args, valid, row, col, acc[i][r]);
    });
  }
  epi.finish(args);
}

// ------------------------------------------------------------------------------------------------ the records
// A record R is plain data of whole 8-byte words with clear() (the neutral element) and fold(const R&).  Threads fold
// by a fixed tree, so the same inputs give the same bits.

// lane 0 <- the wavefront's 64 records
template <typename R>
__device__ __forceinline__ void stat_fold_wave(R& r) {
  static_assert(sizeof(R) % 8 == 0 && std::is_trivially_copyable<R>::value, "a record is shuffled as 8-byte words");
  constexpr int kWords = sizeof(R) / 8;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    unsigned long long w[kWords];
    __builtin_memcpy(w, &r, sizeof(R));
#pragma unroll
    for (int i = 0; i < kWords; ++i) w[i] = __shfl_down(w[i], off);
    R o;
    __builtin_memcpy(&o, w, sizeof(R));
    r.fold(o);
  }
}

// *dst <- the workgroup's 256 records (thread 0 writes): each wavefront's fold through LDS, then in wave order
template <typename R>
__device__ __forceinline__ void stat_fold_group(R& r, R* dst) {
  __shared__ R waves[4];
  stat_fold_wave(r);
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    R t = waves[0];
    for (int w = 1; w < 4; ++w) t.fold(waves[w]);
    *dst = t;
  }
}

// *result <- the partial records folded in index order (one wavefront); Slot: R, or R padded to its workspace slot
template <typename R, typename Slot>
__global__ void __launch_bounds__(64) stat_fold_kernel(const Slot* __restrict__ partials, int count, R* result) {
  R r;
  r.clear();
  for (int i = threadIdx.x; i < count; i += 64) r.fold(partials[i]);
  stat_fold_wave(r);
  if (threadIdx.x == 0) *result = r;
}

// ------------------------------------------------------------------------------------------------ the moments
// a partial or the result of the two record epilogues (ndmps::kValstatRecordBytes)
struct Record {
  double s0, s1;     // moments: sum v, sum v^2            error: sum (v - y)^2, sum y^2
  double lo;         // moments: min                       error: unused
  double hi0, hi1;   // moments: max, unused               error: max |v - y|, max y
  long long c0, c1;  // voxels, NaN among them (moments: v; error: v - y)
  long long c2;      // moments: voxels inside the clip range (the ones behind the four statistics)

  __device__ __forceinline__ void clear() {
    s0 = s1 = 0.0;
    lo = INFINITY;
    hi0 = hi1 = -INFINITY;
    c0 = c1 = c2 = 0;
  }
  __device__ __forceinline__ void fold(const Record& b) {
    s0 += b.s0;
    s1 += b.s1;
    lo = fmin(lo, b.lo);
    hi0 = fmax(hi0, b.hi0);
    hi1 = fmax(hi1, b.hi1);
    c0 += b.c0;
    c1 += b.c1;
    c2 += b.c2;
  }
};
static_assert(sizeof(Record) == ndmps::kValstatRecordBytes, "record layout");

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
  __device__ __forceinline__ void begin(const Args&) { r.clear(); }
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
  __device__ __forceinline__ void finish(const Args& a) { stat_fold_group(r, &a.partials[blockIdx.x]); }
};

// ---- order-preserving keys (the extremes along axes, the place of the global extreme, the extremes per label)
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

// ---- the histogram epilogue's two pieces
// The place of v in the ascending table e[0 .. B]: bin b takes e[b] <= v < e[b + 1], the last bin is closed on the
// right; B: below, B + 1: above, B + 2: NaN.  A binary search in the table, so it is exact for the computed v.
template <typename T>
__device__ __forceinline__ int valstat_bin(const T* e, int B, T v) {
  int bin;
  if (v != v) {
    bin = B + 2;
  } else if (v < e[0]) {
    bin = B;
  } else if (v > e[B]) {
    bin = B + 1;
  } else {
    int lo = 0, hi = B + 1;  // e[lo] <= v, and hi == B + 1 or v < e[hi]: the largest b with e[b] <= v
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (e[mid] <= v) lo = mid; else hi = mid;
    }
    bin = lo == B ? B - 1 : lo;  // v == e[B]: the last bin is closed on the right
  }
  return bin;
}

// cnt[bin] += 1 for every lane with bin >= 0, called by the whole wavefront: the lanes that share the first lane's bin
// make one add; the others add for themselves
__device__ __forceinline__ void valstat_add_folded(unsigned int* cnt, int bin) {
  const int first = __builtin_amdgcn_readfirstlane(bin);
  const bool same = bin == first;
  const unsigned long long mask = __ballot(same);
  if (same) {
    if (first >= 0 && (int)(threadIdx.x & 63) == __ffsll((long long)mask) - 1) atomicAdd(&cnt[first], (unsigned int)__popcll(mask));
  } else if (bin >= 0) {
    atomicAdd(&cnt[bin], 1u);
  }
}

// out (rows x cols) <- the columns perm[0], perm[1], ... of in (chain.hip's gather_cols_kernel in the element type);
// a perm entry outside [0, cols) gives a zero column
template <typename T>
__global__ void __launch_bounds__(256)
valstat_gather_cols_kernel(const T* __restrict__ in, T* __restrict__ out, int64_t rows, int64_t cols,
                           const int32_t* __restrict__ perm) {
  const int64_t total = rows * cols;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t p = perm[e % cols];
    out[e] = (p >= 0 && p < cols) ? in[(e / cols) * cols + p] : (T)0;
  }
}

template <typename T>
__global__ void valstat_unit_kernel(T* p) { *p = (T)1; }

// ------------------------------------------------------------------------------------------------ host
struct ErrorTables {
  const void* ref;
  const int64_t* row_off;
  const int64_t* col_off;
  const int32_t* col_perm;
  int64_t n_cols;
};

// The argument check of every entry, before its first launch (chain_check's conditions on the chain itself).
template <typename T>
int valstat_check(const ChainStatsPlan& sp, const int64_t* dims, const int64_t* bonds, const T* const* cores,
                  const void* d_ws, int64_t ws_bytes, const ErrorTables* err) {
  const ndmps::ChainPlan& p = sp.chain;
  const int L = p.L;
  NDMPS_REQUIRE(cores, "bad valstat argument");
  NDMPS_REQUIRE(bonds[0] == 1 && bonds[L] == 1, "open boundary bonds must be 1");
  for (int i = 0; i < L; ++i)
    NDMPS_REQUIRE(dims[i] >= 1 && cores[i], "dims[%d] must be positive and core %d non-NULL", i, i);
  int64_t left = 1;
  for (int i = 0; i < L; ++i) {
    left *= dims[i];
    NDMPS_REQUIRE(bonds[i + 1] >= 1 && bonds[i + 1] <= left && bonds[i + 1] <= p.numel / left,
                  "bond %d = %lld exceeds min(%lld, %lld), the rank any unfolding can have", i + 1,
                  (long long)bonds[i + 1], (long long)left, (long long)(p.numel / left));
  }
  if (!d_ws || ws_bytes < sp.total_bytes) {
    ndmps::set_error("valstat workspace too small: %lld < %lld", (long long)ws_bytes, (long long)sp.total_bytes);
    return NDMPS_EWORKSPACE;
  }
  NDMPS_REQUIRE(((uintptr_t)d_ws & 255) == 0, "valstat workspace must be 256-byte aligned");
  if (err) {
    NDMPS_REQUIRE(err->ref && err->row_off && err->col_off && err->col_perm, "NULL original or offset table");
    NDMPS_REQUIRE(err->n_cols == sp.reduced.n, "offset tables are for %lld columns, the last product has %lld",
                  (long long)err->n_cols, (long long)sp.reduced.n);
  }
  return NDMPS_OK;
}

struct Operands {
  const void *A, *B;
  const int32_t* perm;  // column order of B inside the product kernel, NULL: as stored
};

// Runs every product before the last as run_chain does and returns the operands of the last one.  gather: the
// columns of its right operand are wanted in the order col_perm (the error epilogue).
template <typename T>
int valstat_run_chain(const ChainStatsPlan& sp, const T* const* cores, void* d_ws, const int32_t* col_perm, hipStream_t s,
                      Operands* ops) {
  const ndmps::ChainPlan& p = sp.chain;
  char* ws = (char*)d_ws;
  auto at = [&](int id) -> T* {
    switch (id) {
      case ndmps::kChainLeft: return (T*)(ws + p.off_left);
      case ndmps::kChainLeft2: return (T*)(ws + sp.off_left2);
      case ndmps::kChainTail0: return (T*)(ws + p.off_tail0);
      case ndmps::kChainTail1: return (T*)(ws + p.off_tail1);
      case ndmps::kChainUnit: return (T*)(ws + sp.off_unit);
      default: return const_cast<T*>(cores[id]);
    }
  };
  for (size_t i = 0; i + 1 < p.products.size(); ++i) {
    const ChainProduct& q = p.products[i];
    NDMPS_REQUIRE(q.c != ndmps::kChainOut && q.c != ndmps::kChainNone, "internal: a product of the stats plan has no buffer");
    NDMPS_TRY(gemm_T(0, q.m, q.n, q.k, at(q.a), at(q.b), q.n, at(q.c), nullptr, 0, s));
  }
  const ChainProduct& q = sp.reduced;
  NDMPS_REQUIRE(q.c == ndmps::kChainNone, "internal: the reduced product has a destination");
  if (q.a == ndmps::kChainUnit) {
    hipLaunchKernelGGL(valstat_unit_kernel<T>, dim3(1), dim3(1), 0, s, at(q.a));
    NDMPS_LAUNCH_CHECK();
  }
  ops->A = at(q.a);
  ops->B = at(q.b);
  ops->perm = col_perm;
  if (col_perm && q.spare != ndmps::kChainNone) {  // where the decode gathers: into the tail buffer that does not hold R
    hipLaunchKernelGGL(valstat_gather_cols_kernel<T>, dim3(grid1d(q.k * q.n)), dim3(256), 0, s, at(q.b), at(q.spare), q.k,
                       q.n, col_perm);
    NDMPS_LAUNCH_CHECK();
    ops->B = at(q.spare);
    ops->perm = nullptr;
  }
  return NDMPS_OK;
}

inline int64_t stat_tiles(const ChainProduct& q) { return ceil_div(q.m, kBM) * ceil_div(q.n, kBN); }
inline int valstat_grid(const ChainProduct& q) { return (int)std::min<int64_t>(stat_tiles(q), ndmps::kValstatMaxGroups); }

// One chain of a call, after the entry's own NDMPS_REQUIREs: check() is the argument check on the chain's part of the
// workspace, run() every product before the last.  Then q is the reduced product, ops its operands, grid its
// launch, and partials / result the record slots of the chain's plan.  It refers to the caller's plan (a
// ChainStatsPlan of its own, or one half of a ChainPairPlan), which has to outlive it.
template <typename T>
struct StatCall {
  const ChainStatsPlan& sp;
  const ChainProduct& q;
  const T* const* cores;
  char* ws;
  hipStream_t s;
  int grid;
  Operands ops{};

  StatCall(const ChainStatsPlan& plan, const T* const* h_cores, void* d_ws, ndmps_stream_t stream)
      : sp(plan), q(plan.reduced), cores(h_cores), ws((char*)d_ws), s((hipStream_t)stream), grid(valstat_grid(plan.reduced)) {}
  int check(const int64_t* dims, const int64_t* bonds, int64_t ws_bytes, const ErrorTables* tables) const {
    return valstat_check(sp, dims, bonds, cores, ws, ws_bytes, tables);
  }
  int run(const int32_t* col_perm) { return valstat_run_chain(sp, cores, ws, col_perm, s, &ops); }
  template <typename R>
  R* partials() const { return (R*)(ws + sp.off_partials); }
  template <typename R>
  R* result() const { return (R*)(ws + sp.off_result); }
};

// the single-chain product with the epilogue Epi
template <typename T, typename Epi>
int stat_launch(const ChainProduct& q, const Operands& ops, const typename Epi::Args& args, int grid, size_t lds, hipStream_t s) {
  hipLaunchKernelGGL((valstat_product_kernel<T, Epi>), dim3(grid), dim3(256), lds, s, (const T*)ops.A, (const T*)ops.B,
                     ops.perm, q.m, q.n, q.k, args);
  NDMPS_LAUNCH_CHECK();
  return NDMPS_OK;
}

// a workgroup counts in 32 bits until its one flush
inline int stat_counters_fit(int64_t tiles, int grid, const char* what) {
  NDMPS_REQUIRE(ceil_div(tiles, grid) * kBM * kBN < (int64_t)UINT32_MAX, "%s: volume too large for 32-bit counters per workgroup",
                what);
  return NDMPS_OK;
}

// the edge table of a histogram; what: "histogram: edges", "joint histogram: edges of a"
template <typename T>
int stat_edges_ok(const T* e, int bins, const char* what) {
  for (int i = 0; i <= bins; ++i)
    NDMPS_REQUIRE(e[i] == e[i] && (i == 0 || e[i] >= e[i - 1]), "%s must be ascending and not NaN (edge %d)", what, i);
  return NDMPS_OK;
}

// *result <- the partial records of `grid` workgroups in index order, on the device
template <typename R, typename Slot>
int stat_fold(const Slot* partials, int grid, R* result, hipStream_t s) {
  hipLaunchKernelGGL((stat_fold_kernel<R, Slot>), dim3(1), dim3(64), 0, s, partials, grid, result);
  NDMPS_LAUNCH_CHECK();
  return NDMPS_OK;
}
// the same, and *host <- the result: the one synchronisation of a record entry
template <typename R, typename Slot>
int stat_fetch_record(const Slot* partials, int grid, R* result, R* host, hipStream_t s) {
  NDMPS_TRY(stat_fold<R>(partials, grid, result, s));
  NDMPS_CHECK_HIP(hipMemcpyAsync(host, result, sizeof(R), hipMemcpyDeviceToHost, s));
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));
  return NDMPS_OK;
}

}  // namespace
