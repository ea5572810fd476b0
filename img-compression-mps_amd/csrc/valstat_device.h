// What valstat.hip (one chain, reduced) and pairstat.hip (two chains, reduced together) both need: the argument check
// of a chain, the products before the last one, the operands of the last one, the tile and grid of the reducing
// product, and the two pieces of the histogram epilogue (the bin search and the fold of the lanes that share the first
// lane's bin).  Internal linkage, as typed.h: each translation unit gets its own copy.
#pragma once
#include <algorithm>

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

inline int valstat_grid(const ChainProduct& q) {
  const int64_t tiles = ceil_div(q.m, kBM) * ceil_div(q.n, kBN);
  return (int)std::min<int64_t>(tiles, ndmps::kValstatMaxGroups);
}

}  // namespace
