// The plan of a dense product (gemm.hip, gemm_bf16.hip): which tile a shape takes, whether its operands are staged
// in quads, the grid, and for bf16 the transposed copy and the fold into several launches.  Pure host arithmetic in
// plain C++17 -- no HIP call, no environment, no globals -- so it compiles and is tested without a GPU; every dense
// entry (ndmps_sgemm, ndmps_dgemm, their _batched and _indexed twins, ndmps_gemm_bf16) launches by it and
// ndmps_gemm_plan_query answers from it.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace ndmps {

enum class GemmElem : int { F32 = 0, BF16 = 1, F64 = 2 };

constexpr int kGemmBK = 16;                  // k-tile of the fp32 / fp64 kernels
constexpr int kGemmThreads = 256;
constexpr int kGemmBf16Tile = 128;           // BM = BN of the bf16 kernel
constexpr int64_t kGemmBf16MaxRowTiles = 65535;  // grid.y of one bf16 launch

struct GemmPlan {
  int bm = 0, bn = 0;          // block tile
  int vec = 0;                 // the launcher's test: whole aligned quads in every operand row (fp32 / fp64)
  int va = 0, vb = 0;          // what the kernel stages in quads: vec and a multiple of 4 elements per thread
  int64_t grid_x = 0, grid_y = 0;
  int guarded = 0;             // every tile through the guarded fetch
  // row / column blocks whose full k-tiles come by the straight-line fetch: gemm_body's inner_a / inner_b counted over
  // the grid, for ndmps_gemm_plan_query (no launch depends on them)
  int64_t inner_a = 0, inner_b = 0;
  int vec_in = 0, vec_out = 0, transposes = 0;  // bf16: 16-byte loads / stores, a (k, n) right operand copied first
  int64_t launches = 0;        // 0: empty product, nothing is launched
};

inline int64_t gemm_ceil_div(int64_t x, int64_t a) { return (x + a - 1) / a; }

// why a product is refused before anything is launched, or NULL.  Pointers are the entries' business.
inline const char* gemm_refusal(GemmElem elem, int transA, int transB, int64_t m, int64_t n, int64_t k, int64_t lda,
                                int64_t ldb, int64_t ldc) {
  if (elem == GemmElem::BF16) {
    if (transA) return "the bf16 product takes no transposed left operand";
    if (!(m > 0 && n > 0 && k > 0)) return "bad GEMM extents";
    if (!(lda >= k && ldc >= n && ldb >= (transB ? k : n))) return "leading dimension smaller than a row";
    if (!(gemm_ceil_div(m, kGemmBf16Tile) < 65536 * 32768LL)) return "too many row tiles";
    return nullptr;
  }
  if (!(m >= 0 && n >= 0 && k >= 0)) return "negative GEMM extent";
  if (!(lda >= (transA ? m : k) && ldb >= (transB ? k : n) && ldc >= n)) return "leading dimension too small";
  if (!(gemm_ceil_div(n, 16) < 65536)) return "GEMM n exceeds grid.y";
  if (!(gemm_ceil_div(m, 32) < 2147483647LL)) return "GEMM m exceeds grid.x";
  return nullptr;
}

// the block tile of a shape; indexed: the table-addressed entries have no narrow tile
inline void gemm_tile(GemmElem elem, int64_t m, int64_t n, bool indexed, int* bm, int* bn) {
  if (elem == GemmElem::F64) {
    if (n <= 16) *bm = 64, *bn = 16;
    else if (n <= 32 || m <= 32) *bm = 32, *bn = 32;
    else *bm = 64, *bn = 64;
  } else if (elem == GemmElem::F32) {
    if (n <= 32 && !indexed) *bm = 128, *bn = 32;
    else if (n <= 64 || m <= 64) *bm = 64, *bn = 64;
    else *bm = 128, *bn = 128;
  } else {
    *bm = *bn = kGemmBf16Tile;
  }
}

// tile, staging and grid of an fp32 / fp64 product once the launcher's vector test is known
inline GemmPlan gemm_plan_tiled(GemmElem elem, int64_t m, int64_t n, bool indexed, bool vec, bool guarded) {
  GemmPlan p;
  p.guarded = guarded ? 1 : 0;
  if (m == 0 || n == 0) return p;
  gemm_tile(elem, m, n, indexed, &p.bm, &p.bn);
  p.vec = vec ? 1 : 0;
  // elements per thread and k-tile: a thread that holds no whole quad of an operand stages it element by element
  p.va = vec && (p.bm * kGemmBK / kGemmThreads) % 4 == 0;
  p.vb = vec && (p.bn * kGemmBK / kGemmThreads) % 4 == 0;
  p.grid_x = gemm_ceil_div(m, p.bm);
  p.grid_y = gemm_ceil_div(n, p.bn);
  p.inner_a = p.va && !guarded ? m / p.bm : 0;
  p.inner_b = p.vb && !guarded ? n / p.bn : 0;
  p.launches = 1;
  return p;
}

// mis_a, mis_b, mis_c: the operands' addresses modulo 64 (a batch: the bitwise OR over its members; bf16 with a
// (k, n) right operand: mis_b is the workspace's, which is what the product kernel reads).  The shape has passed
// gemm_refusal.
inline GemmPlan gemm_plan(GemmElem elem, int transA, int transB, int64_t m, int64_t n, int64_t k, int64_t lda, int64_t ldb,
                          int64_t ldc, int64_t mis_a, int64_t mis_b, int64_t mis_c, bool guarded) {
  if (elem == GemmElem::BF16) {
    GemmPlan p;
    p.bm = p.bn = kGemmBf16Tile;
    p.transposes = transB ? 0 : 1;
    const int64_t ldbt = transB ? ldb : k;
    p.vec_in = lda % 8 == 0 && ldbt % 8 == 0 && mis_a % 16 == 0 && mis_b % 16 == 0;
    p.vec_out = ldc % 8 == 0 && mis_c % 16 == 0;
    const int64_t row_tiles = gemm_ceil_div(m, kGemmBf16Tile);
    p.grid_x = gemm_ceil_div(n, kGemmBf16Tile);
    p.grid_y = std::min(row_tiles, kGemmBf16MaxRowTiles);  // of the first launch
    p.launches = gemm_ceil_div(row_tiles, kGemmBf16MaxRowTiles);
    return p;
  }
  // vector path: whole quads are either inside or outside every bound, and 4-element aligned
  const int64_t al = elem == GemmElem::F64 ? 32 : 16;
  const bool vec = lda % 4 == 0 && ldb % 4 == 0 && k % 4 == 0 && (!transA || m % 4 == 0) && (transB || n % 4 == 0) &&
                   mis_a % al == 0 && mis_b % al == 0;
  return gemm_plan_tiled(elem, m, n, false, vec, guarded);
}

// C = A B with table-addressed A and / or C (fp32): a_tables: A comes through offset tables, whose quads the caller
// vouches for with a_vec4
inline GemmPlan gemm_plan_indexed(int64_t m, int64_t n, int64_t k, int64_t lda, int64_t ldb, bool a_tables, bool a_vec4,
                                  int64_t mis_a, int64_t mis_b, bool guarded) {
  const bool vec = ldb % 4 == 0 && k % 4 == 0 && n % 4 == 0 && mis_a % 16 == 0 && mis_b % 16 == 0 &&
                   (a_tables ? a_vec4 : lda % 4 == 0);
  return gemm_plan_tiled(GemmElem::F32, m, n, true, vec, guarded);
}

}  // namespace ndmps
