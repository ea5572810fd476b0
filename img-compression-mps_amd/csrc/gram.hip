// Gram matrices G = A^T A on the fp64 matrix cores: the small-side Gram of the per-site SVD.
//
//   ndmps_gram_f32 / _bf16 / _f64  : one matrix, A (m, n) row-major in fp32, bf16 or fp64 storage, G fp64
//   ndmps_gram_indexed_f32         : A read through (row, column) offset tables, G stored through a column permutation
//   ndmps_gram_batched_*           : a lockstep group's matrices of one shape in one launch
//   ndmps_gram_*workspace_bytes    : the size queries
//
// fp32 and bf16 elements are converted to fp64 before they meet v_mfma_f64_16x16x4_f64: exact products, one rounding
// per add.  Every route cuts the rows into slabs, writes one partial tile per (tile, slab) into the caller's
// workspace and sums a tile's slabs in a fixed order: G is reproducible bit for bit for a given (batch, m, n).
//
// The file is in three parts: the kernels of each route, then GramPlan -- the ONE place that decides which route a
// call takes, with which geometry, and how large its workspace is -- then the entry points, each of which makes the
// plan, checks its arguments and workspace against the plan, and runs it.
#include <stdlib.h>

#include <algorithm>
#include <mutex>
#include <type_traits>

#include "common.h"

namespace {

using ndmps::f64x4;
using ndmps::load4_as_f32;
using ndmps::load4_stream_f32;

// tile `tile` of the upper triangle of n_tiles_1d x n_tiles_1d tiles, numbered row by row from the diagonal on:
// (ti, tj), ti <= tj
__device__ __forceinline__ void upper_tile(int tile, int n_tiles_1d, int& ti, int& tj) {
  ti = 0;
  while (tile >= n_tiles_1d - ti) {
    tile -= n_tiles_1d - ti;
    ++ti;
  }
  tj = ti + tile;
}

// element (r, c) of the upper triangle and its mirror image: G comes out exactly symmetric.  perm (or NULL): the
// element goes to (perm[r], perm[c])
__device__ __forceinline__ void store_mirrored(double* __restrict__ G, int64_t n, int64_t r, int64_t c, double s,
                                               const int32_t* __restrict__ perm) {
  const int64_t pr = perm ? perm[r] : r, pc = perm ? perm[c] : c;
  G[pr * n + pc] = s;
  G[pc * n + pr] = s;
}

// ----------------------------------------------------------------------------------
// Any shape, any storage type: A (m, n) row-major, G fp64.
// Lane l of a wave reads A[r + (l>>4)][c + (l&15)] -- straight row-major segments, no
// transposition -- converts to f64 and feeds v_mfma_f64_16x16x4_f64 as both operands.
// A workgroup owns one (T*16)^2 tile of the upper triangle over a slab of rows; its 4
// waves interleave 4-row k-steps and fold their accumulators through LDS; the slab result
// goes to a partial buffer, reduced in fixed order (deterministic) by tile_reduce_kernel.
// ----------------------------------------------------------------------------------
template <int T, typename TIN>
__global__ void __launch_bounds__(256, 2)
gram_partial_kernel(const TIN* __restrict__ A, int64_t m, int64_t n, int64_t lda,
                    double* __restrict__ partial, int n_tiles_1d, int64_t rows_per_slab) {
  constexpr int TS = 16 * T;  // tile edge
  __shared__ double red[TS][TS + 1];

  int ti, tj;
  upper_tile(blockIdx.x, n_tiles_1d, ti, tj);
  const int64_t i0 = (int64_t)ti * TS, j0 = (int64_t)tj * TS;
  const int64_t slab = blockIdx.y;
  const int64_t r_begin = slab * rows_per_slab;
  const int64_t r_end = min(m, r_begin + rows_per_slab);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane >> 4, lc = lane & 15;

  f64x4 acc[T][T];
#pragma unroll
  for (int a = 0; a < T; ++a)
#pragma unroll
    for (int b = 0; b < T; ++b) acc[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};

  for (int64_t r = r_begin + 4 * wave; r < r_end; r += 16) {
    const int64_t row = r + lr;
    const bool row_ok = row < r_end;
    double av[T], bv[T];
#pragma unroll
    for (int a = 0; a < T; ++a) {
      const int64_t ca = i0 + 16 * a + lc;
      const int64_t cb = j0 + 16 * a + lc;
      av[a] = (row_ok && ca < n) ? ndmps::to_f64(A[row * lda + ca]) : 0.0;
      bv[a] = (row_ok && cb < n) ? ndmps::to_f64(A[row * lda + cb]) : 0.0;
    }
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
      for (int b = 0; b < T; ++b)
        acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
  }

  // fold the 4 waves through LDS, one after the other (fixed order)
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int a = 0; a < T; ++a)
#pragma unroll
        for (int b = 0; b < T; ++b)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const int rr = 16 * a + lr + 4 * reg, cc = 16 * b + lc;
            if (w == 0) red[rr][cc] = acc[a][b][reg];
            else red[rr][cc] += acc[a][b][reg];
          }
    }
    __syncthreads();
  }
  double* out = partial + ((int64_t)slab * gridDim.x + blockIdx.x) * (TS * TS);
  for (int e = tid; e < TS * TS; e += 256) out[e] = red[e / TS][e % TS];
}

// Slab reduce, fixed summation order (deterministic), in up to two levels so that no thread
// walks more than ~32 slabs: grid (n_tiles, TS*TS/256, n_groups).  Group g sums slabs
// [g*per_group, (g+1)*per_group); `final` writes the (mirrored) tile into G, otherwise the group
// sums go to `out` laid out like a partial buffer with n_groups slabs.
template <int TS>
__global__ void __launch_bounds__(256)
tile_reduce_kernel(const double* __restrict__ partial, int n_slabs, int per_group, int n_tiles_1d,
                   int n_tiles, double* __restrict__ out, double* __restrict__ G, int64_t n, int final,
                   const int32_t* __restrict__ perm = nullptr) {  // perm: element (r, c) goes to (perm[r], perm[c])
  const int e = blockIdx.y * 256 + threadIdx.x;
  if (e >= TS * TS) return;
  const int s0 = blockIdx.z * per_group, s1 = min(n_slabs, s0 + per_group);
  const double* src = partial + (int64_t)blockIdx.x * (TS * TS) + e;
  const int64_t slab_stride = (int64_t)n_tiles * (TS * TS);
  double s = 0.0;
  int sl = s0;
  for (; sl + 4 <= s1; sl += 4) {
    const double v0 = src[(sl + 0) * slab_stride], v1 = src[(sl + 1) * slab_stride];
    const double v2 = src[(sl + 2) * slab_stride], v3 = src[(sl + 3) * slab_stride];
    s = (((s + v0) + v1) + v2) + v3;
  }
  for (; sl < s1; ++sl) s += src[sl * slab_stride];
  if (!final) {
    out[((int64_t)blockIdx.z * n_tiles + blockIdx.x) * (TS * TS) + e] = s;
    return;
  }
  int ti, tj;
  upper_tile(blockIdx.x, n_tiles_1d, ti, tj);
  const int64_t r = (int64_t)ti * TS + e / TS, c = (int64_t)tj * TS + e % TS;
  if (r < n && c < n && (ti != tj || c >= r)) {  // diagonal tiles: upper part mirrored -> exactly symmetric
    store_mirrored(G, n, r, c, s, perm);
  }
}

constexpr int kReduceGroup = 16;

template <int TS>
int launch_tile_reduce(double* partial, int n_slabs, int n_tiles_1d, int n_tiles, double* G, int64_t n,
                       hipStream_t s, const int32_t* perm = nullptr) {
  const unsigned ey = (TS * TS + 255) / 256;
  if (n_slabs <= 2 * kReduceGroup) {
    hipLaunchKernelGGL(tile_reduce_kernel<TS>, dim3(n_tiles, ey, 1), dim3(256), 0, s, partial, n_slabs, n_slabs,
                       n_tiles_1d, n_tiles, (double*)nullptr, G, n, 1, perm);
  } else {
    // level 1 writes its group sums behind the slabs (the workspace has room for them)
    const int groups = (n_slabs + kReduceGroup - 1) / kReduceGroup;
    double* lvl = partial + (int64_t)n_slabs * n_tiles * (TS * TS);
    hipLaunchKernelGGL(tile_reduce_kernel<TS>, dim3(n_tiles, ey, groups), dim3(256), 0, s, partial, n_slabs,
                       kReduceGroup, n_tiles_1d, n_tiles, lvl, G, n, 0);
    hipLaunchKernelGGL(tile_reduce_kernel<TS>, dim3(n_tiles, ey, 1), dim3(256), 0, s, lvl, groups, groups,
                       n_tiles_1d, n_tiles, (double*)nullptr, G, n, 1, perm);
  }
  NDMPS_LAUNCH_CHECK();
  return NDMPS_OK;
}

// ----------------------------------------------------------------------------------
// Gram for 64 <= n < 128 (and at least eight 32-row chunks): a workgroup owns a 64 x 64 tile of the
// upper triangle over a slab of rows; 32-row chunks of the two 64-column panels are staged in LDS
// (16-byte global loads, each element of A fetched once per tile instead of once per lane), the
// next chunk is prefetched into registers while the four waves (2 x 2, 32 x 32 each, four f64 MFMA
// accumulators) consume the current one.  LDS rows are padded by 16 floats: a fragment read (4 rows
// x 16 columns) is conflict-free.  From 128 columns on gram128_kernel below takes over.
// ----------------------------------------------------------------------------------
constexpr int GW_KB = 32;    // rows per staged chunk (gram128_kernel's too)

// row_off / col_off (both or neither): element (r, c) of A at A[row_off[r] + col_off[c]] instead of A[r lda + c] --
// the matrix is the C-order volume read through the index permutation (see GemmIndex); with vec_ok every aligned
// group of four columns has consecutive offsets.
template <typename TIN>
__device__ __forceinline__ void gram_wide_body(const TIN* __restrict__ A, int64_t m, int64_t n, int64_t lda,
                                               double* __restrict__ out, int n_tiles_1d, int64_t rows_per_slab, int vec_ok,
                                               const int64_t* __restrict__ row_off, const int64_t* __restrict__ col_off,
                                               int tile_id, int slab_id) {
  constexpr int GW_TS = 64;            // tile edge
  constexpr int GW_LD = GW_TS + 16;
  constexpr int NT = GW_TS / 32;       // MFMA tiles per wave and direction
  constexpr int SUB = GW_TS / 2;       // wave sub-tile edge
  constexpr int QPR = GW_TS / 4;       // float4 per staged row
  constexpr int VPT = GW_KB * QPR / 256;  // float4 per thread and panel
  __shared__ float Ai[GW_KB][GW_LD];
  __shared__ float Aj[GW_KB][GW_LD];

  int ti, tj;
  upper_tile(tile_id, n_tiles_1d, ti, tj);
  const bool diag = ti == tj;
  const int64_t i0 = (int64_t)ti * GW_TS, j0 = (int64_t)tj * GW_TS;
  const int64_t r_begin = (int64_t)slab_id * rows_per_slab;
  const int64_t r_end = min(m, r_begin + rows_per_slab);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int lr = lane >> 4, lc = lane & 15;

  f64x4 acc[NT][NT];
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b) acc[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};

  // staging map: GW_KB rows x QPR float4 per panel, VPT per thread
  float4 pi[VPT], pj[VPT];
  auto fetch = [&](int64_t r0) {
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
      const int e = tid + 256 * v;
      const int rr = e / QPR, c4 = (e % QPR) * 4;
      const int64_t row = r0 + rr;
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
      if (row < r_end && row_off) {  // gathered: offsets additive in (row, column); vec_ok guaranteed by the host
        const TIN* base = A + row_off[row];
        if (i0 + c4 + 3 < n) x = load4_as_f32(base + col_off[i0 + c4]);
        if (!diag && j0 + c4 + 3 < n) y = load4_as_f32(base + col_off[j0 + c4]);
      } else if (row < r_end) {
        const TIN* base = A + row * lda;
        if (vec_ok && i0 + c4 + 3 < n) x = load4_as_f32(base + i0 + c4);
        else {
          if (i0 + c4 + 0 < n) x.x = (float)base[i0 + c4 + 0];
          if (i0 + c4 + 1 < n) x.y = (float)base[i0 + c4 + 1];
          if (i0 + c4 + 2 < n) x.z = (float)base[i0 + c4 + 2];
          if (i0 + c4 + 3 < n) x.w = (float)base[i0 + c4 + 3];
        }
        if (!diag) {
          if (vec_ok && j0 + c4 + 3 < n) y = load4_as_f32(base + j0 + c4);
          else {
            if (j0 + c4 + 0 < n) y.x = (float)base[j0 + c4 + 0];
            if (j0 + c4 + 1 < n) y.y = (float)base[j0 + c4 + 1];
            if (j0 + c4 + 2 < n) y.z = (float)base[j0 + c4 + 2];
            if (j0 + c4 + 3 < n) y.w = (float)base[j0 + c4 + 3];
          }
        }
      }
      pi[v] = x;
      pj[v] = y;
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
      const int e = tid + 256 * v;
      const int rr = e / QPR, c4 = (e % QPR) * 4;
      *reinterpret_cast<float4*>(&Ai[rr][c4]) = pi[v];
      if (!diag) *reinterpret_cast<float4*>(&Aj[rr][c4]) = pj[v];
    }
  };

  fetch(r_begin);
  for (int64_t r0 = r_begin; r0 < r_end; r0 += GW_KB) {
    __syncthreads();  // previous chunk fully consumed
    stash();
    __syncthreads();
    if (r0 + GW_KB < r_end) fetch(r0 + GW_KB);  // prefetch under the MFMAs
    const float (*Bj)[GW_LD] = diag ? Ai : Aj;
#pragma unroll
    for (int k0 = 0; k0 < GW_KB; k0 += 4) {
      double av[NT], bv[NT];
#pragma unroll
      for (int a = 0; a < NT; ++a) {
        av[a] = (double)Ai[k0 + lr][wr * SUB + 16 * a + lc];
        bv[a] = (double)Bj[k0 + lr][wc * SUB + 16 * a + lc];
      }
#pragma unroll
      for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
    }
  }

#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int rr = wr * SUB + 16 * a + lr + 4 * reg, cc = wc * SUB + 16 * b + lc;
        out[rr * GW_TS + cc] = acc[a][b][reg];
      }
}

template <typename TIN>
__global__ void __launch_bounds__(256, 2)
gram_wide_kernel(const TIN* __restrict__ A, int64_t m, int64_t n, int64_t lda,
                 double* __restrict__ partial, int n_tiles_1d, int64_t rows_per_slab, int vec_ok,
                 const int64_t* __restrict__ row_off = nullptr, const int64_t* __restrict__ col_off = nullptr) {
  gram_wide_body<TIN>(A, m, n, lda, partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (64 * 64),
                             n_tiles_1d, rows_per_slab, vec_ok, row_off, col_off, blockIdx.x, blockIdx.y);
}

// The same tiles for a whole lockstep group in ONE launch (blockIdx.z = matrix): the 64-column raw Gram of a bond cap
// of 32 (BASELINE configs 2 and 4) went out as one launch per volume, each cut into 512 short slabs to fill the GPU by
// itself (16.8 MB of partial tiles written and read back per 64 MB volume); a group shares the GPU, so slabs are long.
struct GramBatchPtrs {
  const void* a[64];
};
template <typename TIN>
__global__ void __launch_bounds__(256, 4)  // a 64-column Gram is a stream: four workgroups per CU keep more of it in flight
gram_wide_batched_kernel(GramBatchPtrs ptrs, int64_t m, int64_t n, int64_t lda, double* __restrict__ partial, int n_tiles_1d,
                         int64_t rows_per_slab, int vec_ok, const int64_t* __restrict__ row_off,
                         const int64_t* __restrict__ col_off) {
  double* out = partial + (((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (64 * 64);
  gram_wide_body<TIN>(static_cast<const TIN*>(ptrs.a[blockIdx.z]), m, n, lda, out, n_tiles_1d, rows_per_slab, vec_ok,
                             row_off, col_off, blockIdx.x, blockIdx.y);
}
// ----------------------------------------------------------------------------------
// n == 64 exactly (the raw Gram of a bond cap of 32: d chi = 8 x 8 columns, 64 MB per 256^3 volume): a STREAM.
// The tile kernel above stages 32-row chunks in LDS behind two barriers and computes the full 64 x 64 tile (16 MFMAs
// per four rows): 1.26 ms per lockstep group of 32 alone, 2.2 ms inside a step -- 1 TB/s.  Here a wave reads four rows
// with ONE coalesced 16-byte load per lane (lane (i, k) = (lane % 16, lane / 16) takes columns 4i .. 4i + 3 of row
// k) and that float4 IS the four MFMA operands: component a belongs to the column block {4i + a}, so
// v_mfma_f64_16x16x4_f64(x_a, x_b) accumulates G[4i + a][4j + b] -- a column permutation that is undone when the tile is
// written.  Ten MFMAs per four rows (blocks a <= b), no LDS, no barrier in the loop, eight loads in flight per lane
// (offsets of a gathered operand one block further ahead).  The four waves of a workgroup take rows 4w .. 4w + 3 of
// every 16 and add their accumulators in a fixed order at the end; the partial tile has the layout
// tile_reduce_batched_kernel<64> expects.
template <typename TIN, bool GATHER>
__global__ void __launch_bounds__(256, 3)  // three waves per SIMD: one waiting for its loads leaves the MFMA pipe to two
gram64_stream_kernel(GramBatchPtrs ptrs, int64_t m, int64_t lda, double* __restrict__ partial, int64_t rows_per_slab,
                     const int64_t* __restrict__ row_off, const int64_t* __restrict__ col_off) {
  constexpr int U = 8;  // k-steps (of four rows per wave) per block
  const TIN* A = static_cast<const TIN*>(ptrs.a[blockIdx.z]);
  double* out = partial + ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * 4096;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, kk = lane >> 4;
  const int64_t r_begin = (int64_t)blockIdx.y * rows_per_slab;
  const int64_t r_end = min(m, r_begin + rows_per_slab);
  const int64_t n_steps = (r_end - r_begin + 15) / 16;
  const int64_t n_blocks = (n_steps + U - 1) / U;
  const int64_t coff = GATHER ? col_off[4 * li] : 4 * li;
  const int64_t row0 = r_begin + 4 * wave + kk;  // this lane's row at step 0; + 16 per step

  f64x4 acc[10];
#pragma unroll
  for (int q = 0; q < 10; ++q) acc[q] = (f64x4){0.0, 0.0, 0.0, 0.0};
#define NDMPS_GRAM64_STEP(v)                                                                                     \
  {                                                                                                              \
    const double x0 = (double)(v).x, x1 = (double)(v).y, x2 = (double)(v).z, x3 = (double)(v).w;                 \
    NDMPS_GRAM64_MFMAS(x0, x1, x2, x3)                                                                           \
  }
#define NDMPS_GRAM64_MFMAS(x0, x1, x2, x3)                                                                       \
  {                                                                                                              \
    acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, x0, acc[0], 0, 0, 0);                                      \
    acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, x1, acc[1], 0, 0, 0);                                      \
    acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, x2, acc[2], 0, 0, 0);                                      \
    acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, x3, acc[3], 0, 0, 0);                                      \
    acc[4] = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, x1, acc[4], 0, 0, 0);                                      \
    acc[5] = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, x2, acc[5], 0, 0, 0);                                      \
    acc[6] = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, x3, acc[6], 0, 0, 0);                                      \
    acc[7] = __builtin_amdgcn_mfma_f64_16x16x4f64(x2, x2, acc[7], 0, 0, 0);                                      \
    acc[8] = __builtin_amdgcn_mfma_f64_16x16x4f64(x2, x3, acc[8], 0, 0, 0);                                      \
    acc[9] = __builtin_amdgcn_mfma_f64_16x16x4f64(x3, x3, acc[9], 0, 0, 0);                                      \
  }
  // Full blocks (every row of every step exists): straight-line loads -- a load under a branch makes the compiler
  // wait for ALL outstanding loads (s_waitcnt vmcnt(0)) in front of the MFMAs, prefetched ones included.  Blocks
  // fetched ahead beyond the last full one repeat it (valid addresses, never used).
  const int64_t n_full = (r_end - r_begin) / (16 * U);
  if (n_full > 0) {
    // a ring of U loads per lane: step s takes slot s % U and refills it at once with step s + U (its offset -- the row's
    // entry of the table of a gathered operand -- was fetched U steps before that): a constant distance of U steps
    // (80 MFMAs) between a load and its use, no drain at block boundaries
    const int64_t last = n_full * U - 1;  // steps beyond the last full one repeat it (valid addresses, never used)
    auto offset_of = [&](int64_t step) {
      const int64_t row = row0 + 16 * min(step, last);
      return GATHER ? row_off[row] : row * lda;
    };
    float4 ring[U];
    int64_t roff[U];
#pragma unroll
    for (int u = 0; u < U; ++u) roff[u] = offset_of(u);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      ring[u] = load4_stream_f32(A + roff[u] + coff);
      roff[u] = offset_of(U + u);
    }
    auto block = [&](int64_t blk) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        // the step's operands are converted BEFORE its slot is reloaded in place, and nothing moves across steps:
        // left to itself the scheduler hoists the block's eight loads to its top into fresh registers and copies them
        // into the loop-carried ones -- a copy that waits for the load it follows
        const double x0 = (double)ring[u].x, x1 = (double)ring[u].y, x2 = (double)ring[u].z, x3 = (double)ring[u].w;
        __builtin_amdgcn_sched_barrier(0);
        ring[u] = load4_stream_f32(A + roff[u] + coff);   // step (blk + 1) U + u
        roff[u] = offset_of((blk + 2) * U + u);
        NDMPS_GRAM64_MFMAS(x0, x1, x2, x3)
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    // four blocks per trip: at a loop header the compiler waits for EVERY outstanding load (the newest was issued ten
    // MFMAs earlier), once per 32 steps then
    int64_t blk = 0;
    for (; blk + 4 <= n_full; blk += 4) {
      block(blk);
      block(blk + 1);
      block(blk + 2);
      block(blk + 3);
    }
    for (; blk < n_full; ++blk) block(blk);
  }
  // the ragged end of the slab, row by row
  for (int64_t row = row0 + 16 * U * n_full; row < r_end + 16; row += 16) {  // uniform trip count over the wave
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < r_end) v = load4_as_f32(A + (GATHER ? row_off[row] : row * lda) + coff);
    if (__builtin_amdgcn_ballot_w64(row < r_end) != 0) NDMPS_GRAM64_STEP(v)
  }
#undef NDMPS_GRAM64_STEP
#undef NDMPS_GRAM64_MFMAS

  // waves 3, 2, 1 hand their sums to wave 0 through LDS, one after the other (fixed order)
  __shared__ double hand[10 * 256];
#pragma unroll 1
  for (int src = 3; src >= 1; --src) {
    if (wave == src) {
#pragma unroll
      for (int q = 0; q < 10; ++q)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) hand[(q * 4 + reg) * 64 + lane] = acc[q][reg];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int q = 0; q < 10; ++q)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) acc[q][reg] += hand[(q * 4 + reg) * 64 + lane];
    }
    __syncthreads();
  }
  if (wave == 0) {
    // block q = (a, b), a <= b; accumulator element (i, j) = (kk + 4 reg, li) is G[4i + a][4j + b]
    constexpr int qa[10] = {0, 0, 0, 0, 1, 1, 1, 2, 2, 3}, qb[10] = {0, 1, 2, 3, 1, 2, 3, 2, 3, 3};
#pragma unroll
    for (int q = 0; q < 10; ++q)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int r = 4 * (kk + 4 * reg) + qa[q], c = 4 * li + qb[q];
        out[r * 64 + c] = acc[q][reg];
        if (qa[q] != qb[q]) out[c * 64 + r] = acc[q][reg];
      }
  }
}

// G of matrix blockIdx.z: its slabs of tile blockIdx.x summed in order; upper part mirrored; optional un-permutation
template <int TS>
__global__ void __launch_bounds__(256)
tile_reduce_batched_kernel(const double* __restrict__ partial, int n_slabs, int n_tiles_1d, int n_tiles, double* __restrict__ G,
                           int64_t stride_G, int64_t n, const int32_t* __restrict__ perm) {
  const int e = blockIdx.y * 256 + threadIdx.x;
  if (e >= TS * TS) return;
  const double* src = partial + ((int64_t)blockIdx.z * n_slabs * n_tiles + blockIdx.x) * (TS * TS) + e;
  double s = 0.0;
  for (int sl = 0; sl < n_slabs; ++sl) s += src[(int64_t)sl * n_tiles * (TS * TS)];
  int ti, tj;
  upper_tile(blockIdx.x, n_tiles_1d, ti, tj);
  const int64_t r = (int64_t)ti * TS + e / TS, c = (int64_t)tj * TS + e % TS;
  if (r < n && c < n && (ti != tj || c >= r)) {
    store_mirrored(G + (int64_t)blockIdx.z * stride_G, n, r, c, s, perm);
  }
}

// ----------------------------------------------------------------------------------
// Gram for n >= 128, the dominant kernel of the bond-capped sweep (fp64 MFMA bound: 2 m n (n + 1) / 2 flops).
// The tiling of gram_wide_kernel at twice the edge (128 x 128 tiles of the upper triangle x row slabs, 32-row chunks of
// the two column panels in LDS, four waves of 64 x 64), rebuilt around what kept that kernel at 67 % of the
// 78 TFLOP/s this GPU sustains on v_mfma_f64_16x16x4_f64 (tools/scratch/mfma_f64_rate.hip):
//   * the chunks are double-buffered in LDS: the global loads of chunk c + 1 fly under the MFMAs of chunk c
//     and are written to the other buffer afterwards -- ONE barrier per chunk, not two around a stall;
//   * the operands of k-step s + 1 are read from LDS and converted before the MFMAs of step s are issued;
//   * a DIAGONAL tile computes only the 16 x 16 tiles of its upper triangle (36 of 64): wave 0 / wave 3 the
//     ten of a diagonal 64 x 64 block, waves 1 and 2 half of the off-diagonal block each -- 10 MFMAs per step
//     on the critical wave instead of 16; diagonal tiles get 1.6 x longer slabs so all workgroups last alike;
//   * one launch serves a whole batch of matrices (blockIdx.y): the small Grams of later sites fill the GPU
//     and the slabs can be long (fewer partial tiles to write and reduce).
// Partial tile of workgroup id of matrix b: partial[(b slots + id) 128^2 ..], off-diagonal tiles first
// (tile-major, S_off slabs each), then the diagonal ones (S_diag slabs each); gram128_reduce_kernel sums a
// tile's slabs in order (deterministic) and writes it mirrored.
// ----------------------------------------------------------------------------------
constexpr int G128_LD = 128 + 16;                 // padded LDS row (floats): fragment reads are conflict-free
constexpr int G128_PANEL = GW_KB * G128_LD;       // floats per panel and buffer
constexpr size_t kGram128Lds = (size_t)4 * G128_PANEL * sizeof(float);  // 2 buffers x 2 panels = 73.7 KB
constexpr int kGram128MaxBatch = 48;              // matrices per launch (pointers travel as kernel arguments)

struct Gram128Geom {
  int tiles_1d, n_off, n_diag;
  int slabs_off, slabs_diag;
  int64_t rows_off, rows_diag;
  int slots;  // workgroups = partial tiles per matrix
  // XCD-aware order (xcd != 0, 1-D grid): a GROUP = the tiles_1d^2 workgroups that read the same two off-diagonal slabs
  // (= one diagonal slab, rows_diag = 2 rows_off) of one matrix, i.e. the same rows of every 128-column panel.
  // Workgroups are dealt round-robin over the 8 XCDs, so the group's members take hardware ids that are 8 apart and
  // consecutive on their XCD: they start together on one XCD and stream the same rows through ONE L2 (each panel
  // was fetched by the four tiles sharing it from four different XCDs otherwise: 4 x the fabric traffic).
  int xcd, members, groups_per_matrix, groups_total;
};
struct Gram128Ptrs {
  const void* a[kGram128MaxBatch];
};

template <int ROLE>  // 0: 4 x 4 tiles; 1: upper triangle of a diagonal block (10 tiles); 2: 2 x 4 tiles
__device__ __forceinline__ void gram128_load(const float* pa, const float* pb, int s, double (&av)[4], double (&bv)[4]) {
  const int off = 4 * s * G128_LD;
  if (ROLE == 1) {
#pragma unroll
    for (int a = 0; a < 4; ++a) av[a] = bv[a] = (double)pa[off + 16 * a];
  } else {
#pragma unroll
    for (int a = 0; a < (ROLE == 2 ? 2 : 4); ++a) av[a] = (double)pa[off + 16 * a];
#pragma unroll
    for (int b = 0; b < 4; ++b) bv[b] = (double)pb[off + 16 * b];
  }
}
template <int ROLE>
__device__ __forceinline__ void gram128_mfma(const double (&av)[4], const double (&bv)[4], f64x4 (&acc)[16]) {
#pragma unroll
  for (int a = 0; a < (ROLE == 2 ? 2 : 4); ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (ROLE != 1 || a <= b) acc[4 * a + b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[4 * a + b], 0, 0, 0);
}
// the eight k-steps of one chunk; pa / pb: this lane's element of row 0 of the two panels (LDS)
template <int ROLE>
__device__ __forceinline__ void gram128_chunk(const float* pa, const float* pb, f64x4 (&acc)[16]) {
  double av[2][4], bv[2][4];
  gram128_load<ROLE>(pa, pb, 0, av[0], bv[0]);
#pragma unroll
  for (int s = 0; s < GW_KB / 4; ++s) {
    if (s + 1 < GW_KB / 4) gram128_load<ROLE>(pa, pb, s + 1, av[(s + 1) & 1], bv[(s + 1) & 1]);
    gram128_mfma<ROLE>(av[s & 1], bv[s & 1], acc);
  }
}

// MODE 0: any shape (guarded, per-lane branches in the fetch).  MODE 1 (plain rows) / 2 (rows and columns through
// the offset tables): every chunk is interior -- whole 128-column panels, slabs of whole 32-row chunks, 16-byte
// loads -- and the fetch is eight straight-line loads.  In MODE 0 every load sits in an exec-masked block and carries
// its own s_waitcnt vmcnt(0) (the registers it overwrites may still be the target of a load of the previous trip,
// and a wait inside a skipped block clears nothing at the join): the eight loads of a chunk go out one after the
// other, each waiting for the one before, in front of the chunk's MFMAs.
template <typename TIN, int MODE>
__global__ void __launch_bounds__(256, 2)
gram128_kernel(Gram128Ptrs ptrs, int64_t m, int64_t n, int64_t lda, double* __restrict__ partial, Gram128Geom g,
               int vec_ok, const int64_t* __restrict__ row_off, const int64_t* __restrict__ col_off) {
  extern __shared__ __attribute__((aligned(16))) float g128_lds[];  // [2 buffers][2 panels][GW_KB][G128_LD]
  int id = blockIdx.x, vol = blockIdx.y;
  if (g.xcd) {
    const int x = blockIdx.x & 7, q = blockIdx.x >> 3;
    const int group = (q / g.members) * 8 + x, mem = q % g.members;
    if (group >= g.groups_total) return;
    vol = group / g.groups_per_matrix;
    const int sp = group % g.groups_per_matrix;
    if (g.xcd == 2) {  // one slab per group, diagonal slabs as long as the others
      id = mem < g.n_off ? mem * g.slabs_off + sp : g.n_off * g.slabs_off + (mem - g.n_off) * g.slabs_diag + sp;
    } else if (mem < 2 * g.n_off) {
      const int sl = 2 * sp + mem / g.n_off;
      if (sl >= g.slabs_off) return;
      id = (mem % g.n_off) * g.slabs_off + sl;
    } else {
      id = g.n_off * g.slabs_off + (mem - 2 * g.n_off) * g.slabs_diag + sp;
    }
  }
  const TIN* __restrict__ A = static_cast<const TIN*>(ptrs.a[vol]);
  int ti, tj, slab;
  int64_t rows;
  if (id < g.n_off * g.slabs_off) {
    int t = id / g.slabs_off;
    slab = id % g.slabs_off;
    rows = g.rows_off;
    ti = 0;
    while (t >= g.tiles_1d - 1 - ti) {
      t -= g.tiles_1d - 1 - ti;
      ++ti;
    }
    tj = ti + 1 + t;
  } else {
    const int t = (id - g.n_off * g.slabs_off) / g.slabs_diag;
    slab = (id - g.n_off * g.slabs_off) % g.slabs_diag;
    rows = g.rows_diag;
    ti = tj = t;
  }
  const bool diag = ti == tj;
  const int64_t i0 = (int64_t)ti * 128, j0 = (int64_t)tj * 128;
  const int64_t r_begin = (int64_t)slab * rows;
  const int64_t r_end = min(m, r_begin + rows);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane >> 4, lc = lane & 15;

  // staging map: GW_KB rows x 32 float4 per panel, 4 per thread
  float4 pi[4], pj[4];
  // gathered reads: the two column offsets of this thread never change (its column quad is fixed) and the row
  // offsets of a chunk are requested one chunk ahead -- looked up inside fetch() they put a table round trip in
  // front of the data loads, and the wave sat through it before it could start the chunk's MFMAs (+18 %)
  int64_t coli = 0, colj = 0, ro[4] = {0, 0, 0, 0};
  auto row_offsets = [&](int64_t r0) {
    if (MODE == 2 || (MODE == 0 && row_off)) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int64_t row = r0 + (tid + 256 * v) / 32;
        ro[v] = row < r_end ? row_off[row] : 0;
      }
    }
  };
  if (MODE == 2 || (MODE == 0 && row_off)) {
    const int c4 = (tid % 32) * 4;
    if (i0 + c4 + 3 < n) coli = col_off[i0 + c4];
    if (j0 + c4 + 3 < n) colj = col_off[j0 + c4];
  }
  auto fetch = [&](int64_t r0) {
    if constexpr (MODE != 0) {
      // interior chunk: straight-line loads, the raw elements converted on their way to LDS (stash)
      const int c4 = (tid % 32) * 4;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const TIN* src = MODE == 2 ? A + ro[v] + coli : A + (r0 + (tid + 256 * v) / 32) * lda + i0 + c4;
        pi[v] = load4_as_f32(src);
      }
      if (!diag) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const TIN* src = MODE == 2 ? A + ro[v] + colj : A + (r0 + (tid + 256 * v) / 32) * lda + j0 + c4;
          pj[v] = load4_as_f32(src);
        }
      }
      return;
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int e = tid + 256 * v;
      const int rr = e / 32, c4 = (e % 32) * 4;
      const int64_t row = r0 + rr;
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
      if (row < r_end && row_off) {  // gathered: offsets additive in (row, column); vec_ok guaranteed by the host
        const TIN* base = A + ro[v];
        if (i0 + c4 + 3 < n) x = load4_as_f32(base + coli);
        if (!diag && j0 + c4 + 3 < n) y = load4_as_f32(base + colj);
      } else if (row < r_end) {
        const TIN* base = A + row * lda;
        if (vec_ok && i0 + c4 + 3 < n) x = load4_as_f32(base + i0 + c4);
        else {
          if (i0 + c4 + 0 < n) x.x = (float)base[i0 + c4 + 0];
          if (i0 + c4 + 1 < n) x.y = (float)base[i0 + c4 + 1];
          if (i0 + c4 + 2 < n) x.z = (float)base[i0 + c4 + 2];
          if (i0 + c4 + 3 < n) x.w = (float)base[i0 + c4 + 3];
        }
        if (!diag) {
          if (vec_ok && j0 + c4 + 3 < n) y = load4_as_f32(base + j0 + c4);
          else {
            if (j0 + c4 + 0 < n) y.x = (float)base[j0 + c4 + 0];
            if (j0 + c4 + 1 < n) y.y = (float)base[j0 + c4 + 1];
            if (j0 + c4 + 2 < n) y.z = (float)base[j0 + c4 + 2];
            if (j0 + c4 + 3 < n) y.w = (float)base[j0 + c4 + 3];
          }
        }
      }
      pi[v] = x;
      pj[v] = y;
    }
  };
  auto stash = [&](int buf) {
    float* Pi = g128_lds + (2 * buf) * G128_PANEL;
    float* Pj = Pi + G128_PANEL;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int e = tid + 256 * v;
      const int rr = e / 32, c4 = (e % 32) * 4;
      *reinterpret_cast<float4*>(Pi + rr * G128_LD + c4) = pi[v];
      if (!diag) *reinterpret_cast<float4*>(Pj + rr * G128_LD + c4) = pj[v];
    }
  };

  // operand columns of this wave inside the two panels
  //   off-diagonal tile : wave (wr, wc) -> rows wr 64 of panel i, columns wc 64 of panel j
  //   diagonal tile     : wave 0 -> block (0, 0), wave 3 -> block (1, 1) (upper triangles), waves 1 / 2 -> rows
  //                       0..31 / 32..63 of block (0, 1); both operands from panel i
  int a_col, b_col;
  if (!diag) {
    a_col = (wave >> 1) * 64;
    b_col = (wave & 1) * 64;
  } else if (wave == 0 || wave == 3) {
    a_col = b_col = wave == 0 ? 0 : 64;
  } else {
    a_col = wave == 1 ? 0 : 32;
    b_col = 64;
  }

  double* out = partial + ((int64_t)vol * g.slots + id) * (128 * 128);
  // one copy of the chunk loop per role (the role is fixed for the life of the wave; a branch per chunk made
  // the register allocator keep the accumulators three times)
  auto run = [&](auto role_tag) {
    constexpr int ROLE = decltype(role_tag)::value;
    f64x4 acc[16];
#pragma unroll
    for (int a = 0; a < 16; ++a) acc[a] = (f64x4){0.0, 0.0, 0.0, 0.0};
    if (r_begin < r_end) {
      row_offsets(r_begin);
      fetch(r_begin);
      stash(0);
      row_offsets(r_begin + GW_KB);
    }
    __syncthreads();
    int buf = 0;
    for (int64_t r0 = r_begin; r0 < r_end; r0 += GW_KB, buf ^= 1) {
      const bool more = r0 + GW_KB < r_end;
      if (more) {
        fetch(r0 + GW_KB);          // in flight under the MFMAs
        row_offsets(r0 + 2 * GW_KB);  // for the fetch of the next iteration
      }
      const float* Pi = g128_lds + (2 * buf) * G128_PANEL + lr * G128_LD + lc;
      const float* Pj = ROLE == 0 ? Pi + G128_PANEL : Pi;
      gram128_chunk<ROLE>(Pi + a_col, Pj + b_col, acc);
      if (more) stash(buf ^ 1);
      __syncthreads();  // the other buffer is complete and nobody reads this one any more
    }
#pragma unroll
    for (int a = 0; a < (ROLE == 2 ? 2 : 4); ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (ROLE == 1 && a > b) continue;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int rr = a_col + 16 * a + lr + 4 * reg, cc = b_col + 16 * b + lc;
          out[rr * 128 + cc] = acc[4 * a + b][reg];
        }
      }
  };
  if (!diag) run(std::integral_constant<int, 0>{});
  else if (wave == 0 || wave == 3) run(std::integral_constant<int, 1>{});
  else run(std::integral_constant<int, 2>{});
}

// G of matrix blockIdx.z from its partial tiles: tile t = blockIdx.x (off-diagonal ones first), element
// e = blockIdx.y 256 + threadIdx.x; slabs summed in order, four in flight.
__global__ void __launch_bounds__(256)
gram128_reduce_kernel(const double* __restrict__ partial, Gram128Geom g, double* __restrict__ G, int64_t stride_G, int64_t n,
                      const int32_t* __restrict__ perm) {  // perm (or NULL): element (r, c) goes to (perm[r], perm[c])
  const int e = blockIdx.y * 256 + threadIdx.x;
  const int t = blockIdx.x;
  int ti, tj, base, count;
  if (t < g.n_off) {
    int u = t;
    ti = 0;
    while (u >= g.tiles_1d - 1 - ti) {
      u -= g.tiles_1d - 1 - ti;
      ++ti;
    }
    tj = ti + 1 + u;
    base = t * g.slabs_off;
    count = g.slabs_off;
  } else {
    ti = tj = t - g.n_off;
    base = g.n_off * g.slabs_off + (t - g.n_off) * g.slabs_diag;
    count = g.slabs_diag;
  }
  const int64_t r = (int64_t)ti * 128 + e / 128, c = (int64_t)tj * 128 + e % 128;
  if (r >= n || c >= n || (ti == tj && c < r)) return;  // diagonal tiles: upper part only (the rest was not computed)
  const double* src = partial + ((int64_t)blockIdx.z * g.slots + base) * (128 * 128) + e;
  double s = 0.0;
  int sl = 0;
  for (; sl + 4 <= count; sl += 4) {
    const double v0 = src[(int64_t)(sl + 0) * 16384], v1 = src[(int64_t)(sl + 1) * 16384];
    const double v2 = src[(int64_t)(sl + 2) * 16384], v3 = src[(int64_t)(sl + 3) * 16384];
    s = (((s + v0) + v1) + v2) + v3;
  }
  for (; sl < count; ++sl) s += src[(int64_t)sl * 16384];
  store_mirrored(G + (int64_t)blockIdx.z * stride_G, n, r, c, s, perm);
}

// ----------------------------------------------------------------------------------
// Gram for very narrow matrices (n <= 8, the first site of the sweep: m = N / d rows of d
// voxels): pure streaming.  One thread per row (grid-stride), the 36 products of a row go to
// fp64 registers; wave shuffle + LDS fold; one partial per workgroup, summed in fixed order.
// ----------------------------------------------------------------------------------
template <typename TIN>
__global__ void __launch_bounds__(256)
gram_small_kernel(const TIN* __restrict__ A, int64_t m, int n, int64_t lda, double* __restrict__ partial,
                  int vec_ok) {
  __shared__ double red[4][36];
  double acc[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) acc[i] = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < m; r += stride) {
    float x[8];
    const TIN* row = A + r * lda;
    if (vec_ok) {
      const float4 a = load4_as_f32(row), b = load4_as_f32(row + 4);
      x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) x[c] = c < n ? (float)row[c] : 0.f;
    }
    int idx = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = i; j < 8; ++j) acc[idx++] += (double)x[i] * (double)x[j];
  }
#pragma unroll
  for (int i = 0; i < 36; ++i) {
    double v = acc[i];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < 36)
    partial[(int64_t)blockIdx.x * 36 + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__global__ void __launch_bounds__(256)
gram_small_reduce_kernel(const double* __restrict__ partial, int n_blocks, double* __restrict__ G, int n) {
  __shared__ double part[7][36];
  const int e = threadIdx.x % 36, grp = threadIdx.x / 36;  // 7 groups of 36 threads (252 used)
  if (grp < 7) {
    double acc = 0.0;
    for (int b = grp; b < n_blocks; b += 7) acc += partial[(int64_t)b * 36 + e];
    part[grp][e] = acc;
  }
  __syncthreads();
  if (threadIdx.x >= 36) return;
  double s = 0.0;
  for (int k = 0; k < 7; ++k) s += part[k][e];
  int i = 0, rem = e;  // unrank e -> (i, j), j >= i
  while (rem >= 8 - i) {
    rem -= 8 - i;
    ++i;
  }
  const int j = i + rem;
  if (i < n && j < n) {
    G[i * n + j] = s;
    G[j * n + i] = s;
  }
}

// ---------------------------------------------------------------------------------- the plan
// Which kernel a call runs, with which geometry, and how many workspace bytes that takes.  The size queries return
// workspace_bytes, the launchers check the caller's buffer against the same field and lay their partial tiles out
// by the same geometry: the two cannot disagree.
enum class GramElem { F32, BF16, F64 };
template <typename TIN>
constexpr GramElem gram_elem() {
  return std::is_same<TIN, double>::value ? GramElem::F64 : std::is_same<TIN, float>::value ? GramElem::F32 : GramElem::BF16;
}

enum class GramRoute {
  None,            // nothing to run: an empty matrix, or a batched call of a shape only the single-matrix entries take
  Small,           // n <= 8: gram_small_kernel
  Tiles16,         // gram_partial_kernel: (16 T)^2 tiles read straight from global memory; every fp64 matrix
  Tiles64,         // 64 <= n < 128, m >= 256, one matrix: gram_wide_kernel
  Tiles128,        // n >= 128, m >= 256, one matrix or a batch: gram128_kernel
  Tiles64Batched,  // 64 <= n < 128, m >= 256, two matrices or more: gram_wide_batched_kernel
  Stream64,        // n == 64 of those: gram64_stream_kernel
};

// The A/B switches of the family (tools/README.md).  Tests and tools set them inside a running process, so every
// plan reads them afresh.
struct GramSwitches {
  int xcd;       // NDMPS_GRAM_XCD=1|2: XCD-aware workgroup order of the big batched Tiles128 launches (Gram128Geom)
  bool no_turn;  // NDMPS_GRAM_NO_TURN: no Gram launch takes the device-side turn between streams
  bool general;  // NDMPS_GRAM_GENERAL: Tiles128 on its guarded (any-shape) instantiation whatever the shape
  bool tiles64;  // NDMPS_GRAM64_TILES: a batch of 64-column matrices on the tile kernel instead of the stream
};
GramSwitches gram_switches() {
  const char* xcd = getenv("NDMPS_GRAM_XCD");
  return {xcd ? atoi(xcd) : 0, getenv("NDMPS_GRAM_NO_TURN") != nullptr, getenv("NDMPS_GRAM_GENERAL") != nullptr,
          getenv("NDMPS_GRAM64_TILES") != nullptr};
}
// NDMPS_ONE_TURN=1 (A/B): the Gram launches take the resident tridiagonalisations' lock, whole -- with several batches
// in flight (core/batch.py lanes) a Gram launch and a resident launch of another batch otherwise run together and slow
// each other (both fp64: one pipeline).  Unlike the switches above it is latched by the first launch that asks.
bool gram_one_turn() {
  static const bool one_turn = getenv("NDMPS_ONE_TURN") != nullptr;
  return one_turn;
}

constexpr int kGramSmallBlocks = 256;  // workgroups (= partial sums of 36 products) of gram_small_kernel at the most
constexpr int64_t kTile64Doubles = 64 * 64, kTile128Doubles = 128 * 128;

// Upper triangle of (16 T)^2 tiles x row slabs (gram_partial_kernel, gram_wide_body, gram64_stream_kernel)
struct GramGeom {
  int T;          // 16-wide sub-tiles per tile edge
  int tiles_1d;
  int n_tiles;    // upper triangle incl. diagonal
  int n_slabs;
  int64_t rows_per_slab;
};
// want_wgs workgroups per matrix spread over its tiles give the slabs asked for (one at least); none is shorter
// than min_rows, every one a multiple of `unit` rows
GramGeom gram_geometry(int T, int64_t m, int64_t n, int64_t want_wgs, bool whole_wgs, int64_t min_rows, int64_t unit) {
  GramGeom g;
  g.T = T;
  g.tiles_1d = (int)ndmps::ceil_div(n, 16 * T);
  g.n_tiles = g.tiles_1d * (g.tiles_1d + 1) / 2;
  // whole_wgs: never fewer workgroups than asked for (the slab count is rounded up)
  const int64_t want = std::max<int64_t>(1, whole_wgs ? ndmps::ceil_div(want_wgs, g.n_tiles) : want_wgs / g.n_tiles);
  g.rows_per_slab = ndmps::round_up(std::max<int64_t>(ndmps::ceil_div(m, want), min_rows), unit);
  g.n_slabs = (int)std::max<int64_t>(1, ndmps::ceil_div(m, g.rows_per_slab));
  return g;
}

// Slabs of gram128_kernel.  An off-diagonal workgroup costs 16 MFMAs per k-step, a diagonal one 10, so the
// diagonal tiles get 1.6 x longer slabs.  One matrix alone fills the GPU once (~2 workgroups per CU); a batch is
// cut into ~12 rounds of 512 workgroups (the tail of the last round is what is lost), never below 512 rows per
// workgroup (128 for a lone matrix).  The geometry depends on (m, n, batch) and the XCD switch only: a given call
// sequence is reproducible bit for bit.
Gram128Geom gram128_geometry(int64_t m, int64_t n, int batch, int xmode) {
  Gram128Geom g;
  g.tiles_1d = (int)ndmps::ceil_div(n, 128);
  g.n_off = g.tiles_1d * (g.tiles_1d - 1) / 2;
  g.n_diag = g.tiles_1d;
  const double weight = g.n_off + 0.625 * g.n_diag;  // workgroups per off-diagonal slab count
  const double want = 2.0 * ndmps::kNumCU * (batch > 1 ? 12.0 : 1.0) / std::max(batch, 1) / weight;
  const int64_t floor_rows = batch > 1 ? 512 : 128;  // a lone small matrix still spreads over the GPU
  int64_t s_off = std::max<int64_t>(1, std::min<int64_t>((int64_t)(want + 0.5), std::max<int64_t>(m / floor_rows, 1)));
  g.rows_off = ndmps::round_up(ndmps::ceil_div(m, s_off), GW_KB);
  g.rows_diag = ndmps::round_up((g.rows_off * 8 + 4) / 5, GW_KB);
  g.slabs_off = (int)ndmps::ceil_div(m, g.rows_off);
  g.slabs_diag = (int)ndmps::ceil_div(m, g.rows_diag);
  g.xcd = 0;
  g.members = g.groups_per_matrix = g.groups_total = 0;
  // big batched launches (the ones that take the device-side turn): XCD-aware groups, diagonal slabs of exactly two
  // off-diagonal slabs (a diagonal workgroup then does 2 x 10 / 16 of an off-diagonal one's MFMA work)
  if (batch > 1 && g.tiles_1d >= 2 && g.slabs_off >= 4 && xmode == 1) {
    g.rows_diag = 2 * g.rows_off;
    g.slabs_diag = (int)ndmps::ceil_div(m, g.rows_diag);
    g.xcd = 1;
    g.members = 2 * g.n_off + g.n_diag;
    g.groups_per_matrix = g.slabs_diag;
    g.groups_total = batch * g.groups_per_matrix;
  } else if (batch > 1 && g.tiles_1d >= 2 && g.slabs_off >= 4 && xmode == 2) {
    // as many workgroups as before: slabs longer by (n_off + 0.625 n_diag) / (n_off + n_diag)
    const int64_t s2 = std::max<int64_t>(1, (int64_t)(g.slabs_off * weight / (g.n_off + g.n_diag) + 0.5));
    g.rows_off = g.rows_diag = ndmps::round_up(ndmps::ceil_div(m, s2), GW_KB);
    g.slabs_off = g.slabs_diag = (int)ndmps::ceil_div(m, g.rows_off);
    g.xcd = 2;
    g.members = g.n_off + g.n_diag;
    g.groups_per_matrix = g.slabs_off;
    g.groups_total = batch * g.groups_per_matrix;
  }
  g.slots = g.n_off * g.slabs_off + g.n_diag * g.slabs_diag;
  return g;
}

struct GramPlan {
  GramRoute route;
  bool gathered;         // the operand is read through (row, column) offset tables
  GramSwitches sw;
  int small_blocks;      // Small: workgroups of this launch
  GramGeom slabs;        // Tiles16, Tiles64, Tiles64Batched, Stream64
  Gram128Geom g128;      // Tiles128
  int64_t workspace_bytes;
};

// batched: the call came through ndmps_gram_batched_*, which have the two LDS-staged tile sizes and the stream only
GramRoute gram_route(GramElem elem, int batch, int64_t m, int64_t n, bool batched, const GramSwitches& sw) {
  if (batch < 1 || m <= 0 || n <= 0) return GramRoute::None;
  const bool staged = m >= 256;  // at least eight 32-row chunks: worth staging in LDS
  if (batched) {
    if (n >= 128 && staged) return GramRoute::Tiles128;
    if (n >= 64 && staged && batch >= 2) return n == 64 && !sw.tiles64 ? GramRoute::Stream64 : GramRoute::Tiles64Batched;
    return GramRoute::None;
  }
  if (elem == GramElem::F64) return GramRoute::Tiles16;
  if (n <= 8) return GramRoute::Small;
  if (n >= 128 && staged) return GramRoute::Tiles128;
  if (n >= 64 && staged) return GramRoute::Tiles64;
  return GramRoute::Tiles16;
}

GramPlan gram_plan(GramElem elem, int batch, int64_t m, int64_t n, bool gathered, bool batched) {
  GramPlan p{};
  p.sw = gram_switches();
  p.gathered = gathered;
  p.route = gram_route(elem, batch, m, n, batched, p.sw);
  const int64_t f64 = (int64_t)sizeof(double);
  switch (p.route) {
    case GramRoute::None:
      break;
    case GramRoute::Small:  // a workgroup per 2048 rows; the workspace is sized for the most there can be
      p.small_blocks = (int)std::min<int64_t>(std::max<int64_t>(ndmps::ceil_div(m, 256 * 8), 1), kGramSmallBlocks);
      p.workspace_bytes = (int64_t)kGramSmallBlocks * 36 * f64 + 256;
      break;
    case GramRoute::Tiles16:
    case GramRoute::Tiles64: {
      // ~2 workgroups per CU; slabs of whole 16-row steps (4 waves x 4 rows) or whole 32-row chunks
      if (p.route == GramRoute::Tiles16)
        p.slabs = gram_geometry(n <= 16 ? 1 : (n <= 32 ? 2 : 4), m, n, 2 * ndmps::kNumCU, false, 64, 16);
      else
        p.slabs = gram_geometry(4, m, n, 2 * ndmps::kNumCU, false, 4 * GW_KB, GW_KB);
      // the slabs, behind them the group sums of launch_tile_reduce's first level, two tiles of slack
      const GramGeom& g = p.slabs;
      const int64_t ts = 16 * g.T;
      p.workspace_bytes = (int64_t)(g.n_slabs + g.n_slabs / kReduceGroup + 2) * g.n_tiles * ts * ts * f64 + 256;
      break;
    }
    case GramRoute::Tiles128:
      p.g128 = gram128_geometry(m, n, batch, p.sw.xcd);
      p.workspace_bytes = (int64_t)batch * p.g128.slots * kTile128Doubles * f64 + 256;
      break;
    case GramRoute::Tiles64Batched:
    case GramRoute::Stream64: {
      // tiles: ~10 workgroups per CU over the whole group (two rounds at five resident), so slabs are long; stream:
      // 6 per CU (three resident)
      const int64_t per_cu = p.route == GramRoute::Stream64 ? 6 : 10;
      p.slabs = gram_geometry(4, m, n, ndmps::ceil_div(per_cu * ndmps::kNumCU, batch), true, 4 * GW_KB, GW_KB);
      p.workspace_bytes = (int64_t)batch * p.slabs.n_slabs * p.slabs.n_tiles * kTile64Doubles * f64 + 256;
      break;
    }
  }
  return p;
}

int gram_check_workspace(const GramPlan& p, const void* d_ws, int64_t ws_bytes) {
  if (d_ws && ws_bytes >= p.workspace_bytes) return NDMPS_OK;
  ndmps::set_error("Gram workspace too small: %lld < %lld", (long long)ws_bytes, (long long)p.workspace_bytes);
  return NDMPS_EWORKSPACE;
}

}  // namespace

// Upper bound of every single-matrix plan's workspace_bytes over every n' <= n and every m, and of the batched
// plans' for `batch` matrices: the sweep sizes its Gram workspace before it knows the bonds it will find.  Counted
// in partial tiles, from the geometries above:
//   Tiles16, Tiles64: at most max(1, 512 / tiles) slabs per tile, so slabs x tiles <= max(512, tiles(n)); the
//     workspace holds (slabs + slabs / 16 + 2) x tiles of them, at most 64 x 64 doubles each: 17/16 of that product
//     plus 2 tiles(n), taken as 3 tiles(n) to cover the rounding;
//   Tiles128, one matrix: slots ~ 512 workgroups (slabs_off x (n_off + 0.625 n_diag) <= 512, the diagonal slabs
//     1.6 x longer) plus the rounding of the two slab counts: the same expression with 128 x 128 tiles;
//   a batch: ~12 rounds of 512 slots over the whole group, plus the rounding of the slab counts per matrix (the
//     batched 64-wide routes ask for 10 x 256 tiles of a quarter of the size: far below).
// Small needs 256 x 36 doubles: below each of these.
int64_t ndmps::gram_ws_bound(int64_t n, int batch) {
  const int64_t f64 = (int64_t)sizeof(double);
  const int64_t t1 = ceil_div(n, 64), nt1 = t1 * (t1 + 1) / 2;
  const int64_t narrow = (std::max<int64_t>(512, nt1) * 17 / 16 + 3 * nt1) * kTile64Doubles * f64 + 256;
  const int64_t t2 = ceil_div(n, 128), nt2 = t2 * (t2 + 1) / 2;
  const int64_t wide = (std::max<int64_t>(512, nt2) * 17 / 16 + 3 * nt2) * kTile128Doubles * f64 + 256;
  const int64_t batched = batch > 1 ? (12 * 512 + 3 * nt2 * batch + 64) * kTile128Doubles * f64 + 256 : 0;
  return std::max(std::max(narrow, wide), batched);
}

namespace {

// ---------------------------------------------------------------------------------- running a plan
int gram128_opt_in() {
  static std::mutex mu;
  static bool done[64] = {};
  int dev = 0;
  NDMPS_CHECK_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  if (dev < 0 || dev >= 64 || done[dev]) return NDMPS_OK;
#define NDMPS_GRAM128_OPT_IN(T, MODE)                                                                          \
  NDMPS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&gram128_kernel<T, MODE>),                 \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGram128Lds))
  NDMPS_GRAM128_OPT_IN(float, 0);
  NDMPS_GRAM128_OPT_IN(float, 1);
  NDMPS_GRAM128_OPT_IN(float, 2);
  NDMPS_GRAM128_OPT_IN(__bf16, 0);
  NDMPS_GRAM128_OPT_IN(__bf16, 1);
  NDMPS_GRAM128_OPT_IN(__bf16, 2);
#undef NDMPS_GRAM128_OPT_IN
  done[dev] = true;
  return NDMPS_OK;
}

// The operands of a batched launch.  vec_ok: every row of every matrix starts on a boundary of four elements (16
// bytes of fp32, 8 bytes of bf16) and holds a whole number of fours -- what the vector loads and a gathered operand
// (whose offset tables come in aligned runs of four) need.
template <typename TIN>
int gram_operands(const GramPlan& p, int batch, const TIN* const* h_A, int64_t n, int64_t lda, const int64_t* d_col_off,
                  int* vec_ok) {
  *vec_ok = (lda % 4 == 0 && n % 4 == 0) ? 1 : 0;
  for (int b = 0; b < batch; ++b) {
    NDMPS_REQUIRE(h_A[b], "NULL Gram operand %d", b);
    if ((uintptr_t)h_A[b] % (4 * sizeof(TIN)) != 0) *vec_ok = 0;
  }
  if (p.gathered) NDMPS_REQUIRE(d_col_off && *vec_ok, "gathered Gram needs n %% 4 == 0 and aligned bases");
  return NDMPS_OK;
}

// Tiles128: G[b] = A[b]^T A[b] for `batch` matrices of one shape (h_A: host array of device pointers)
template <typename TIN>
int run_tiles128(const GramPlan& p, int batch, const TIN* const* h_A, int64_t m, int64_t n, int64_t lda, double* d_G,
                 int64_t stride_G, double* partial, hipStream_t s, const int64_t* d_row_off, const int64_t* d_col_off,
                 const int32_t* d_perm) {
  NDMPS_TRY(gram128_opt_in());
  const Gram128Geom& g = p.g128;
  int vec_ok;
  NDMPS_TRY(gram_operands(p, batch, h_A, n, lda, d_col_off, &vec_ok));
  // a launch that fills the GPU for milliseconds (a lockstep group's raw Gram) takes its turn with those of other
  // streams: two of them at once gain nothing (both MFMA-bound) and keep each other's groups in phase
  const bool turn = (int64_t)batch * g.slots >= 4096 && !p.sw.no_turn;
  const bool one_turn = gram_one_turn();
  ndmps::Turn gram_turn(s, one_turn ? ndmps::kTurnTeam : ndmps::kTurnGram, one_turn ? 2u : 1u, one_turn ? 2u : 1u);
  if (turn) NDMPS_TRY(gram_turn.begin());
  // every chunk interior (whole panels, whole 32-row chunks, 16-byte loads): the straight-line fetch
  const bool interior = vec_ok && n % 128 == 0 && m % GW_KB == 0 && g.rows_off % GW_KB == 0 && g.rows_diag % GW_KB == 0 &&
                        !p.sw.general;
  auto kernel = !interior ? gram128_kernel<TIN, 0> : (p.gathered ? gram128_kernel<TIN, 2> : gram128_kernel<TIN, 1>);
  void* span = ndmps::span_begin(s);
  for (int base = 0; base < batch; base += kGram128MaxBatch) {
    const int count = std::min(kGram128MaxBatch, batch - base);
    Gram128Ptrs ptrs;
    for (int t = 0; t < count; ++t) ptrs.a[t] = h_A[base + t];
    double* part = partial + (int64_t)base * g.slots * kTile128Doubles;
    if (g.xcd) {
      Gram128Geom gc = g;  // this launch's matrices
      gc.groups_total = count * g.groups_per_matrix;
      const unsigned wgs = (unsigned)(ndmps::ceil_div(gc.groups_total, 8) * g.members * 8);
      hipLaunchKernelGGL(kernel, dim3(wgs), dim3(256), kGram128Lds, s, ptrs, m, n, lda, part, gc, vec_ok, d_row_off,
                         d_col_off);
    } else {
      hipLaunchKernelGGL(kernel, dim3(g.slots, count), dim3(256), kGram128Lds, s, ptrs, m, n, lda, part, g, vec_ok,
                         d_row_off, d_col_off);
    }
  }
  // algorithmic work of the span: the upper triangle incl. the diagonal, 2 flops per product
  ndmps::span_end(span, s, turn ? ndmps::kSpanGram : ndmps::kSpanGramSmall, (batch + kGram128MaxBatch - 1) / kGram128MaxBatch,
                  (int64_t)batch * m * n * (n + 1));
  NDMPS_TRY(gram_turn.end());
  hipLaunchKernelGGL(gram128_reduce_kernel, dim3(g.n_off + g.n_diag, 64, batch), dim3(256), 0, s, partial, g, d_G, stride_G, n,
                     d_perm);
  NDMPS_LAUNCH_CHECK();
  return NDMPS_OK;
}

// Tiles64Batched and Stream64: up to 64 matrices per launch, each launch followed by its reduction
template <typename TIN>
int run_tiles64_batched(const GramPlan& p, int batch, const TIN* const* h_A, int64_t m, int64_t n, int64_t lda, double* d_G,
                        int64_t stride_G, double* partial, hipStream_t s, const int64_t* d_row_off,
                        const int64_t* d_col_off, const int32_t* d_perm) {
  const GramGeom& g = p.slabs;
  const bool stream = p.route == GramRoute::Stream64;
  int vec_ok;
  NDMPS_TRY(gram_operands(p, batch, h_A, n, lda, d_col_off, &vec_ok));
  NDMPS_REQUIRE(!stream || vec_ok, "the 64-column Gram stream needs lda %% 4 == 0 and 16-byte aligned operands");
  void* span = ndmps::span_begin(s);
  for (int base = 0; base < batch; base += 64) {
    const int count = std::min(64, batch - base);
    GramBatchPtrs ptrs;
    for (int t = 0; t < count; ++t) ptrs.a[t] = h_A[base + t];
    double* part = partial + (int64_t)base * g.n_slabs * g.n_tiles * kTile64Doubles;
    if (stream && p.gathered)
      hipLaunchKernelGGL((gram64_stream_kernel<TIN, true>), dim3(1, g.n_slabs, count), dim3(256), 0, s, ptrs, m, lda, part,
                         g.rows_per_slab, d_row_off, d_col_off);
    else if (stream)
      hipLaunchKernelGGL((gram64_stream_kernel<TIN, false>), dim3(1, g.n_slabs, count), dim3(256), 0, s, ptrs, m, lda, part,
                         g.rows_per_slab, d_row_off, d_col_off);
    else
      hipLaunchKernelGGL((gram_wide_batched_kernel<TIN>), dim3(g.n_tiles, g.n_slabs, count), dim3(256), 0, s, ptrs, m, n, lda,
                         part, g.tiles_1d, g.rows_per_slab, vec_ok, d_row_off, d_col_off);
    hipLaunchKernelGGL(tile_reduce_batched_kernel<64>, dim3(g.n_tiles, 16, count), dim3(256), 0, s, part, g.n_slabs, g.tiles_1d,
                       g.n_tiles, d_G + (int64_t)base * stride_G, stride_G, n, d_perm);
  }
  ndmps::span_end(span, s, ndmps::kSpanGramSmall, (batch + 63) / 64, (int64_t)batch * m * n * (n + 1));
  NDMPS_LAUNCH_CHECK();
  return NDMPS_OK;
}

template <int T, typename TIN>
int run_tiles16(const GramGeom& g, const TIN* d_A, int64_t m, int64_t n, int64_t lda, double* d_G, double* partial,
                hipStream_t s) {
  NDMPS_REQUIRE(g.n_slabs < 65536, "Gram slab count %d exceeds grid.y", g.n_slabs);
  hipLaunchKernelGGL((gram_partial_kernel<T, TIN>), dim3(g.n_tiles, g.n_slabs), dim3(256), 0, s, d_A, m, n, lda, partial,
                     g.tiles_1d, g.rows_per_slab);
  NDMPS_LAUNCH_CHECK();
  return launch_tile_reduce<16 * T>(partial, g.n_slabs, g.tiles_1d, g.n_tiles, d_G, n, s);
}

template <typename TIN>
int run_tiles64(const GramGeom& g, const TIN* d_A, int64_t m, int64_t n, int64_t lda, double* d_G, double* partial,
                hipStream_t s, int vec_ok, const int64_t* d_row_off, const int64_t* d_col_off, const int32_t* d_perm) {
  NDMPS_REQUIRE(g.n_slabs < 65536, "Gram slab count %d exceeds grid.y", g.n_slabs);
  hipLaunchKernelGGL((gram_wide_kernel<TIN>), dim3(g.n_tiles, g.n_slabs), dim3(256), 0, s, d_A, m, n, lda, partial, g.tiles_1d,
                     g.rows_per_slab, vec_ok, d_row_off, d_col_off);
  NDMPS_LAUNCH_CHECK();
  return launch_tile_reduce<64>(partial, g.n_slabs, g.tiles_1d, g.n_tiles, d_G, n, s, d_perm);
}

template <typename TIN>
int run_small(int blocks, const TIN* d_A, int64_t m, int64_t n, int64_t lda, double* d_G, double* partial, hipStream_t s,
              int vec_ok) {
  hipLaunchKernelGGL(gram_small_kernel<TIN>, dim3(blocks), dim3(256), 0, s, d_A, m, (int)n, lda, partial,
                     (vec_ok && n == 8) ? 1 : 0);
  hipLaunchKernelGGL(gram_small_reduce_kernel, dim3(1), dim3(256), 0, s, partial, blocks, d_G, (int)n);
  NDMPS_LAUNCH_CHECK();
  return NDMPS_OK;
}

// One matrix of any storage type.  fp64 always plans Tiles16 (gram_route), the only route instantiated for it.
template <typename TIN>
int gram_single(const TIN* d_A, int64_t m, int64_t n, int64_t lda, double* d_G, void* d_ws, int64_t ws_bytes,
                ndmps_stream_t stream, const int64_t* d_row_off = nullptr, const int64_t* d_col_off = nullptr,
                const int32_t* d_perm = nullptr) {
  NDMPS_REQUIRE(d_A && d_G, "NULL Gram operand");
  NDMPS_REQUIRE(m > 0 && n > 0 && lda >= n, "bad Gram extents m=%lld n=%lld lda=%lld", (long long)m,
                (long long)n, (long long)lda);
  const GramPlan p = gram_plan(gram_elem<TIN>(), 1, m, n, d_row_off != nullptr, false);
  NDMPS_TRY(gram_check_workspace(p, d_ws, ws_bytes));
  hipStream_t s = (hipStream_t)stream;
  double* partial = (double*)d_ws;
  const bool staged = p.route == GramRoute::Tiles64 || p.route == GramRoute::Tiles128;
  const bool aligned = (uintptr_t)d_A % (4 * sizeof(TIN)) == 0;  // four elements per load: 16 bytes of fp32, 8 of bf16
  NDMPS_REQUIRE(!d_perm || d_row_off, "a column permutation comes with the offset tables");
  if (p.gathered)
    NDMPS_REQUIRE(d_col_off && staged && n % 4 == 0 && aligned,
                  "gathered Gram needs the wide path (n >= 64, m >= 256), n %% 4 == 0 and an aligned base");
  if constexpr (!std::is_same<TIN, double>::value) {
    const int vec_ok = (lda % 4 == 0 && n % 4 == 0 && aligned) ? 1 : 0;
    if (p.route == GramRoute::Small) return run_small<TIN>(p.small_blocks, d_A, m, n, lda, d_G, partial, s, vec_ok);
    if (p.route == GramRoute::Tiles128)
      return run_tiles128<TIN>(p, 1, &d_A, m, n, lda, d_G, n * n, partial, s, d_row_off, d_col_off, d_perm);
    if (p.route == GramRoute::Tiles64)
      return run_tiles64<TIN>(p.slabs, d_A, m, n, lda, d_G, partial, s, vec_ok, d_row_off, d_col_off, d_perm);
  }
  if (p.slabs.T == 1) return run_tiles16<1, TIN>(p.slabs, d_A, m, n, lda, d_G, partial, s);
  if (p.slabs.T == 2) return run_tiles16<2, TIN>(p.slabs, d_A, m, n, lda, d_G, partial, s);
  return run_tiles16<4, TIN>(p.slabs, d_A, m, n, lda, d_G, partial, s);
}

// A batch of matrices of one shape: h_A[b] (host array of device pointers) -> d_G + b stride_G.  A shape without a
// batched route (n < 64, m < 256, one matrix of fewer than 128 columns) is a bad argument: the caller loops over
// the single-matrix entry.
template <typename TIN>
int gram_batched(int batch, const TIN* const* h_A, int64_t m, int64_t n, int64_t lda, double* d_G, int64_t stride_G,
                 void* d_ws, int64_t ws_bytes, ndmps_stream_t stream, const int64_t* d_row_off = nullptr,
                 const int64_t* d_col_off = nullptr, const int32_t* d_perm = nullptr) {
  const GramPlan p = gram_plan(gram_elem<TIN>(), batch, m, n, d_row_off != nullptr, true);
  NDMPS_REQUIRE(batch >= 1 && h_A && d_G && p.route != GramRoute::None && lda >= n && stride_G >= n * n,
                "bad batched Gram argument (batch=%d m=%lld n=%lld)", batch, (long long)m, (long long)n);
  NDMPS_TRY(gram_check_workspace(p, d_ws, ws_bytes));
  if (p.route == GramRoute::Tiles128)
    return run_tiles128<TIN>(p, batch, h_A, m, n, lda, d_G, stride_G, (double*)d_ws, (hipStream_t)stream, d_row_off,
                             d_col_off, d_perm);
  return run_tiles64_batched<TIN>(p, batch, h_A, m, n, lda, d_G, stride_G, (double*)d_ws, (hipStream_t)stream, d_row_off,
                                  d_col_off, d_perm);
}

}  // namespace

// ---------------------------------------------------------------------------------- entry points
extern "C" int64_t ndmps_gram_workspace_bytes(int64_t m, int64_t n) {
  return gram_plan(GramElem::F32, 1, m, n, false, false).workspace_bytes;
}
// fp64 storage (the reference's own element type, core/ndmps.py:56): the matrix is read as fp64 straight from global
// memory by the tile kernel without LDS staging (64 x 64 tiles of the upper triangle x row slabs) -- a fidelity
// mode, not the throughput path.  Products of two fp64 numbers are rounded: G carries ~sqrt(m) eps relative error.
extern "C" int64_t ndmps_gram_f64_workspace_bytes(int64_t m, int64_t n) {
  return gram_plan(GramElem::F64, 1, m, n, false, false).workspace_bytes;
}
// 0: the shape has no batched route
extern "C" int64_t ndmps_gram_batched_workspace_bytes(int batch, int64_t m, int64_t n) {
  return gram_plan(GramElem::F32, batch, m, n, false, true).workspace_bytes;
}

// The plan of a call, for tests and tools (slot order: include/ndmps_hip.h).  Host arithmetic only: no GPU call, and
// no launcher goes through it.
extern "C" int ndmps_gram_plan_query(int elem, int batch, int64_t m, int64_t n, int gathered, int batched, int64_t* h_out) {
  NDMPS_REQUIRE(h_out && elem >= 0 && elem <= 2, "bad Gram plan query (elem=%d)", elem);
  const GramPlan p = gram_plan(elem == 0 ? GramElem::F32 : (elem == 1 ? GramElem::BF16 : GramElem::F64), batch, m, n,
                               gathered != 0, batched != 0);
  const int64_t out[NDMPS_GRAM_PLAN_SLOTS] = {
      (int64_t)p.route,    p.small_blocks,    p.slabs.T,        p.slabs.n_tiles, p.slabs.n_slabs, p.slabs.rows_per_slab,
      p.g128.tiles_1d,     p.g128.slabs_off,  p.g128.slabs_diag, p.g128.rows_off, p.g128.rows_diag, p.g128.xcd,
      p.g128.slots,        p.workspace_bytes};
  std::copy(out, out + NDMPS_GRAM_PLAN_SLOTS, h_out);
  return NDMPS_OK;
}

extern "C" int ndmps_gram_f32(const float* d_A, int64_t m, int64_t n, int64_t lda, double* d_G,
                              void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  return gram_single<float>(d_A, m, n, lda, d_G, d_ws, ws_bytes, stream);
}
// same with a bf16 matrix (products of two bf16 numbers are exact in fp32, let alone fp64)
extern "C" int ndmps_gram_bf16(const void* d_A, int64_t m, int64_t n, int64_t lda, double* d_G,
                               void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  return gram_single<__bf16>((const __bf16*)d_A, m, n, lda, d_G, d_ws, ws_bytes, stream);
}
extern "C" int ndmps_gram_f64(const double* d_A, int64_t m, int64_t n, int64_t lda, double* d_G, void* d_ws,
                              int64_t ws_bytes, ndmps_stream_t stream) {
  return gram_single<double>(d_A, m, n, lda, d_G, d_ws, ws_bytes, stream);
}

// G = A^T A where element (r, c) of A is d_base[d_row_off[r] + d_col_off[c]] (the C-order volume read through the
// index permutation; d_col_off in aligned runs of four consecutive offsets); wide path only (n >= 64, m >= 256).
// d_col_perm (may be NULL): the columns were visited in another order than the caller numbers them (memory order
// of the volume); entry (a, b) of the product is stored at G[d_col_perm[a]][d_col_perm[b]] by the slab reduction
// itself (a separate pass over a group's 512 x 512 matrices took 0.47 ms per launch of 32).
extern "C" int ndmps_gram_indexed_f32(const float* d_base, int64_t m, int64_t n, const int64_t* d_row_off,
                                      const int64_t* d_col_off, const int32_t* d_col_perm, double* d_G, void* d_ws,
                                      int64_t ws_bytes, ndmps_stream_t stream) {
  NDMPS_REQUIRE(d_row_off && d_col_off, "NULL offset table");
  return gram_single<float>(d_base, m, n, n, d_G, d_ws, ws_bytes, stream, d_row_off, d_col_off, d_col_perm);
}

// Batched Gram of `batch` matrices of one shape (m >= 256; n >= 128, or n >= 64 for two matrices or more): one
// launch for the whole batch (what a lockstep group of volumes needs at a site).
extern "C" int ndmps_gram_batched_f32(int batch, const float* const* h_A, int64_t m, int64_t n, int64_t lda,
                                      double* d_G, int64_t stride_G, void* d_ws, int64_t ws_bytes,
                                      ndmps_stream_t stream) {
  return gram_batched<float>(batch, h_A, m, n, lda, d_G, stride_G, d_ws, ws_bytes, stream);
}
extern "C" int ndmps_gram_batched_bf16(int batch, const void* const* h_A, int64_t m, int64_t n, int64_t lda,
                                       double* d_G, int64_t stride_G, void* d_ws, int64_t ws_bytes,
                                       ndmps_stream_t stream) {
  return gram_batched<__bf16>(batch, (const __bf16* const*)h_A, m, n, lda, d_G, stride_G, d_ws, ws_bytes, stream);
}
extern "C" int ndmps_gram_batched_indexed_f32(int batch, const float* const* h_base, int64_t m, int64_t n,
                                              const int64_t* d_row_off, const int64_t* d_col_off,
                                              const int32_t* d_col_perm, double* d_G, int64_t stride_G, void* d_ws,
                                              int64_t ws_bytes, ndmps_stream_t stream) {
  NDMPS_REQUIRE(d_row_off && d_col_off, "NULL offset table");
  return gram_batched<float>(batch, h_base, m, n, n, d_G, stride_G, d_ws, ws_bytes, stream, d_row_off, d_col_off, d_col_perm);
}
