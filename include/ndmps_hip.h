/*
 * ndmps_hip.h -- C ABI of libndmps_hip.so, the MI355X (gfx950) implementation of the
 * NDMPS encode -> truncate -> reconstruct hot path of Alandroid/img-compression-mps.
 *
 * The reference has no FFI: its hot path is Python calling quimb / NumPy / SciPy
 * (SURVEY.md 8b).  Each entry point below therefore names the reference call it
 * replaces (file:line relative to /root/reference/src/imgcompressionmps/).
 * INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer named d_* is DEVICE memory (HBM) owned by the caller; h_* is host.
 *   - all matrices are row-major; cores are (chi_i, d_i, chi_{i+1}) row-major.
 *   - `stream` is a hipStream_t passed as void* (0 = default stream).
 *   - every function returns 0 on success, a negative NDMPS_E* code otherwise;
 *     ndmps_last_error() returns a thread-local message for the last failure.
 *   - no function allocates device memory except ndmps_plan_create(); workspaces are
 *     caller-provided and sized by the *_layout / *_workspace_bytes queries.
 *   - functions that return data-dependent bond sizes synchronise `stream` internally.
 */
#ifndef NDMPS_HIP_H
#define NDMPS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NDMPS_OK 0
#define NDMPS_EINVAL (-1)   /* bad argument (maps to ValueError) */
#define NDMPS_EHIP (-2)     /* HIP runtime failure (maps to RuntimeError) */
#define NDMPS_ENOCONV (-3)  /* eigen-solver did not converge */
#define NDMPS_EWORKSPACE (-4) /* workspace too small */
#define NDMPS_ETEAM (-5)    /* a resident tridiagonalisation gave up waiting for its workgroups (GPU shared with
                             * something that holds the compute units): the call's outputs are invalid; repeat it
                             * after ndmps_syevd_topk_set_team(0) (sweeps whose input is intact do so themselves) */

typedef void* ndmps_stream_t;
typedef struct ndmps_plan ndmps_plan_t;

int ndmps_version(void);
const char* ndmps_last_error(void);
/* number of HIP devices visible, or a negative code; never initialises a context */
int ndmps_device_count(void);

/* n HIP streams of the current device on pairwise different hardware queues (as far as the runtime
 * has queues: *n_independent tells how many are; the rest share).  The runtime binds a stream to one
 * of its few queues at first use and does not report which, so the binding is measured with a bounded
 * spin kernel.  For the concurrent volume groups of the batch caller
 * (reference: evaluation/benchmark.py:58-100 loops over independent tensors one by one; here each
 * group of the list runs on its own stream). */
int ndmps_streams_create(int n, void** h_streams, int* n_independent);
int ndmps_streams_destroy(int n, void* const* h_streams);

/* Launch spans for the roofline of bench.py: when enabled, the kernels bench.py prices bracket themselves with HIP
 * events on the stream they are launched on and file the span under a slot: 1 = column launches of the direct
 * eigen-solver (amount = algorithmic bytes), 2 = the resident tridiagonalisation (one span per launch sequence of a
 * batch; bytes), 3 = the Gram launches that fill the GPU for milliseconds and take a device-side turn (a lockstep
 * group's raw Gram; amount = FLOPS m n (n + 1) per matrix), 4 = every other batched Gram launch (flops).  collect
 * sums device ms, launches and amounts of a slot's spans recorded so far (and clears them); it waits for their
 * events.  No reference counterpart. */
int ndmps_profile_enable(int on);
int ndmps_profile_collect(int slot, double* h_ms, int64_t* h_launches, int64_t* h_bytes);

/* ---------------------------------------------------------------------------------
 * Index permutation ("reshape stage").
 * Replaces: utils/core.py:6-35,129-168 (gen_encoding_map, never materialised here),
 *           core/ndmps.py:66-71 (scatter  contracted[enc] = tensor.flatten()) and
 *           core/ndmps.py:144-148 (gather recovered = dense[enc]).
 * factor_arr is the (L, ndim) int64 array of utils/core.py:79-126 (get_factorlist).
 * --------------------------------------------------------------------------------- */
int ndmps_plan_create(ndmps_plan_t** out, int ndim, const int64_t* h_shape, int L,
                      const int64_t* h_factor_arr);
/* The same permutation onto the site-order tensor with its AXES REVERSED (C-order over d_{L-1} .. d_0): what a
 * left-to-right sweep (quimb's other from_dense convention, SURVEY a4's caveat) works on when it runs as a
 * right-to-left sweep of the mirrored chain.  Every plan entry point works on it; "site order" then means the reversed
 * order (ndmps_plan_split_offsets: n_cols = a product of LEADING site dimensions). */
int ndmps_plan_create_reversed(ndmps_plan_t** out, int ndim, const int64_t* h_shape, int L,
                               const int64_t* h_factor_arr);
int ndmps_plan_destroy(ndmps_plan_t* plan);
int64_t ndmps_plan_numel(const ndmps_plan_t* plan);
/* 1 if the LDS-tiled kernels are used for this plan, 0 for the generic gather */
int ndmps_plan_is_tiled(const ndmps_plan_t* plan);
/* Host-only emulation of the kernels' index arithmetic from the plan's tables (no GPU
 * needed; used by the CPU tests).  h_out[numel]: mode 0 = source offset read per site-order
 * position (generic encode), 1 = site-order offset read per C-order position (generic
 * decode), 2 = source offset stored per site-order position by the tiled kernels (-1 when
 * the plan is not tiled).  Returns 1/0 (tiled or not) or a negative error code. */
int ndmps_plan_emulate(int ndim, const int64_t* h_shape, int L, const int64_t* h_factor_arr,
                       int mode, int64_t* h_out);
int ndmps_plan_emulate_reversed(int ndim, const int64_t* h_shape, int L, const int64_t* h_factor_arr,
                                int mode, int64_t* h_out);
/* dst (C-order over site dims d_0..d_{L-1}) <- src (C-order over shape); bit-exact */
int ndmps_encode_permute(const ndmps_plan_t* plan, const void* d_src, void* d_dst,
                         int elem_bytes, ndmps_stream_t stream);
/* out (C-order over shape) <- dense (C-order over site dims); bit-exact */
int ndmps_decode_permute(const ndmps_plan_t* plan, const void* d_dense, void* d_out,
                         int elem_bytes, ndmps_stream_t stream);
/* The same permutations for the volumes of a lockstep group in ONE launch (thirty-two per launch): h_src / h_dst are
 * HOST arrays of `count` device pointers.  Replaces the per-volume Python loop around core/ndmps.py:66-71 and :144-147
 * (evaluation/benchmark.py:80-100); bit-exact like the single-volume calls. */
int ndmps_encode_permute_many(const ndmps_plan_t* plan, int count, const void* const* h_src, void* const* h_dst,
                              int elem_bytes, ndmps_stream_t stream);
int ndmps_decode_permute_many(const ndmps_plan_t* plan, int count, const void* const* h_dense, void* const* h_out,
                              int elem_bytes, ndmps_stream_t stream);
/* force the generic gather kernels (testing / A-B timing) */
int ndmps_encode_permute_generic(const ndmps_plan_t* plan, const void* d_src, void* d_dst,
                                 int elem_bytes, ndmps_stream_t stream);
int ndmps_decode_permute_generic(const ndmps_plan_t* plan, const void* d_dense, void* d_out,
                                 int elem_bytes, ndmps_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Last-axis orthonormal DCT-II / DCT-III.
 * Replaces: scipy.fftpack.dct / idct at core/ndmps.py:62-63 and :152-153.
 * d_x, d_y: (rows, n) row-major fp32; d_basis: (n, n) fp32 scratch filled by
 * ndmps_dct_basis_f32 once per n (forward basis B[j][k] = s_k cos(pi (2j+1) k / 2n)).
 * --------------------------------------------------------------------------------- */
int ndmps_dct_basis_f32(float* d_basis, int64_t n, ndmps_stream_t stream);
int ndmps_dct_last_f32(const float* d_x, float* d_y, int64_t rows, int64_t n,
                       const float* d_basis, ndmps_stream_t stream);
int ndmps_idct_last_f32(const float* d_y, float* d_x, int64_t rows, int64_t n,
                        const float* d_basis, ndmps_stream_t stream);
/* The same transforms for the volumes of a lockstep group in ONE launch (thirty-two per launch): h_x / h_y are HOST
 * arrays of `count` device pointers, every volume (rows, n) row-major and distinct from its result.  Replaces the
 * per-volume Python loop around core/ndmps.py:62-63 and :152-153 (evaluation/benchmark.py:80-100); results equal the
 * single-volume calls bit for bit: every volume takes the route of its own single call (a volume whose operands are
 * not 16-byte aligned goes through the basis product, its aligned neighbours through the FFT).  d_basis may be NULL
 * when n is a power of two in [64, 1024] and every operand is 16-byte aligned (the FFT route). */
int ndmps_dct_last_many_f32(int count, const float* const* h_x, float* const* h_y, int64_t rows, int64_t n,
                            const float* d_basis, ndmps_stream_t stream);
int ndmps_idct_last_many_f32(int count, const float* const* h_y, float* const* h_x, int64_t rows, int64_t n,
                             const float* d_basis, ndmps_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Reductions that keep NDMPS state (core/ndmps.py:60-61 norm, :75,:80-82 boundary_list).
 * h_out / d_out as named; *_f32 read fp32 and accumulate in fp64.
 * --------------------------------------------------------------------------------- */
int ndmps_sumsq_f32(const float* d_x, int64_t n, double* h_out, void* d_ws, int64_t ws_bytes,
                    ndmps_stream_t stream);
int ndmps_minmax_f32(const float* d_x, int64_t n, float* h_min, float* h_max, void* d_ws,
                     int64_t ws_bytes, ndmps_stream_t stream);
/* min/max (and optionally the fp64 sum of squares) of `count` tensors with one launch and one
 * synchronisation (boundary_list of all cores, core/ndmps.py:80-82): h_ptrs / h_lens are host
 * arrays, h_out gets (min, max) pairs, h_sumsq (may be NULL) one double per tensor */
int64_t ndmps_minmax_many_workspace_bytes(int count);
int ndmps_minmax_many_f32(int count, const float* const* h_ptrs, const int64_t* h_lens,
                          float* h_out, double* h_sumsq, void* d_ws, int64_t ws_bytes,
                          ndmps_stream_t stream);

/* The same reduction for the cores of a lockstep group sitting in one arena (row b = volume b, core i at
 * h_offsets[i] with h_lens[i] elements; at most 64 cores), in two halves so that nothing waits in between:
 * _launch enqueues the kernel (asynchronous; tensor (b, i) is entry b * n_cores + i), _collect copies the partials
 * back, synchronises and folds them into (min, max) pairs and sums of squares.  core/ndmps.py:75-76 computes these
 * eagerly; here they are issued with the sweep and read when boundary_list / norm_value are asked for. */
int64_t ndmps_minmax_partials_bytes(int count);
int ndmps_minmax_arena_launch_f32(const float* d_base, int64_t row_stride, int batch, int n_cores,
                                  const int64_t* h_offsets, const int64_t* h_lens, double* d_partial,
                                  ndmps_stream_t stream);
int ndmps_minmax_collect(int count, const double* d_partial, float* h_out, double* h_sumsq, ndmps_stream_t stream);
int ndmps_scale_f32(float* d_x, int64_t n, double factor, ndmps_stream_t stream);
/* h_x[t][0 .. n) *= h_factor[t] for `count` fp32 tensors of n elements each in one launch per thirty-two tensors: the
 * division by the norm of core/ndmps.py:60-61 for a whole lockstep group (h_x, h_factor: HOST arrays). */
int ndmps_scale_many_f32(int count, float* const* h_x, int64_t n, const double* h_factor, ndmps_stream_t stream);
int64_t ndmps_reduce_workspace_bytes(void);

/* ---------------------------------------------------------------------------------
 * Dense building blocks (exported for tests and for INTEGRATION.md users).
 * --------------------------------------------------------------------------------- */
/* C(m,n) = op(A)(m,k) op(B)(k,n), fp32 MFMA (v_mfma_f32_32x32x2_f32), fp32 accumulate */
int ndmps_sgemm(int transA, int transB, int64_t m, int64_t n, int64_t k, const float* d_A,
                int64_t lda, const float* d_B, int64_t ldb, float* d_C, int64_t ldc,
                ndmps_stream_t stream);
/* same in fp64 (v_mfma_f64_16x16x4_f64) */
int ndmps_dgemm(int transA, int transB, int64_t m, int64_t n, int64_t k, const double* d_A,
                int64_t lda, const double* d_B, int64_t ldb, double* d_C, int64_t ldc,
                ndmps_stream_t stream);

/* `batch` (<= ndmps_gemm_batched_max()) products of one shape in ONE launch: h_A / h_B / h_C are HOST arrays of
 * device pointers (the reference multiplies volume by volume in a Python loop, evaluation/benchmark.py:73-100);
 * same tiles and arithmetic as ndmps_sgemm / ndmps_dgemm / ndmps_sgemm_indexed on each triple. */
int ndmps_gemm_batched_max(void);
int ndmps_sgemm_batched(int batch, int transA, int transB, int64_t m, int64_t n, int64_t k, const float* const* h_A,
                        int64_t lda, const float* const* h_B, int64_t ldb, float* const* h_C, int64_t ldc,
                        ndmps_stream_t stream);
int ndmps_dgemm_batched(int batch, int transA, int transB, int64_t m, int64_t n, int64_t k, const double* const* h_A,
                        int64_t lda, const double* const* h_B, int64_t ldb, double* const* h_C, int64_t ldc,
                        ndmps_stream_t stream);
int ndmps_sgemm_indexed_batched(int batch, int64_t m, int64_t n, int64_t k, const float* const* h_A, int64_t lda,
                                const int64_t* d_a_row, const int64_t* d_a_col, int a_vec4, const float* const* h_B,
                                int64_t ldb, float* const* h_C, int64_t ldc, const int64_t* d_c_row,
                                const int64_t* d_c_col, ndmps_stream_t stream);
/* G(n,n) fp64 = A^T A for A (m,n) fp32 row-major; products exact, fp64 accumulation */
int64_t ndmps_gram_workspace_bytes(int64_t m, int64_t n);
int ndmps_gram_f32(const float* d_A, int64_t m, int64_t n, int64_t lda, double* d_G,
                   void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);
/* bf16 storage path (BASELINE config 5; the reference fixes its dtype at core/ndmps.py:56).
 * ndmps_gemm_bf16: C (m, n) = A (m, k) op(B), op(B) = B (k, n) for transB == 0 and B^T with B (n, k) for
 * transB == 1; A, B, C bf16 row-major, fp32 accumulation on v_mfma_f32_32x32x16_bf16.  d_ws:
 * ndmps_gemm_bf16_workspace_bytes(transB, n, k) bytes (a (k, n) right operand is transposed first). */
int64_t ndmps_gemm_bf16_workspace_bytes(int transB, int64_t n, int64_t k);
int ndmps_gemm_bf16(int transB, int64_t m, int64_t n, int64_t k, const void* d_A, int64_t lda,
                    const void* d_B, int64_t ldb, void* d_C, int64_t ldc, void* d_ws, int64_t ws_bytes,
                    ndmps_stream_t stream);
/* The plan a dense product would launch by, for tests and tools: host arithmetic only, no GPU call; ndmps_sgemm,
 * ndmps_dgemm, their _batched twins and ndmps_gemm_bf16 launch by the same plan.  elem: 0 fp32, 1 bf16, 2 fp64 (bf16
 * takes transA == 0 only).  mis_a, mis_b, mis_c: the operands' addresses modulo 64, in bytes (a batch: the bitwise OR
 * over its members; bf16 with transB == 0: mis_b is the workspace's, where the transposed copy is read from).
 * guarded: whether NDMPS_GEMM_GUARDED is set (the query does not read the environment).  Shapes the entry would
 * refuse are refused (NDMPS_EINVAL).  h_out receives NDMPS_GEMM_PLAN_SLOTS values:
 *    0 bm   1 bn        (block tile; 0 0 for an empty fp32 / fp64 product)
 *    2 vec              (fp32 / fp64: the launcher's test for whole aligned quads in both operands)
 *    3 va   4 vb        (what the kernel stages in quads: vec and bm * 16 / 256 resp. bn * 16 / 256 a multiple of 4)
 *    5 grid_x   6 grid_y  (fp32 / fp64: row blocks, column blocks; bf16: column blocks, row blocks of the first launch)
 *    7 inner_a  8 inner_b (row / column blocks whose full k-tiles come by the straight-line fetch: 0 under guarded)
 *    9 vec_in  10 vec_out  11 transposes   (bf16: 16-byte loads, 16-byte stores, a (k, n) right operand copied first)
 *   12 launches           (0: m == 0 or n == 0, nothing runs; bf16: one per 65535 row tiles) */
#define NDMPS_GEMM_PLAN_SLOTS 13
int ndmps_gemm_plan_query(int elem, int transA, int transB, int64_t m, int64_t n, int64_t k, int64_t lda, int64_t ldb,
                          int64_t ldc, int64_t mis_a, int64_t mis_b, int64_t mis_c, int guarded, int64_t* h_out);
/* The same for `batch` matrices of one shape in ONE launch (m >= 256 and n >= 128, or 64 <= n < 128 with at least
 * two matrices: _workspace_bytes returns 0 for shapes without a group-wide launch; what a lockstep group of
 * volumes needs at a site of the sweep, core/ndmps.py:74 per volume in the reference): h_A is a HOST array of
 * device pointers, G of matrix b goes to d_G + b * stride_G.  _indexed: element (r, c) of matrix b is
 * h_base[b][d_row_off[r] + d_col_off[c]] (see ndmps_gram_indexed_f32). */
int64_t ndmps_gram_batched_workspace_bytes(int batch, int64_t m, int64_t n);
int ndmps_gram_batched_f32(int batch, const float* const* h_A, int64_t m, int64_t n, int64_t lda, double* d_G,
                           int64_t stride_G, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_gram_batched_bf16(int batch, const void* const* h_A, int64_t m, int64_t n, int64_t lda, double* d_G,
                            int64_t stride_G, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_gram_batched_indexed_f32(int batch, const float* const* h_base, int64_t m, int64_t n,
                                   const int64_t* d_row_off, const int64_t* d_col_off,
                                   const int32_t* d_col_perm, double* d_G, int64_t stride_G, void* d_ws,
                                   int64_t ws_bytes, ndmps_stream_t stream);
/* The plan a Gram call would run by, for tests and tools: host arithmetic only, no GPU call, no effect on any launch.
 * elem: 0 fp32, 1 bf16, 2 fp64; gathered: the operand comes through offset tables; batched: the call comes through
 * an ndmps_gram_batched_* entry.  The NDMPS_GRAM_* switches are read as a launch would read them.  h_out receives
 * NDMPS_GRAM_PLAN_SLOTS values (fields of routes the plan does not take are 0):
 *    0 route: 0 none, 1 Small, 2 Tiles16, 3 Tiles64, 4 Tiles128, 5 Tiles64Batched, 6 Stream64
 *    1 small_blocks                                     (Small: workgroups of the launch)
 *    2 T   3 n_tiles   4 n_slabs   5 rows_per_slab      (Tiles16, Tiles64, Tiles64Batched, Stream64: tiles of (16 T)^2)
 *    6 tiles_1d   7 slabs_off   8 slabs_diag   9 rows_off   10 rows_diag   11 xcd   12 slots      (Tiles128)
 *   13 workspace_bytes                                  (what the size query of the entry returns) */
#define NDMPS_GRAM_PLAN_SLOTS 14
int ndmps_gram_plan_query(int elem, int batch, int64_t m, int64_t n, int gathered, int batched, int64_t* h_out);

/* G = A^T A for a bf16 matrix A (products exact, fp64 accumulation); workspace as ndmps_gram_f32 */
int ndmps_gram_bf16(const void* d_A, int64_t m, int64_t n, int64_t lda, double* d_G, void* d_ws,
                    int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_convert_bf16_to_f32(const void* d_x, int64_t n, float* d_y, ndmps_stream_t stream);
int ndmps_convert_f32_to_bf16(const float* d_x, int64_t n, void* d_y, ndmps_stream_t stream);
/* symmetric eigen-decomposition (block two-sided Jacobi, fp64): G = V diag(w) V^T,
 * w descending, eigenvectors in the COLUMNS of V, each with its largest-magnitude
 * component positive (the first one on ties).  Only the symmetric part 0.5 (G + G^T) of the input is
 * decomposed.  d_G is destroyed.  Synchronises the stream.
 * Thresholds: a sweep that visits no |a_pq| above rel_tol * max|a_ii| ends the iteration, and an |a_pq| at or
 * below 1e-19 * max|a_ii| is not rotated -- both are relative to the largest DIAGONAL entry of the input, not
 * to its norm (finding the norm would cost every solve a pass over n^2 entries).  Every caller passes a
 * positive semi-definite matrix, for which max|a_ii| is the norm within a factor n.  Indefinite matrices
 * whose diagonal stays within a factor 8 of max|lambda| are inside the contract and tested
 * (tests/jacobi_cases.py).  For a symmetric matrix whose diagonal is small against its off-diagonal
 * entries the thresholds fall below the rounding of the matrix (they are 0 for a zero diagonal):
 * convergence within the limit of 40 sweeps is not promised, and the call may end with NDMPS_ENOCONV.
 * Nothing depends on the absolute scale: a power of two in front of G changes no bit of V. */
int64_t ndmps_syevj_workspace_bytes(int64_t n);
int ndmps_syevj_f64(double* d_G, int64_t n, double* d_V, double* d_w, void* d_ws,
                    int64_t ws_bytes, int* h_sweeps, ndmps_stream_t stream);
/* batch of independent eigenproblems solved in lockstep (one launch sequence for all):
 * matrix b is d_G + b*stride_G, n_b x n_b (ld n_b); outputs likewise.  Same conventions. */
int64_t ndmps_syevj_batched_workspace_bytes(int64_t n_max, int batch);
int ndmps_syevj_batched_f64(int batch, double* d_G, int64_t stride_G, const int64_t* h_n, double* d_V,
                            int64_t stride_V, double* d_w, int64_t stride_w, void* d_ws,
                            int64_t ws_bytes, int* h_sweeps, ndmps_stream_t stream);
/* same with an explicit convergence threshold: a sweep with no |a_pq| above rel_tol * max|a_ii|
 * ends the iteration (ndmps_syevj_*_f64 use 1e-15; the fp32 sweep uses kSweepEigTol, tt.hip) */
int ndmps_syevj_batched_tol_f64(int batch, double* d_G, int64_t stride_G, const int64_t* h_n,
                                double* d_V, int64_t stride_V, double* d_w, int64_t stride_w,
                                double rel_tol, void* d_ws, int64_t ws_bytes, int* h_sweeps,
                                ndmps_stream_t stream);
/* two-phase form (used by the sweep): eigenvalues first -- the caller derives the kept rank of every
 * matrix from them -- then only the first h_k[b] eigenvectors (columns 0..k-1 of V).  Same arguments
 * in both calls; d_ws must stay untouched in between.  For batches of matrices up to 896 the solver
 * does not update V per step: it records every step's rotation blocks in d_ws and replays them on the
 * k wanted columns held in LDS. */
int ndmps_syevj_batched_values_f64(int batch, double* d_G, int64_t stride_G, const int64_t* h_n,
                                   double* d_V, int64_t stride_V, double* d_w, int64_t stride_w,
                                   double rel_tol, void* d_ws, int64_t ws_bytes, int* h_sweeps,
                                   ndmps_stream_t stream);
int ndmps_syevj_batched_vectors_f64(int batch, double* d_G, int64_t stride_G, const int64_t* h_n,
                                    double* d_V, int64_t stride_V, double* d_w, int64_t stride_w,
                                    const int64_t* h_k, void* d_ws, int64_t ws_bytes,
                                    ndmps_stream_t stream);

/* Leading k eigenpairs by a direct method (Householder tridiagonalisation, multi-section on the Sturm
 * sequence, inverse iteration with a Cholesky-QR of the block, reflectors replayed on the k columns): the
 * path of the bond-capped sweep, where k = chi <= 128 of n = d chi <= 4096 are wanted (replaces the thin SVD
 * quimb's from_dense calls per site, core/ndmps.py:74).  Same conventions as ndmps_syevj_*: w descending,
 * eigenvector c in column c of V (ld n), largest-magnitude component positive.  Two phases like the Jacobi
 * pair above; both are asynchronous on `stream` (vectors synchronises only when h_status is given;
 * h_status[b] != 0: the orthonormalisation of matrix b broke down).
 * The two-phase calls take any k_max <= ndmps_syevd_topk_max_k_wide() (= every eigenpair of the largest order): the
 * exact sweeps and compress() want all eigenpairs above a cutoff (core/ndmps.py:74,104-106: dgesdd through quimb).
 * Above ndmps_syevd_topk_max_k() wanted vectors the eigenvectors of T are iterated in column blocks of 128 and
 * orthonormalised across the chip (Gram matrix on the fp64 MFMA, blocked Cholesky, one-launch triangular solve:
 * csrc/eig_wide.inc), and so are the vectors of one or two matrices of order >= 1024.  Tridiagonalisation: orders up to
 * 2048 whose teams fit the chip together stay resident in registers for all columns (one launch); above that, panel by
 * panel (csrc/eig_panel.inc) with the last 2048 / 1024 / 512 columns handed to the resident kernel. */
int64_t ndmps_syevd_topk_max_n(void);
int64_t ndmps_syevd_topk_max_k(void);
int64_t ndmps_syevd_topk_max_k_wide(void);
int64_t ndmps_syevd_topk_workspace_bytes(int64_t n_max, int batch, int64_t k_max);
/* byte offset, inside the workspace, of 16 int64 wall-clock marks (100 MHz) per matrix left by the vectors
 * phase (profiling aid, tools/trd_probe.py) */
int64_t ndmps_syevd_topk_stamps_offset(int64_t n_max, int batch, int64_t k_max);
/* TEST HOOK: where ndmps_syevd_topk_values_f64 leaves the tridiagonalisation Q^T A Q = T of A = (G + G^T) / 2 in the
 * workspace (tests/trd_cases.py).  h_out[0..3] = byte offsets of Vh, tau, d and e, h_out[4] = lda in doubles (n_max
 * rounded up to 2); member b lies b * n_max * lda (Vh) and b * n_max (tau, d, e) doubles further on.  Host arithmetic
 * only, no GPU call, no effect on any launch; NDMPS_TRD_BAND / _SYM are read as _workspace_bytes reads them (they do
 * not move these buffers).  For a member of order n, by every one-stage reduction:
 *   Q = H_0 H_1 ... H_{n-2},  H_j = I - tau[j] v_j v_j^T,  v_j = row j of Vh (lda doubles per row);
 *   v_j is 0.0 at the indices 0 .. j, exactly 1.0 at j + 1, and 0.0 at n .. lda - 1; tau[j] is 0 (H_j = I) or in [1, 2];
 *   d[j] = T[j][j], e[j] = T[j + 1][j]; e[n - 1] = tau[n - 1] = 0 and row n - 1 of Vh is zero.
 * A column whose part below the diagonal has a norm under 2^-450 is taken for zero (H_j = I): the reduction squares
 * entries without rescaling, and matrices are expected within 2^+-250.
 * The two-stage reductions (NDMPS_TRD_BAND) leave d and e alike; their Vh holds the block reflectors of the first
 * stage only, in another format. */
int ndmps_syevd_topk_reduction_offsets(int64_t n_max, int batch, int64_t k_max, int64_t* h_out);
/* Cholesky factor S = L L^T of a symmetric positive definite matrix (lower triangle read, L with zeros above written in
 * place; blocked, fp64 MFMA): the square root compress() needs of G2 = T2 T2^T (core/ndmps.py:104-106; quimb takes an LQ of
 * T2 there).  d_scratch: ndmps_potrf_scratch_elems(n) doubles.  Synchronises; *h_status = 1: not positive definite. */
int64_t ndmps_potrf_scratch_elems(int64_t n);
int ndmps_potrf_lower_f64(double* d_S, int64_t n, double* d_scratch, int* h_status, ndmps_stream_t stream);
int ndmps_syevd_topk_values_f64(int batch, const double* d_G, int64_t stride_G, const int64_t* h_n,
                                double* d_V, int64_t stride_V, double* d_w, int64_t stride_w,
                                int64_t k_max, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_syevd_topk_vectors_f64(int batch, const int64_t* h_n, const int64_t* h_k, int64_t k_max,
                                 void* d_ws, int64_t ws_bytes, int* h_status, ndmps_stream_t stream);
/* The resident tridiagonalisation (orders 129..2048, one launch for all columns of every matrix) makes the workgroups
 * of a matrix wait for each other; every wait is bounded (3 s) and a team that gave up leaves status 2.
 * _recover_f64: call after _values_f64 with the same batch / sizes / workspace where the host synchronises anyway:
 * waits for `stream`; if any matrix carries status 2, phase 1 is done again for the batch on the per-column / panel launches
 * (asynchronous), *h_recovered (may be NULL) = 1.  _set_team(0 / 1): resident launch off / on for the calling host
 * thread, returns the previous setting.  _team_fallbacks: how often a resident launch was given up and redone
 * (process-wide); _note_team_fallback: for callers that repeat a sequence of their own.
 * ndmps_debug_inject_team_abort(n): TEST HOOK -- the next n resident launches are replaced by what an aborted one
 * leaves behind (status 2, reduction not done), without the 3 s wait.
 * _team_slots(order): workgroups of the resident kernel that takes matrices of `order` (<= 512, <= 1024, <= 2048) the
 * current device keeps resident at once (occupancy x compute units); a batch whose teams -- order / 8 workgroups per
 * matrix -- exceed it takes another route (more launches, the panel-blocked reduction); 0 on error. */
int ndmps_syevd_topk_recover_f64(int batch, const int64_t* h_n, int64_t k_max, void* d_ws, int64_t ws_bytes,
                                 int* h_recovered, ndmps_stream_t stream);
int ndmps_syevd_topk_set_team(int enabled);
/* Per host thread: 1 = the caller keeps several batches in flight on different streams (core/batch.py lanes): batches of five
 * to eight order-512 matrices then use 32-column blocks -- a quarter of the workgroup slots and half a turn, so the
 * reductions of consecutive batches overlap -- instead of the 8-column blocks that are fastest for ONE batch on an empty GPU
 * (one to four matrices keep them: their narrow launch fits half the slots).
 * Returns the previous setting.  No counterpart in the reference (LAPACK's dgesdd inside quimb, core/ndmps.py:74). */
int ndmps_syevd_topk_set_streamed(int streamed);
int64_t ndmps_syevd_topk_team_fallbacks(void);
int ndmps_syevd_topk_team_slots(int64_t order);
int ndmps_syevd_topk_note_team_fallback(void);
/* The launches a solve of `batch` matrices of the orders h_n with k_max eigenpairs would make, for tests, tools and
 * callers that must know which kernel ran: answered from the solver's own planning function (trd_route), host arithmetic
 * only, no effect on any launch.  The NDMPS_TRD_* / NDMPS_ORTHO_* / NDMPS_BACK_* switches are read as a call would read
 * them.  team_enabled, streamed: the settings of _set_team / _set_streamed to plan for, -1 = the calling thread's current
 * ones (a recovery plans with team_enabled = 0).  h_slots[3]: the _team_slots of orders 512, 1024 and 2048; NULL asks the
 * current device -- with h_slots given the call makes no GPU call.  Phase 2 is planned for ranks up to min(k_max, n).
 * h_out receives NDMPS_EIG_ROUTE_SLOTS values (fields of routes the plan does not take are 0):
 *    0 reduction: 0 Columns (one launch per column), 1 Band2, 2 Band4 (two-stage), 3 Team (resident, orders <= 512),
 *      4 BigTeam (resident, orders 513 .. 2048), 5 Panel, 6 PanelHybrid (panels, then the resident kernel)
 *    1 hand-over width of PanelHybrid (2048, 1024 or 512 last columns)
 *    2 resident kernel: 0 none, 1 8-column tagged blocks with 2 rows per thread, 2 32-column blocks meeting at a counter,
 *      3 half storage, 4 / 5 8-column tagged blocks with 4 / 8 rows per thread, 6 / 7 dense -> band of width 2 / 4
 *    3 order the resident kernel reduces   4 workgroups per team   5 matrices per launch   6 dynamic LDS bytes
 *    7 placed XCD by XCD   8 paired on the CUs   9 takes half the device-side turn (0: the whole turn)
 *   10 column launches: columns per block (8 / 32)   11 rows per thread   12 number of launches
 *   13 columns the panels leave (Panel: 128)   14 the tail finds the stored half only   15 tail: 0 none (bulge chase),
 *      1 registers, 2 LDS   16 panel launches replayed from a cached graph
 *   17 inverse iteration: columns per block   18 its ablation bits (NDMPS_INVIT_DBG)
 *   19 orthonormalisation: 0 chip-wide with the rank read on the device, 1 chip-wide, 2 one workgroup (<= 64 vectors),
 *      3 one workgroup in blocks of 64, 4 one workgroup column by column
 *   20 back-transformation: 0 rows dealt to the lanes, 1 rows dealt to the chip, 2 blocks of 64 reflectors on the MFMA
 *   21 SEG  22 R  23 RB  24 WYB of the lane-dealt kernel   25 T factors of 1 / 2: 1 on the caller's stream, 2 on the side stream
 *   26 workspace bytes   27 stamps offset   28 / 29 offsets of the descriptors and of the hand-over's descriptors
 *   30 padded vector count the chip-wide buffers hold (0: none)   31 doubles per matrix of the row-dealt partials */
#define NDMPS_EIG_ROUTE_SLOTS 32
int ndmps_syevd_topk_route_query(int batch, const int64_t* h_n, int64_t k_max, int team_enabled, int streamed,
                                 const int* h_slots, int64_t* h_out);
int ndmps_debug_inject_team_abort(int launches);
/* TEST HOOK: the cross-lane sums the tridiagonalisation kernels fold with (csrc/lanes.h: DPP moves and permlane swaps in
 * place of ds_bpermute), on one wave: d_out[12][64] = the sums of d_in[64] over 2, 4, 8, 16, 32, 64 adjacent lanes, then
 * over the lanes with equal lane % 1, 2, 4, 8, 16, 32 -- every lane holds its group's sum. */
int ndmps_debug_lane_sums_f64(const double* d_in, double* d_out, ndmps_stream_t stream);
/* Phase 2 with the rank decided ON THE DEVICE from phase 1's eigenvalues:
 * k_b = #{i < min(k_cap, n_b) : sqrt(max(w_i, 0)) > cutoff * sqrt(max(w_0, 0))}, at least 1; k_cap <=
 * ndmps_syevd_topk_max_k(), cutoff >= 0 (cutoff >= 1 keeps one; the zero matrix keeps one, a unit vector).  Columns
 * k_b .. min(k_cap, n_b)-1 of V are zero-filled, so a caller sizes everything by k_cap and never waits for the rank.
 * Write extents, per matrix b of order n_b (a batch may mix orders below k_cap with larger ones): of V exactly the
 * columns 0 .. min(k_cap, n_b)-1 of its n_b x n_b block (ld n_b) -- no column behind them, nothing past n_b^2;
 * d_ranks[b] (device) receives k_b; d_spectra (may be NULL) the min(k_cap, n_b) leading singular values
 * sqrt(max(w_i, 0)) at b * spectra_stride -- a matrix of order n_b < k_cap has no more, and the entries from
 * min(k_cap, n_b) up to spectra_stride are left as they were; d_status (may be NULL) the breakdown flags (2, a resident
 * team that gave up, is sticky).  d_G of phase 1 is only read.  Fully asynchronous. */
int ndmps_syevd_topk_vectors_auto_f64(int batch, const int64_t* h_n, int64_t k_cap, double cutoff,
                                      int* d_ranks, double* d_spectra, int64_t spectra_stride,
                                      int* d_status, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);

/* ---------------------------------------------------------------------------------
 * MPS sweep: replaces quimb MatrixProductState.from_dense (core/ndmps.py:74).
 * Right->left, per site: unfold (prod_{j<i} d_j) x (d_i chi_{i+1}) -> SVD (Gram + Jacobi,
 * fp64 small-side) -> keep s_k > cutoff*s_0, at most max_bond (<=0: unlimited) -> V^T is
 * site i, U S is carried left.  Cores are written fp32 at d_cores + core_offsets[i].
 *
 * ndmps_tt_layout fills (all host arrays of L+1 entries):
 *   h_max_bonds[i]   upper bound of chi_i (chi_0 = chi_L = 1)
 *   h_core_offsets[i] element offset of core i in the arena; [L] = arena elements
 *   h_spec_offsets[i] offset of bond i's singular values in h_spectra; [L] = total
 *   *h_workspace_bytes device workspace needed by ndmps_tt_sweep_f32
 * --------------------------------------------------------------------------------- */
int ndmps_tt_layout(int L, const int64_t* h_dims, int64_t max_bond, int64_t* h_max_bonds,
                    int64_t* h_core_offsets, int64_t* h_spec_offsets,
                    int64_t* h_workspace_bytes);
/* d_dense: N fp32 in site order (output of ndmps_encode_permute); it is overwritten.
 * h_bonds_out: L+1 actual bonds; h_spectra (may be NULL): singular values per bond. */
int ndmps_tt_sweep_f32(float* d_dense, int L, const int64_t* h_dims, double cutoff,
                       int64_t max_bond, float* d_cores, const int64_t* h_core_offsets,
                       int64_t* h_bonds_out, double* h_spectra, const int64_t* h_spec_offsets,
                       void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);

/* Batch of independent volumes of the same shape (the reference loops over lists of tensors,
 * evaluation/benchmark.py:73-76): h_dense[b] / h_cores[b] are per-volume device pointers,
 * h_bonds_out is batch x (L+1), h_spectra batch x h_spec_offsets[L].  The volumes advance
 * through the sites in lockstep so each site's eigenproblems are one batched solve. */
/* 1 when the sweep for these site dims and bond cap decides the ranks on the device (every site on the direct
 * top-k solver; no host round trip between sites): cores are then written at the layout's offsets in PADDED shape
 * (max_bonds[i], d_i, max_bonds[i+1]) with zeros beyond the actual bonds reported in h_bonds_out, and the caller
 * slices them.  0: cores are compact (bonds[i], d_i, bonds[i+1]). */
int ndmps_tt_sweep_pads_cores(int L, const int64_t* h_dims, int64_t max_bond);
/* The fused fp32 sweep in two halves, for sweeps that decide their ranks on the device (ndmps_tt_sweep_pads_cores = 1,
 * L > 1): everything such a sweep needs from the host is known before it starts.
 *   ndmps_tt_sweep_batched_fused_begin_f32  ENQUEUES the whole sweep (arguments as ndmps_tt_sweep_batched_fused_f32) and the
 *       copies of ranks, solver status and kept singular values into the caller's PINNED host buffers
 *       (h_pinned_ranks: ndmps_tt_sweep_async_ints(batch, L) ints; h_pinned_spec: ndmps_tt_sweep_async_doubles(...)
 *       doubles, may be a dummy when that is 0); does not wait.  h_bonds_scratch: batch (L + 1) entries.
 *   ndmps_tt_sweep_finish  after the caller has synchronised with the stream (an event behind _begin): fills h_bonds_out
 *       and h_spectra like the one-call form, or returns the solver's error -- NDMPS_ETEAM when a resident
 *       tridiagonalisation gave up; nothing is repeated here: the volumes are intact, the caller redoes the batch with
 *       ndmps_tt_sweep_batched_fused_f32, which retries on the column launches.
 * Replaces the same MatrixProductState.from_dense (core/ndmps.py:74); the reference has no counterpart of the split (NumPy
 * is synchronous).  core/batch.py begins batch k + 1 before it reads batch k: the objects of k are built under k + 1. */
int64_t ndmps_tt_sweep_async_ints(int batch, int L);
int64_t ndmps_tt_sweep_async_doubles(int batch, int L, const int64_t* h_dims, int64_t max_bond);
int ndmps_tt_sweep_batched_fused_begin_f32(int batch, const float* const* h_volume, int L, const int64_t* h_dims,
                                           double cutoff, int64_t max_bond, float* const* h_cores,
                                           const int64_t* h_core_offsets, int64_t* h_bonds_scratch,
                                           const int64_t* d_row_off, const int64_t* d_row_off_sorted,
                                           const int32_t* d_row_order, const int64_t* d_col_off,
                                           const int32_t* d_col_perm, int64_t n_cols, void* d_ws, int64_t ws_bytes,
                                           int* h_pinned_ranks, double* h_pinned_spec, ndmps_stream_t stream);
int ndmps_tt_sweep_finish(int batch, int L, const int64_t* h_dims, int64_t max_bond, const int* h_pinned_ranks,
                          const double* h_pinned_spec, int64_t* h_bonds_out, double* h_spectra,
                          const int64_t* h_spec_offsets);
int64_t ndmps_tt_sweep_batched_workspace_bytes(int batch, int L, const int64_t* h_dims,
                                               int64_t max_bond);
int ndmps_tt_sweep_batched_f32(int batch, float* const* h_dense, int L, const int64_t* h_dims,
                               double cutoff, int64_t max_bond, float* const* h_cores,
                               const int64_t* h_core_offsets, int64_t* h_bonds_out,
                               double* h_spectra, const int64_t* h_spec_offsets, void* d_ws,
                               int64_t ws_bytes, ndmps_stream_t stream);

/* The fp32 sweep with the reshape stage fused in (core/ndmps.py:66-71 + :74): the raw Gram pass and the
 * projection of the merged trailing run read the C-order volumes through the index permutation; h_volume[b] is
 * left untouched and no site-order tensor is formed.  n_cols = ndmps_tt_merge_columns(L, dims, max_bond)
 * (0: not available for this shape / bond cap); tables from ndmps_plan_split_offsets(plan, n_cols, ...) with the
 * columns sorted by offset (d_col_off ascending and in aligned runs of four consecutive offsets, d_col_perm[c] =
 * site-order column of the c-th smallest offset). */
int64_t ndmps_tt_merge_columns(int L, const int64_t* h_dims, int64_t max_bond);
int ndmps_tt_sweep_batched_fused_f32(int batch, const float* const* h_volume, int L, const int64_t* h_dims,
                                     double cutoff, int64_t max_bond, float* const* h_cores,
                                     const int64_t* h_core_offsets, int64_t* h_bonds_out,
                                     double* h_spectra, const int64_t* h_spec_offsets,
                                     const int64_t* d_row_off, const int64_t* d_row_off_sorted,
                                     const int32_t* d_row_order, const int64_t* d_col_off,
                                     const int32_t* d_col_perm, int64_t n_cols, void* d_ws, int64_t ws_bytes,
                                     ndmps_stream_t stream);
/* d_row_off_sorted (may be NULL): the entries of d_row_off in ascending order.  A Gram matrix is a sum over rows, so
 * its kernels may visit them in any order; in ascending order of their offsets they read the volume front to back
 * (32 x 262144 x 64: 1.14 -> 0.74 ms).  d_row_order (may be NULL): d_row_off_sorted[s] = d_row_off[d_row_order[s]]; with
 * it the first projection of a 64-column merged run (bond cap 32) is the stream below, its result rows scattered to
 * their places; every other projection keeps d_row_off.
 * ndmps_sgemm_gathered64_stream_batched: C[b] (m x n, n = 32 or 64, leading dimension ldc) = A[b] W[b] with A[b] the
 * (m x 64) matrix h_A[b][d_row_sorted[s] + d_col_off[c]] (rows in ascending order of their offsets, columns in
 * aligned runs of four consecutive offsets), row s of the product stored as row d_row_order[s] of C[b]. */
int ndmps_sgemm_gathered64_stream_batched(int batch, int64_t m, int64_t n, const float* const* h_A,
                                          const int64_t* d_row_sorted, const int32_t* d_row_order,
                                          const int64_t* d_col_off, const float* const* h_B, int64_t ldb,
                                          float* const* h_C, int64_t ldc, ndmps_stream_t stream);
/* (ndmps_gram_indexed_f32:)
 * G = A^T A where element (r, c) of A is d_base[d_row_off[r] + d_col_off[c]] (wide path: n >= 64, m >= 256);
 * d_col_perm (may be NULL): entry (a, b) of the product is stored at G[d_col_perm[a]][d_col_perm[b]] -- the columns
 * were visited in the memory order of the volume, the result comes out in site order */
int ndmps_gram_indexed_f32(const float* d_base, int64_t m, int64_t n, const int64_t* d_row_off,
                           const int64_t* d_col_off, const int32_t* d_col_perm, double* d_G, void* d_ws,
                           int64_t ws_bytes, ndmps_stream_t stream);

/* The same sweep on bf16 storage: site-order tensors, carried matrices and cores are bf16 in HBM, Gram
 * matrices / eigen-decompositions / bases fp64, products fp32-accumulated on the bf16 MFMA.  Layout and
 * workspace queries are those of the fp32 sweep (offsets count elements; its workspace size is an upper bound). */
int ndmps_tt_sweep_batched_bf16(int batch, void* const* h_dense, int L, const int64_t* h_dims,
                                double cutoff, int64_t max_bond, void* const* h_cores,
                                const int64_t* h_core_offsets, int64_t* h_bonds_out,
                                double* h_spectra, const int64_t* h_spec_offsets, void* d_ws,
                                int64_t ws_bytes, ndmps_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Bond truncation: replaces quimb tensor_compress_bond(t1, t2, cutoff, cutoff_mode="rel")
 * (core/ndmps.py:104-106; reduced=True, absorb="both").  t1 (chi_l, d1, chi),
 * t2 (chi, d2, chi_r) fp32.  New cores are written to d_new1 / d_new2 (sized for chi),
 * *h_new_chi receives the kept bond; h_s (may be NULL) receives chi singular values.
 * --------------------------------------------------------------------------------- */
int64_t ndmps_compress_bond_workspace_bytes(int64_t chi_l, int64_t d1, int64_t chi, int64_t d2,
                                            int64_t chi_r);
int ndmps_compress_bond_f32(const float* d_t1, const float* d_t2, int64_t chi_l, int64_t d1,
                            int64_t chi, int64_t d2, int64_t chi_r, double cutoff,
                            int64_t max_bond, float* d_new1, float* d_new2, int64_t* h_new_chi,
                            double* h_s, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Chain contraction: replaces `mps ^ ...` (core/ndmps.py:140), cumulative left->right.
 * h_cores: host array of L device pointers; h_bonds: L+1 bonds.  d_dense receives the
 * (d_0..d_{L-1}) tensor, N fp32.
 * --------------------------------------------------------------------------------- */
int64_t ndmps_chain_workspace_bytes(int L, const int64_t* h_dims, const int64_t* h_bonds);
int ndmps_chain_contract_f32(int L, const int64_t* h_dims, const int64_t* h_bonds,
                             const float* const* h_cores, float* d_dense, void* d_ws,
                             int64_t ws_bytes, ndmps_stream_t stream);

/* Chain contraction that writes the C-order VOLUME: the inverse index permutation (core/ndmps.py:144-148)
 * rides on the last product of the chain, every element goes from the MFMA accumulator to its voxel; the
 * site-order tensor is never written.  n_cols = ndmps_chain_tail_columns(L, dims) (0: this chain has no
 * pre-contracted tail, use ndmps_chain_contract_f32 + ndmps_decode_permute); tables from
 * ndmps_plan_split_offsets(plan, n_cols, row_off, col_off): d_col_off = col_off sorted ascending, d_col_perm[c] =
 * the site-order column with the c-th smallest offset. */
int64_t ndmps_chain_tail_columns(int L, const int64_t* h_dims);
int ndmps_plan_split_offsets(const ndmps_plan_t* plan, int64_t n_cols, int64_t* h_row_off,
                             int64_t* h_col_off);
int ndmps_chain_contract_scatter_f32(int L, const int64_t* h_dims, const int64_t* h_bonds,
                                     const float* const* h_cores, float* d_out,
                                     const int64_t* d_row_off, const int64_t* d_col_off,
                                     const int32_t* d_col_perm, int64_t n_cols, void* d_ws,
                                     int64_t ws_bytes, ndmps_stream_t stream);
/* The same for a list of MPS over the same sites (the reference reconstructs a list with a Python loop,
 * evaluation/benchmark.py:80-100): volume b has bonds h_bonds[b (L + 1) ..], cores h_cores[b L ..] and is written
 * to h_out[b].  MPS that share their bonds go through the chain together (one batched launch per stage, each in
 * its own slice of d_ws); otherwise the volumes are contracted in turn.  d_ws >=
 * ndmps_chain_batched_workspace_bytes(batch, L, dims, bonds). */
int64_t ndmps_chain_batched_workspace_bytes(int batch, int L, const int64_t* h_dims, const int64_t* h_bonds);
int ndmps_chain_contract_scatter_batched_f32(int batch, int L, const int64_t* h_dims, const int64_t* h_bonds,
                                             const float* const* h_cores, float* const* h_out,
                                             const int64_t* d_row_off, const int64_t* d_col_off,
                                             const int32_t* d_col_perm, int64_t n_cols, void* d_ws,
                                             int64_t ws_bytes, ndmps_stream_t stream);
/* The plan a chain call would run by, for tests and tools: host arithmetic only, no GPU call, no effect on any launch.
 * elem: 0 fp32, 1 bf16, 2 fp64.  h_out receives NDMPS_CHAIN_PLAN_SLOTS(L) values:
 *    0 j0 (first site of the pre-contracted tail, L: none)   1 tail columns (0: none)   2 number of products (L - 1)
 *    3 left_elems   4 tail_elems (capacities of ws_left / of either tail buffer)   5 workspace bytes
 * then, per product in the order of the launches, C (m x n) = A (m x k) B (k x n):
 *    kind (0 tail, 1 left, 2 final)   m   n   k   A   B   C   spare
 * with buffers named as: i >= 0 core i, -1 ws_left, -2 ws_tail0, -3 ws_tail1, -4 the output, -5 none.  spare: the
 * tail buffer the final product's right operand is gathered into by the scatter entries. */
#define NDMPS_CHAIN_PLAN_SLOTS(L) (6 + 8 * ((L) - 1))
int ndmps_chain_plan_query(int elem, int L, const int64_t* h_dims, const int64_t* h_bonds, int64_t* h_out);
/* Value statistics of the volume a chain decodes to, and its error against an original, WITHOUT the volume: the chain
 * is contracted as ndmps_chain_contract_* contracts it, but the last product -- the only one that touches N
 * elements -- hands its accumulator tiles to a reducing epilogue instead of storing them (csrc/valstat.hip; the product kernel: csrc/valstat_device.h).  fp32
 * cores on the fp32 MFMA, fp64 cores on the fp64 MFMA.  Every call checks its arguments before its first launch,
 * reads its small result record back once and returns with the stream synchronised.  The same inputs give the same
 * bits: sums are fp64, folded in a fixed order, and only integers are added atomically.
 *
 * Workspace: ndmps_valstat_workspace_bytes(L, dims, bonds, elem_bytes (4 or 8), n_bins) = the decode workspace
 * (ndmps_chain_workspace_bytes*) + a second left buffer + the reduction scratch (partial records, the result, and
 * for n_bins > 0 the histogram's n_bins + 3 counters and n_bins + 1 edges); 0 for bad arguments.  d_ws must be
 * 256-byte aligned.  n_bins = 0 serves the moments and error calls.  For a chain without a pre-contracted tail (and for
 * L == 1) the decode plan's left buffer has N elements, and so has the second one: no memory is saved there.
 *
 * ndmps_valstat_plan_query: the plan, for tests and tools (host arithmetic only).  elem: 0 fp32, 2 fp64.  h_out
 * receives NDMPS_VALSTAT_PLAN_SLOTS(L) values:
 *    0 j0   1 tail columns   2 number of products (L - 1)   3 left_elems   4 tail_elems
 *    5 decode workspace bytes   6 second left buffer bytes   7 reduction scratch bytes   8 workspace bytes (5 + 6 + 7)
 * then the L - 1 products as ndmps_chain_plan_query lists them (same products, same order), and last the product that
 * is reduced (the last of them again; for L == 1 core 0 as a 1 x d_0 matrix behind a unit left operand).  Buffers
 * as there, and: -6 the second left buffer (wherever the decode plan uses the output as an intermediate),
 * -7 the unit operand; the reduced product's destination is -5 (none).
 *
 * moments: h_stats = {min, max, sum, sum of squares} over the voxels with clip_lo <= v <= clip_hi (-inf, +inf: all
 * of them; a narrower range is how a quantile search looks inside its bracket), h_counts = {voxels, NaN voxels,
 * voxels inside the clip range}.  NaN voxels are counted and take no part in the statistics (none taken: min = +inf,
 * max = -inf).
 * histogram: h_edges (HOST, n_bins + 1 values in the element type, ascending, no NaN; 1 <= n_bins <= 4096) as
 * numpy.histogram reads them: bin b holds edges[b] <= v < edges[b + 1], the last bin includes its right edge.
 * h_counts receives n_bins + 3 values: the bins, then the voxels below edges[0], above edges[n_bins], and NaN.
 * Binning is exact for the computed v (binary search in the edge table).
 * error: d_ref is the original as a C-order volume in the element type; d_row_off / d_col_off / d_col_perm are the
 * tables of ndmps_plan_split_offsets(plan, n_cols, ...) with the columns sorted by offset, as the fused decode takes
 * them, n_cols = ndmps_chain_tail_columns, or the last site's dimension for a chain without a tail.
 * h_stats = {sum (v - y)^2, max |v - y|, sum y^2, max y}, h_counts = {voxels, voxels whose v - y is NaN (left out
 * of the four), 0}. */
#define NDMPS_VALSTAT_PLAN_SLOTS(L) (9 + 8 * (L))
int64_t ndmps_valstat_workspace_bytes(int L, const int64_t* h_dims, const int64_t* h_bonds, int64_t elem_bytes,
                                      int64_t n_bins);
int ndmps_valstat_plan_query(int elem, int L, const int64_t* h_dims, const int64_t* h_bonds, int64_t n_bins,
                             int64_t* h_out);
int ndmps_valstat_moments_f32(int L, const int64_t* h_dims, const int64_t* h_bonds, const float* const* h_cores,
                              double clip_lo, double clip_hi, double* h_stats, int64_t* h_counts, void* d_ws,
                              int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_valstat_moments_f64(int L, const int64_t* h_dims, const int64_t* h_bonds, const double* const* h_cores,
                              double clip_lo, double clip_hi, double* h_stats, int64_t* h_counts, void* d_ws,
                              int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_valstat_histogram_f32(int L, const int64_t* h_dims, const int64_t* h_bonds, const float* const* h_cores,
                                const float* h_edges, int n_bins, int64_t* h_counts, void* d_ws, int64_t ws_bytes,
                                ndmps_stream_t stream);
int ndmps_valstat_histogram_f64(int L, const int64_t* h_dims, const int64_t* h_bonds, const double* const* h_cores,
                                const double* h_edges, int n_bins, int64_t* h_counts, void* d_ws, int64_t ws_bytes,
                                ndmps_stream_t stream);
int ndmps_valstat_error_f32(int L, const int64_t* h_dims, const int64_t* h_bonds, const float* const* h_cores,
                            const float* d_ref, const int64_t* d_row_off, const int64_t* d_col_off,
                            const int32_t* d_col_perm, int64_t n_cols, double* h_stats, int64_t* h_counts, void* d_ws,
                            int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_valstat_error_f64(int L, const int64_t* h_dims, const int64_t* h_bonds, const double* const* h_cores,
                            const double* d_ref, const int64_t* d_row_off, const int64_t* d_col_off,
                            const int32_t* d_col_perm, int64_t n_cols, double* h_stats, int64_t* h_counts, void* d_ws,
                            int64_t ws_bytes, ndmps_stream_t stream);
/* ---- Extremes along axes and the place of the global extreme, from the cores (csrc/axisext.hip, core/axisext.py).
 * The same chain contraction and the same workspace as the value statistics (ndmps_valstat_workspace_bytes with
 * n_bins = 0); the last product's epilogue turns every voxel into an unsigned key whose integer order is the order of
 * the values and combines the keys of one output cell with integer atomic maxima, so the same inputs give the same
 * bits.  NaN voxels take no part.  op: 0 max, 1 min.  Every argument check returns before the first launch.
 *
 * axisext: the projected array has out_numel cells; element (r, c) of the last product belongs to cell
 * d_row_out[r] + d_col_out[c] (an offset outside [0, out_numel) updates nothing) and has the coordinate
 * d_row_idx[r] + d_col_idx[c] along the reduced axis.  The column tables are in the order d_col_perm (site-order
 * column of the c-th table entry), which must make columns of equal d_col_out adjacent; n_cols as for the error
 * entry.  d_values (device, out_numel elements) receives the extremes, NaN for a cell nothing reached.  d_row_idx,
 * d_col_idx and d_index (device, out_numel int64) are given together or all NULL: d_index receives the smallest
 * coordinate at which the extreme sits, -1 where d_values is NaN.  The call returns without synchronising.
 * argext: the tables of ndmps_plan_split_offsets as the error entry takes them; *h_value receives the extreme of the
 * whole volume and *h_flat_index the smallest C-order index it sits at (NaN and -1 for a volume of NaN only).
 * Returns with the stream synchronised. */
int ndmps_axisext_f32(int L, const int64_t* h_dims, const int64_t* h_bonds, const float* const* h_cores, int op,
                      const int64_t* d_row_out, const int64_t* d_col_out, const int32_t* d_col_perm, int64_t n_cols,
                      const int32_t* d_row_idx, const int32_t* d_col_idx, int64_t out_numel, float* d_values,
                      int64_t* d_index, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_axisext_f64(int L, const int64_t* h_dims, const int64_t* h_bonds, const double* const* h_cores, int op,
                      const int64_t* d_row_out, const int64_t* d_col_out, const int32_t* d_col_perm, int64_t n_cols,
                      const int32_t* d_row_idx, const int32_t* d_col_idx, int64_t out_numel, double* d_values,
                      int64_t* d_index, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_argext_f32(int L, const int64_t* h_dims, const int64_t* h_bonds, const float* const* h_cores, int op,
                     const int64_t* d_row_off, const int64_t* d_col_off, const int32_t* d_col_perm, int64_t n_cols,
                     double* h_value, int64_t* h_flat_index, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_argext_f64(int L, const int64_t* h_dims, const int64_t* h_bonds, const double* const* h_cores, int op,
                     const int64_t* d_row_off, const int64_t* d_col_off, const int32_t* d_col_perm, int64_t n_cols,
                     double* h_value, int64_t* h_flat_index, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);
/* ---- The voxels inside or outside an interval, or NaN, as a list, from the cores (csrc/select.hip, core/select.py).
 * The chain contraction and the workspace of the value statistics (ndmps_valstat_workspace_bytes with n_bins = 0) and
 * the tables of the error entry.  mode 0: lo <= v <= hi; 1: v is not NaN and not inside; 2: v is NaN (lo and hi are
 * not read).  lo and hi are cast to the element type and compared with the computed voxel in that type, as the
 * clipped moments pass compares, so its count is the length of the list.  A match takes the next free slot s of a
 * 64-bit cursor and writes d_index[s] = d_row_off[r] + d_col_off[c] (the flat C-order index; an offset outside the
 * volume matches nothing) and d_values[s] = v when s < capacity; matches at and beyond capacity are counted and not
 * written, so nothing outside the first `capacity` slots is touched (capacity 0: d_index and d_values may be NULL).
 * *h_total receives the number of matches.  The slots are in order of arrival: sort by index for a fixed result.
 * Every argument check returns before the first launch; returns with the stream synchronised. */
int ndmps_select_f32(int L, const int64_t* h_dims, const int64_t* h_bonds, const float* const* h_cores, int mode,
                     double lo, double hi, const int64_t* d_row_off, const int64_t* d_col_off, const int32_t* d_col_perm,
                     int64_t n_cols, int64_t capacity, int64_t* d_index, float* d_values, int64_t* h_total, void* d_ws,
                     int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_select_f64(int L, const int64_t* h_dims, const int64_t* h_bonds, const double* const* h_cores, int mode,
                     double lo, double hi, const int64_t* d_row_off, const int64_t* d_col_off, const int32_t* d_col_perm,
                     int64_t n_cols, int64_t capacity, int64_t* d_index, double* d_values, int64_t* h_total, void* d_ws,
                     int64_t ws_bytes, ndmps_stream_t stream);
/* ---- Statistics per label of an atlas, from the cores (csrc/labelstat.hip, core/labelstat.py).
 * The chain contraction of the value statistics; the last product runs twice over the same operands.  The first run is
 * the moments pass, whose minimum and maximum fix on the device the two power-of-two scales s and s2; the second hands
 * every voxel v with its label d_labels[d_row_off[r] + d_col_off[c]] (the tables of the error entry; an offset outside
 * the volume reads nothing) to an epilogue that adds llrint(v 2^s) and llrint(v v 2^s2) into 64-bit integers and takes
 * integer maxima of order-preserving keys for min and max.  Only integers are added atomically: the same inputs give
 * the same bits.  NaN voxels are counted per label and take no part in the rest; an infinite voxel is refused with
 * NDMPS_EINVAL ("label statistics need finite voxels").  A label outside [0, n_labels) is counted in `outside`.
 *
 * The scales (ndmps_labelstat_scales, host arithmetic only; the device applies the same function): with
 * nb = ceil(log2 numel) and maxabs < 2^e by frexp, s = 61 - nb - e; s2 = 61 - nb - e2 with e2 from the fp64 product
 * maxabs * maxabs (2 e where that product leaves the fp64 range); both clamped to [-1000, 1000]; maxabs = 0 gives
 * s = s2 = 0.  Then numel * |v| 2^s <= 2^61: no sum can overflow.
 *
 * Workspace: ndmps_labelstat_workspace_bytes = ndmps_valstat_workspace_bytes(..., n_bins = 0) + the label table,
 * 8 * (6 * n_labels + 5) bytes rounded up to 256: six 64-bit slots per label (sum, sum of squares, count, NaN count,
 * min key, max key), then outside, overflow, s, s2 and the non-finite flag.  0 for bad arguments.
 * d_labels: device, C order of the volume, label_elem_bytes 1 (uint8), 2 (int16) or 4 (int32).  1 <= n_labels <= 4096;
 * more than 1024 labels run the labelled pass once per window of 1024.
 * Results (HOST): h_sums[n_labels] the integer sums (value = h_sums[l] 2^-s), h_sumsq[n_labels] (2^-s2),
 * h_counts[2 n_labels] the non-NaN counts then the NaN counts, h_minmax[2 n_labels] the minima then the maxima as
 * doubles (NaN where the count is 0), h_info = {outside, s, s2, voxels}.  Returns with the stream synchronised. */
int64_t ndmps_labelstat_workspace_bytes(int L, const int64_t* h_dims, const int64_t* h_bonds, int64_t elem_bytes,
                                        int64_t n_labels);
int ndmps_labelstat_scales(double maxabs, int64_t numel, int* s, int* s2);
int ndmps_labelstat_f32(int L, const int64_t* h_dims, const int64_t* h_bonds, const float* const* h_cores,
                        const void* d_labels, int label_elem_bytes, const int64_t* d_row_off, const int64_t* d_col_off,
                        const int32_t* d_col_perm, int64_t n_cols, int n_labels, int64_t* h_sums, uint64_t* h_sumsq,
                        int64_t* h_counts, double* h_minmax, int64_t* h_info, void* d_ws, int64_t ws_bytes,
                        ndmps_stream_t stream);
int ndmps_labelstat_f64(int L, const int64_t* h_dims, const int64_t* h_bonds, const double* const* h_cores,
                        const void* d_labels, int label_elem_bytes, const int64_t* d_row_off, const int64_t* d_col_off,
                        const int32_t* d_col_perm, int64_t n_cols, int n_labels, int64_t* h_sums, uint64_t* h_sumsq,
                        int64_t* h_counts, double* h_minmax, int64_t* h_info, void* d_ws, int64_t ws_bytes,
                        ndmps_stream_t stream);
/* ---- Histograms per label of an atlas, from the cores (csrc/labelhist.hip, core/labelhist.py): the labelled reading
 * of ndmps_labelstat_* (d_labels, label_elem_bytes and the tables of the error entry; a label outside [0, n_labels)
 * is counted in `outside`) with the exact bin search of ndmps_valstat_histogram_*.  A voxel is binned against the
 * edge row of its label.  h_edges (HOST, element type): per_label == 0 one row of n_bins + 1 edges for every label,
 * per_label != 0 n_labels rows of n_bins + 1.  A row is ascending and not NaN; it need not be strictly ascending, so
 * a short row may repeat its last edge (a voxel equal to that edge lands in the last bin, which is closed on the
 * right), and -inf / +inf are legal edges.  Only integers are added atomically: the same inputs give the same bits.
 * NaN voxels are counted per label; an infinite voxel is binned like any other.
 *
 * One launch takes a window of labels whose edge rows, keys and 32-bit counters fit in 64 KiB of dynamic LDS:
 *   lds(w) = elem_bytes * ((per_label ? w : 1) * (n_bins + 1) + 2 w) + 4 w (n_bins + 3),
 * window = the largest w <= n_labels with lds(w) <= 65536 (at least 1 for n_bins <= 4096), launches =
 * ceil(n_labels / window).  More than 64 launches are refused with NDMPS_EINVAL ("use fewer bins or split the
 * atlas").  ndmps_labelhist_plan_query (host arithmetic only) writes h_out = {window, launches, lds(window), table
 * bytes} or returns that refusal; the table is 8 * (n_labels * (n_bins + 5) + 1) bytes rounded up to 256.
 *
 * Workspace: ndmps_valstat_workspace_bytes(..., n_bins = 0) + the table + the edge rows rounded up to 256; 0 for bad
 * arguments and for a call that would be refused.  1 <= n_labels <= 4096, 1 <= n_bins <= 4096.
 * Results (HOST): h_counts[n_labels * (n_bins + 3)], per label the bins, then below, above and the NaN count;
 * h_minmax[2 n_labels] the smallest and then the largest voxel inside [e[0], e[n_bins]] of each label as doubles (NaN
 * where there is none); h_info = {outside, voxels}.  Every argument check returns before the first launch; returns
 * with the stream synchronised. */
int64_t ndmps_labelhist_workspace_bytes(int L, const int64_t* h_dims, const int64_t* h_bonds, int64_t elem_bytes,
                                        int64_t n_labels, int64_t n_bins, int per_label);
int ndmps_labelhist_plan_query(int64_t elem_bytes, int64_t n_labels, int64_t n_bins, int per_label, int64_t* h_out);
int ndmps_labelhist_f32(int L, const int64_t* h_dims, const int64_t* h_bonds, const float* const* h_cores,
                        const void* d_labels, int label_elem_bytes, const int64_t* d_row_off, const int64_t* d_col_off,
                        const int32_t* d_col_perm, int64_t n_cols, int n_labels, const float* h_edges, int n_bins,
                        int per_label, int64_t* h_counts, double* h_minmax, int64_t* h_info, void* d_ws,
                        int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_labelhist_f64(int L, const int64_t* h_dims, const int64_t* h_bonds, const double* const* h_cores,
                        const void* d_labels, int label_elem_bytes, const int64_t* d_row_off, const int64_t* d_col_off,
                        const int32_t* d_col_perm, int64_t n_cols, int n_labels, const double* h_edges, int n_bins,
                        int per_label, int64_t* h_counts, double* h_minmax, int64_t* h_info, void* d_ws,
                        int64_t ws_bytes, ndmps_stream_t stream);
/* ---- Statistics of TWO chains of one shape and one factorisation, from the cores (csrc/pairstat.hip,
 * core/pairstat.py): the pair moments and the joint histogram of the two volumes, with neither written.  Both chains
 * have the site dims h_dims, so their last products have the same rows and columns (the split depends on the dims
 * alone) and differ only in k; one kernel forms both accumulator tiles of a tile index and hands the voxel pairs to
 * a reducing epilogue.  A voxel's value is computed exactly as the ndmps_valstat_* entries compute it.  fp32 or fp64,
 * both chains in the same element type.  Every call checks its arguments before its first launch, reads its result
 * back once and returns with the stream synchronised; the same inputs give the same bits.
 *
 * Workspace: ndmps_pairstat_workspace_bytes(L, dims, bonds_a, bonds_b, elem_bytes (4 or 8), bins_a, bins_b) =
 * ndmps_valstat_workspace_bytes(.., bonds_a, .., 0) + the same for bonds_b + the pair scratch (512 partial records of
 * 128 bytes, 256 bytes for the result, and for a histogram bins_a * bins_b + 2 counters and the two edge tables, each
 * rounded up to 256 bytes); bins 0, 0 serves the moments call; 0 for bad arguments.  An axis takes at most 1024
 * bins, the two together at most 16384 cells.  d_ws must be 256-byte aligned.
 *
 * ndmps_pairstat_plan_query: the plan, for tests and tools (host arithmetic only).  elem: 0 fp32, 2 fp64.  h_out
 * receives NDMPS_PAIRSTAT_PLAN_SLOTS values:
 *    0 m   1 n   2 k of a   3 k of b (the last products)   4 workspace bytes of a   5 of b
 *    6 offset of b's workspace   7 of the partial records   8 of the result   9 of the counters   10 of the edges of a
 *    11 of the edges of b   12 pair scratch bytes   13 workspace bytes
 *
 * moments: h_stats = {sum a, sum b, sum a^2, sum b^2, sum a b, sum (a - b)^2, min a, max a, min b, max b,
 * max |a - b|} over the voxels where neither value is NaN, h_counts = {their number, the voxels where either is}.
 * histogram: h_edges_a[bins_a + 1] / h_edges_b[bins_b + 1] are HOST arrays in the element type, ascending, no NaN;
 * cell (ia, ib) takes edges_a[ia] <= a < edges_a[ia + 1] and edges_b[ib] <= b < edges_b[ib + 1], the last bin of
 * either axis closed on the right (numpy.histogram2d).  h_counts[bins_a * bins_b + 2] (HOST): the cells row-major
 * (ia * bins_b + ib), then the voxels with either value out of range, then the voxels with either value NaN (NaN
 * wins over out of range). */
#define NDMPS_PAIRSTAT_PLAN_SLOTS 14
int64_t ndmps_pairstat_workspace_bytes(int L, const int64_t* h_dims, const int64_t* h_bonds_a, const int64_t* h_bonds_b,
                                       int64_t elem_bytes, int64_t bins_a, int64_t bins_b);
int ndmps_pairstat_plan_query(int elem, int L, const int64_t* h_dims, const int64_t* h_bonds_a, const int64_t* h_bonds_b,
                              int64_t bins_a, int64_t bins_b, int64_t* h_out);
int ndmps_pairstat_moments_f32(int L, const int64_t* h_dims, const int64_t* h_bonds_a, const int64_t* h_bonds_b,
                               const float* const* h_cores_a, const float* const* h_cores_b, double* h_stats,
                               int64_t* h_counts, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_pairstat_moments_f64(int L, const int64_t* h_dims, const int64_t* h_bonds_a, const int64_t* h_bonds_b,
                               const double* const* h_cores_a, const double* const* h_cores_b, double* h_stats,
                               int64_t* h_counts, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_pairstat_histogram_f32(int L, const int64_t* h_dims, const int64_t* h_bonds_a, const int64_t* h_bonds_b,
                                 const float* const* h_cores_a, const float* const* h_cores_b, const float* h_edges_a,
                                 int bins_a, const float* h_edges_b, int bins_b, int64_t* h_counts, void* d_ws,
                                 int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_pairstat_histogram_f64(int L, const int64_t* h_dims, const int64_t* h_bonds_a, const int64_t* h_bonds_b,
                                 const double* const* h_cores_a, const double* const* h_cores_b, const double* h_edges_a,
                                 int bins_a, const double* h_edges_b, int bins_b, int64_t* h_counts, void* d_ws,
                                 int64_t ws_bytes, ndmps_stream_t stream);
/* ---- Pair statistics per label of an atlas, from the cores (csrc/labelpair.hip, core/labelpair.py): two values per
 * voxel under the label d_labels[d_row_off[r] + d_col_off[c]].  ndmps_labelpair_*: the voxels of two chains of one
 * shape and one factorisation (as ndmps_pairstat_*; both run in the column order d_col_perm).  ndmps_labelpair_original_*:
 * the voxel of one chain and the element of d_ref (device, C order, element type) at the voxel's address, which is
 * also where the label is read.  A call is the moments pass of ndmps_pairstat_moments_* over the same operands, whose
 * extremes fix six exponents on the device, then one labelled launch per window of 512 labels.  Per voxel where
 * neither value is NaN, with d = (double)a - (double)b and the products formed in fp64, llrint(. 2^scale) of a, b,
 * a b (signed) and a a, b b, d d (unsigned) is added into 64-bit integers, and integer maxima of order-preserving
 * keys give min a, max a, min b, max b and max |d| (the last an fp64 key in either element type).  Only integers are
 * added atomically: the same inputs give the same bits.  A voxel with either value NaN is counted in n_nan of its
 * label; an infinite voxel or element of d_ref (or an fp64 difference that overflows) is refused with NDMPS_EINVAL
 * ("label pair statistics need finite voxels").  A label outside [0, n_labels) is counted in `outside`.
 *
 * The exponents (ndmps_labelpair_scales, host arithmetic only; the device applies the same function), h_scales[6] =
 * {s_a, s2_a, s_b, s2_b, s_ab, s2_d}: (s_a, s2_a) = ndmps_labelstat_scales(max |a|), (s_b, s2_b) likewise from max |b|,
 * s2_d the second exponent of ndmps_labelstat_scales(max |a - b|), and s_ab = 61 - nb - e with
 * fl(max |a| max |b|) < 2^e by frexp (e_a + e_b where that product is 0 or infinite), clamped to [-1000, 1000]; 0 when
 * either maximum is 0.  The maxima are taken over the voxels where neither value is NaN.
 *
 * Workspace: ndmps_labelpair_workspace_bytes(L, dims, bonds_a, bonds_b, elem_bytes, n_labels) =
 * ndmps_pairstat_workspace_bytes(.., 0, 0), or with h_bonds_b == NULL (the original)
 * ndmps_valstat_workspace_bytes(.., n_bins = 0), + the table, 8 * (13 * n_labels + 14) bytes rounded up to 256:
 * thirteen 64-bit slots per label (sum a, sum b, sum a b, sum a^2, sum b^2, sum d^2, count, NaN count, and the keys of
 * min a, max a, min b, max b, max |d|), then outside, overflow, the six exponents, the non-finite flag and the five
 * extremes of the whole volume.  0 for bad arguments.  1 <= n_labels <= 4096; d_labels as ndmps_labelstat_*.
 * Results (HOST): h_sums[3 n_labels] the signed integers of a, b, a b (value = integer 2^-s_a, 2^-s_b, 2^-s_ab);
 * h_sumsq[3 n_labels] the unsigned ones of a a, b b, d d (2^-s2_a, 2^-s2_b, 2^-s2_d); h_counts[2 n_labels] the counted
 * voxels then the NaN counts; h_ext[5 n_labels] min a, max a, min b, max b, max |d| as doubles (NaN where the count
 * is 0); h_info[NDMPS_LABELPAIR_INFO_SLOTS] = {outside, s_a, s2_a, s_b, s2_b, s_ab, s2_d, voxels}; h_whole[5] the
 * same five extremes over every counted voxel of the volume, labelled or not (+-inf where none is counted).
 * Every argument check returns before the first launch; one copy to the host; returns with the stream synchronised. */
#define NDMPS_LABELPAIR_INFO_SLOTS 8
int64_t ndmps_labelpair_workspace_bytes(int L, const int64_t* h_dims, const int64_t* h_bonds_a, const int64_t* h_bonds_b,
                                        int64_t elem_bytes, int64_t n_labels);
int ndmps_labelpair_scales(double maxabs_a, double maxabs_b, double max_abs_diff, int64_t numel, int* h_scales);
int ndmps_labelpair_f32(int L, const int64_t* h_dims, const int64_t* h_bonds_a, const int64_t* h_bonds_b,
                        const float* const* h_cores_a, const float* const* h_cores_b, const void* d_labels,
                        int label_elem_bytes, const int64_t* d_row_off, const int64_t* d_col_off, const int32_t* d_col_perm,
                        int64_t n_cols, int n_labels, int64_t* h_sums, uint64_t* h_sumsq, int64_t* h_counts, double* h_ext,
                        int64_t* h_info, double* h_whole, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_labelpair_f64(int L, const int64_t* h_dims, const int64_t* h_bonds_a, const int64_t* h_bonds_b,
                        const double* const* h_cores_a, const double* const* h_cores_b, const void* d_labels,
                        int label_elem_bytes, const int64_t* d_row_off, const int64_t* d_col_off, const int32_t* d_col_perm,
                        int64_t n_cols, int n_labels, int64_t* h_sums, uint64_t* h_sumsq, int64_t* h_counts, double* h_ext,
                        int64_t* h_info, double* h_whole, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_labelpair_original_f32(int L, const int64_t* h_dims, const int64_t* h_bonds, const float* const* h_cores,
                                 const float* d_ref, const void* d_labels, int label_elem_bytes, const int64_t* d_row_off,
                                 const int64_t* d_col_off, const int32_t* d_col_perm, int64_t n_cols, int n_labels,
                                 int64_t* h_sums, uint64_t* h_sumsq, int64_t* h_counts, double* h_ext, int64_t* h_info,
                                 double* h_whole, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_labelpair_original_f64(int L, const int64_t* h_dims, const int64_t* h_bonds, const double* const* h_cores,
                                 const double* d_ref, const void* d_labels, int label_elem_bytes, const int64_t* d_row_off,
                                 const int64_t* d_col_off, const int32_t* d_col_perm, int64_t n_cols, int n_labels,
                                 int64_t* h_sums, uint64_t* h_sumsq, int64_t* h_counts, double* h_ext, int64_t* h_info,
                                 double* h_whole, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);
/* C = A B with table-driven addressing of A and / or C: element (m, k) of A at d_A[d_a_row[m] + d_a_col[k]],
 * element (m, n) of C at d_C[d_c_row[m] + d_c_col[n]] (NULL pair: dense row-major).  a_vec4: d_a_col comes in
 * aligned runs of four consecutive offsets. */
int ndmps_sgemm_indexed(int64_t m, int64_t n, int64_t k, const float* d_A, int64_t lda,
                        const int64_t* d_a_row, const int64_t* d_a_col, int a_vec4, const float* d_B,
                        int64_t ldb, float* d_C, int64_t ldc, const int64_t* d_c_row,
                        const int64_t* d_c_col, ndmps_stream_t stream);
/* bf16 cores in, bf16 tensor out, fp32 accumulation (v_mfma_f32_32x32x16_bf16); workspace:
 * ndmps_chain_workspace_bytes (the fp32 size covers the bf16 intermediates and the transposed operands) */
int ndmps_chain_contract_bf16(int L, const int64_t* h_dims, const int64_t* h_bonds,
                              const void* const* h_cores, void* d_dense, void* d_ws,
                              int64_t ws_bytes, ndmps_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Region decode: replaces to_tensor()[key] (core/ndmps.py:131-153 decodes the whole volume, then indexes).
 * Left-to-right contraction over the live prefixes of a voxel set only (tables from core/region.py): for each
 * site s < L-1, h_nodes[s] nodes (a parent index and, through h_tiles[s] tiles (phys, row0, count <= 32) of nodes
 * that share their physical index, a gathered product with core s); the last site writes d_out[e] for e < n_out.
 * d_tables (int32, table_len = 2 n_out + sum_s (h_nodes[s] + 3 h_tiles[s])): per level parent[h_nodes[s]] then
 * the tiles; then leaf_parent[n_out], leaf_phys[n_out].  Entries out of range read zeros, never outside a buffer.
 * d_ws >= ndmps_region_workspace_bytes(L, bonds, nodes, sizeof element) (0 for L == 1).
 * --------------------------------------------------------------------------------- */
int64_t ndmps_region_workspace_bytes(int L, const int64_t* h_bonds, const int64_t* h_nodes, int64_t elem_bytes);
int ndmps_region_contract_f32(int L, const int64_t* h_dims, const int64_t* h_bonds, const float* const* h_cores,
                              const int64_t* h_nodes, const int64_t* h_tiles, const int32_t* d_tables,
                              int64_t table_len, int64_t n_out, float* d_out, void* d_ws, int64_t ws_bytes,
                              ndmps_stream_t stream);
int ndmps_region_contract_f64(int L, const int64_t* h_dims, const int64_t* h_bonds, const double* const* h_cores,
                              const int64_t* h_nodes, const int64_t* h_tiles, const int32_t* d_tables,
                              int64_t table_len, int64_t n_out, double* d_out, void* d_ws, int64_t ws_bytes,
                              ndmps_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Region decode of a series (NDMPS.decode_regions / values_at_many): the same region of T frames over the same
 * sites in one call -- one plan, one table upload, L launches with a frame dimension.  h_dims, h_nodes, h_tiles,
 * d_tables and table_len are those of ndmps_region_contract_* (the plan depends on the shape and the key only).
 * h_bonds (T x (L + 1), row t the bonds of frame t, outer bonds 1; inner bonds may differ between frames) is checked
 * on the host and gives the per-level caps cap_s = max_t bonds[t][s].
 * d_records, the frame records, is ONE device buffer the caller fills with one copy:
 *     T * L        core pointers (8 bytes each), frame-major: entry t * L + s is core s of frame t, a
 *                  (bonds[t][s], h_dims[s], bonds[t][s+1]) array of the call's element type;
 *     T * (L + 1)  int64 bonds, the same values as h_bonds.
 * d_out is (T, n_out): frame t's region at d_out + t * n_out, element for element what ndmps_region_contract_* gives
 * for that frame alone (one tile body serves both kernel families).
 * Workspace: two ping-pong buffers of T slabs; frame t uses the slab at t * frame_stride elements, frame_stride =
 * max_s h_nodes[s] * cap_{s+1}, with its rows packed at its own bond.  ndmps_region_series_workspace_bytes gives
 * 2 * round_up(T * frame_stride * elem_bytes, 256) (0 for L == 1, -1 for bad arguments); a smaller d_ws returns
 * NDMPS_EWORKSPACE before anything is launched.  1 <= T <= 65535 (a grid dimension) and L <= 64: larger series are
 * contracted in chunks of frames by the caller (core/region.py plan_series).
 * The kernels trust the records no more than the tables: a frame whose device record holds a bond below 1 or above
 * its cap, or a null core pointer, reads nothing, writes nothing to the workspace and gets zeros in d_out.
 * --------------------------------------------------------------------------------- */
int64_t ndmps_region_series_workspace_bytes(int T, int L, const int64_t* h_bonds, const int64_t* h_nodes,
                                            int64_t elem_bytes);
int ndmps_region_series_contract_f32(int T, int L, const int64_t* h_dims, const int64_t* h_bonds,
                                     const int64_t* h_nodes, const int64_t* h_tiles, const int32_t* d_tables,
                                     int64_t table_len, const void* d_records, int64_t n_out, float* d_out,
                                     void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_region_series_contract_f64(int T, int L, const int64_t* h_dims, const int64_t* h_bonds,
                                     const int64_t* h_nodes, const int64_t* h_tiles, const int32_t* d_tables,
                                     int64_t table_len, const void* d_records, int64_t n_out, double* d_out,
                                     void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Block-averaged decode (NDMPS.downsample / sum / mean): no reference counterpart (there: to_tensor(), core/ndmps.py:
 * 131-153, then a reshape and a mean).  Reduces every site of the chain (tables from core/pool.py):
 *     out_l[x, q, y] = h_weight[l] * sum_r A_l[x, qoff_l[q] + roff_l[r], y]
 * h_sites (L x 4): d'_l, n_red_l, start of qoff_l and of roff_l in d_offs (int32, offs_len entries).  Sites l < L_keep
 * are kept: out_l is a (chi_l, d'_l, chi_{l+1}) core at h_out[l] (NULL: the site is used as it is, nothing written).
 * Sites l >= L_keep must have d'_l = 1: they are collapsed right to left into a vector that site L_keep - 1 absorbs,
 * h_out[L_keep - 1] receiving its (chi, d', 1) core; with L_keep == 0, h_out[0] receives the scalar.
 * dtype: 0 fp32, 1 bf16 (outputs fp32), 2 fp64 (outputs fp64); sums in fp64.  d_ws >= ndmps_pool_workspace_bytes(L,
 * bonds) when L_keep < L.  Table entries outside a core read nothing.
 * ndmps_pool_dct_basis_*: d_W (n / block, n) = weight * the orthonormal DCT-II basis (ndmps_dct_basis_*) summed over
 * blocks of `block` rows; DCT coefficient rows y give the block-pooled voxels y W^T (ndmps_sgemm(0, 1, ...)).
 * --------------------------------------------------------------------------------- */
int64_t ndmps_pool_workspace_bytes(int L, const int64_t* h_bonds);
int ndmps_pool_cores(int dtype, int L, const int64_t* h_dims, const int64_t* h_bonds, const void* const* h_cores,
                     int L_keep, const int64_t* h_sites, const double* h_weight, const int32_t* d_offs,
                     int64_t offs_len, void* const* h_out, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_pool_dct_basis_f32(float* d_W, int64_t n, int64_t block, double weight, ndmps_stream_t stream);
int ndmps_pool_dct_basis_f64(double* d_W, int64_t n, int64_t block, double weight, ndmps_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Linear combination (no reference counterpart; core/lincomb.py): the TT-SVD rounding of sum_a w_a X^a for K
 * chains with the same L site dims, right to left, from pair-batched left Gram matrices (csrc/lincomb.hip).
 * h_bonds: K x (L + 1) (row a = input a's bonds, outer bonds 1); h_codes: K storage codes (0 fp32, 1 bf16, 2 fp64);
 * h_cores: K x L device pointers (row a = input a's cores).  Every summed bond sum_a chi_{a,k} must be <= 4096.
 * ndmps_lincomb_layout: returns the output arena's element count; h_out_off (L + 1): site j's core starts at element
 * h_out_off[j] (a prefix of its slot is used); *h_ws_bytes: workspace; *h_spec_stride: row stride of h_spectra.
 * ndmps_lincomb_round: out_code 0 fp32 or 2 fp64 cores into d_out; h_out_bonds (L + 1) the new bonds; h_spectra
 * (L x spec_stride doubles) row k = the kept singular values at bond k.  Keeps s_j > max(cutoff s_0, floor scale)
 * (floor 1e-6 for fp32 output, 1e-8 for fp64), at most max_bond (<= 0: none).  Returns 1 when nothing survives at
 * some bond, or scale is 0: the zero MPS (every bond 1, zero cores, a kept value of 0 per bond).  Synchronises the
 * stream.
 * --------------------------------------------------------------------------------- */
int64_t ndmps_lincomb_layout(int K, int L, const int64_t* h_dims, const int64_t* h_bonds, int64_t max_bond,
                             int64_t* h_out_off, int64_t* h_ws_bytes, int64_t* h_spec_stride);
int ndmps_lincomb_round(int K, int L, const int64_t* h_dims, const int64_t* h_bonds, const int* h_codes,
                        const void* const* h_cores, const double* h_weights, double cutoff, int64_t max_bond, int out_code,
                        double scale, void* d_out, int64_t out_elems, int64_t* h_out_bonds, double* h_spectra,
                        int64_t spec_stride, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Axis operators (no reference counterpart; core/axisop.py, csrc/axisop.hip): a matrix-product operator that acts on
 * one axis's digit per site, applied to a chain of L sites in one launch.  Site j of the input is (chi_j, d_j,
 * chi_{j+1}) with d_j = pre_j f_j post_j and the physical index (p f_j + digit) post_j + q; h_factors: the L radices
 * f_j; h_strides: the L strides post_j; h_mpo_bonds: the L + 1 operator bonds D_j (outer ones 1); h_mpo: the cores
 * M_j (D_j, f_j, f_j, D_{j+1}) indexed [c, o, i, c'], one after the other, mpo_len doubles in all.  Site j of the
 * result is
 *     Z_j[c chi_j + a, (p f_j + o) post_j + q, c' chi_{j+1} + a'] = sum_i M_j[c, o, i, c'] X_j[a, (p f_j + i) post_j + q, a']
 * a (D_j chi_j, d_j, D_{j+1} chi_{j+1}) core; every widened bond must be <= 4096.  code: storage of the input (0 fp32,
 * 1 bf16, 2 fp64); Z is fp64 for code 2 and fp32 otherwise, summed in fp64 over the entries of M that are not 0.
 * ndmps_axisop_layout: returns the element count of the result; h_out_off (L + 1): site j starts at element
 * h_out_off[j] of d_out; *h_ws_bytes: workspace.  ndmps_axisop_apply synchronises the stream.
 * --------------------------------------------------------------------------------- */
int64_t ndmps_axisop_layout(int L, const int64_t* h_dims, const int64_t* h_bonds, const int64_t* h_factors,
                            const int64_t* h_mpo_bonds, int64_t* h_out_off, int64_t* h_ws_bytes);
int ndmps_axisop_apply(int L, const int64_t* h_dims, const int64_t* h_bonds, int code, const void* const* h_cores,
                       const int64_t* h_factors, const int64_t* h_strides, const int64_t* h_mpo_bonds,
                       const double* h_mpo, int64_t mpo_len, void* d_out, int64_t out_elems, void* d_ws,
                       int64_t ws_bytes, ndmps_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Gram matrix of a series (no reference counterpart; core/series.py, csrc/series.hip): d_G[a, b] = <X^a, X^b> for
 * every pair of two lists of chains with the same L site dims, fp64, row-major Ka x Kb on the device.
 * h_bonds_*: K x (L + 1) (outer bonds 1); h_codes_*: storage codes (0 fp32, 1 bf16, 2 fp64); h_cores_*: K x L device
 * pointers.  symmetric != 0: both lists are the same (same pointers); a <= b is computed and copied to [b, a].
 * Route (ndmps_series_gram_route): 0 every inner bond <= 64, one launch with one workgroup per pair; 1 larger bonds,
 * all chains with the same bonds, ndmps_dgemm_batched per site; 2 larger ragged bonds, ndmps_dgemm pair by pair.
 * The same inputs give the same bits.  The result is left in d_G in stream order; route 0 waits for the upload of
 * its task tables before it launches, nothing waits afterwards.
 * --------------------------------------------------------------------------------- */
int64_t ndmps_series_gram_workspace_bytes(int Ka, int Kb, int L, const int64_t* h_dims, const int64_t* h_bonds_a,
                                          const int64_t* h_bonds_b);
int ndmps_series_gram_route(int Ka, int Kb, int L, const int64_t* h_dims, const int64_t* h_bonds_a,
                            const int64_t* h_bonds_b);
int ndmps_series_gram(int Ka, int Kb, int symmetric, int L, const int64_t* h_dims, const int64_t* h_bonds_a,
                      const int* h_codes_a, const void* const* h_cores_a, const int64_t* h_bonds_b,
                      const int* h_codes_b, const void* const* h_cores_b, double* d_G, void* d_ws, int64_t ws_bytes,
                      ndmps_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Masked / weighted Gram matrix of a series (no reference counterpart; core/wgram.py, csrc/wgram.hip):
 * d_G[a, b] = sum_x w(x) X^a(x) X^b(x) for every pair of two lists of chains and ONE weight chain w over the same L
 * site dims, by the exact three-chain contraction on the cores (no rounding, no sketch).  The lists are given as in
 * ndmps_series_gram; h_bonds_w: the weight's L + 1 bonds (outer ones 1, inner ones unrestricted), code_w its storage
 * code, h_cores_w its L device pointers.
 * Route (ndmps_series_wgram_route): 0 every inner bond of both lists <= 64, one sandwich launch and one fp64 product
 * per site over a whole chunk of pairs; 2 larger bonds, pair by pair on ndmps_dgemm / ndmps_dgemm_batched.
 * Workspace: the pairs are processed in chunks that fit d_ws.  ndmps_series_wgram_workspace_bytes returns what the call
 * uses under a cap of cap_bytes (all pairs in one chunk if they fit), or NDMPS_EWORKSPACE if not even one pair fits;
 * ndmps_series_wgram chunks by the ws_bytes it is given.  The workspace need not be zeroed.  The chunking changes no bit
 * of d_G, and the same inputs give the same bits.  The route and workspace functions need no device.
 * --------------------------------------------------------------------------------- */
int ndmps_series_wgram_route(int Ka, int Kb, int L, const int64_t* h_dims, const int64_t* h_bonds_a,
                             const int64_t* h_bonds_b, const int64_t* h_bonds_w);
int64_t ndmps_series_wgram_workspace_bytes(int Ka, int Kb, int symmetric, int L, const int64_t* h_dims,
                                           const int64_t* h_bonds_a, const int64_t* h_bonds_b,
                                           const int64_t* h_bonds_w, int64_t cap_bytes);
int ndmps_series_wgram(int Ka, int Kb, int symmetric, int L, const int64_t* h_dims, const int64_t* h_bonds_a,
                       const int* h_codes_a, const void* const* h_cores_a, const int64_t* h_bonds_b,
                       const int* h_codes_b, const void* const* h_cores_b, const int64_t* h_bonds_w, int code_w,
                       const void* const* h_cores_w, double* d_G, void* d_ws, int64_t ws_bytes,
                       ndmps_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Elementwise product of two chains by a randomised sketch (no reference counterpart; core/hadamard.py,
 * csrc/hadamard.hip).  Both chains have the L site dims h_dims; h_bonds_a / h_bonds_b: their L + 1 bonds (outer ones 1,
 * at most 4096); h_ell: the L + 1 sketch bonds l_k, l_0 = l_L = 1 and 1 <= l_k <= min(512, chi_{a,k} chi_{b,k}).
 * ndmps_hadamard_layout: returns the element count of the fp64 output arena; h_out_off (L + 1): site k starts at
 * element h_out_off[k] and has the capacity l_k d_k l_{k+1}; the sketch cores R_k (l_k, d_k, l_{k+1}) are laid out the
 * same way in h_R.  *h_ws_bytes, with m_k = chi_{a,k} chi_{b,k} and every piece rounded up to 256 bytes: 8 times
 *     sum_k l_k d_k l_{k+1}  (R)  +  sum_{inner k, l_k < m_k} l_k m_k  (environments)  +  max_k l_k d_k m_{k+1}  (Y of the
 *     environment pass and X of the forward pass share it: they are never live together)  +  max_k l_k m_k  (M)
 *     + 2 max_k l_k d_k l_{k+1}  (S, Q)  +  2 lmax^2 + lmax  (G, V, w)
 * plus ndmps_syevj_workspace_bytes(lmax) and, when some bond exceeds 64, both chains' cores in fp64 and
 * max_k l_k chi_{a,k} d_k chi_{b,k+1} doubles.
 * ndmps_hadamard_sketch: the left-orthonormal fp64 chain of bonds h_ranks[k] <= l_k that sketches the product chain
 * (site k written contiguously as (r_k, d_k, r_{k+1}) at h_out_off[k]).  code_*: storage of a chain's cores (0 fp32,
 * 1 bf16, 2 fp64); h_cores_*: L device pointers; h_R: r_len = the layout's element count HOST doubles.  Returns 0, or
 * 1 when the product is zero (every h_ranks[k] = 1, d_out undefined).  Synchronises the stream.
 * ndmps_hadamard_sandwich: the kernel family alone on one site, A (ca, d, ca2) and B (cb, d, cb2), n <= 512:
 *   form 0 (forward):      d_out[rho d + i] (ca2 x cb2) = A[:, i, :]^T d_E[rho] B[:, i, :],          d_E: n matrices ca x cb
 *   form 1 (environment):  d_out[rho] (ca x cb) = sum_i A[:, i, :] d_E[rho d + i] B[:, i, :]^T,      d_E: n d matrices ca2 x cb2
 * row-major fp64, summed in fixed order.  With all four bonds <= 64 it is one launch and needs no workspace;
 * otherwise d_ws holds 8 (ca d ca2 + cb d cb2 + n ca d cb2) bytes plus 768.  Only the ro x co elements of each
 * result are written.
 * Every argument error (NULL pointers, bad codes, outer bonds != 1, l_k > 512, a short arena or workspace) is
 * NDMPS_EINVAL before anything is launched.
 * --------------------------------------------------------------------------------- */
int64_t ndmps_hadamard_layout(int L, const int64_t* h_dims, const int64_t* h_bonds_a, const int64_t* h_bonds_b,
                              const int64_t* h_ell, int64_t* h_out_off, int64_t* h_ws_bytes);
int ndmps_hadamard_sketch(int L, const int64_t* h_dims, const int64_t* h_bonds_a, int code_a,
                          const void* const* h_cores_a, const int64_t* h_bonds_b, int code_b,
                          const void* const* h_cores_b, const int64_t* h_ell, const double* h_R, int64_t r_len,
                          double* d_out, int64_t out_elems, int64_t* h_ranks, void* d_ws, int64_t ws_bytes,
                          ndmps_stream_t stream);
int ndmps_hadamard_sandwich(int form, int64_t ca, int64_t d, int64_t ca2, int64_t cb, int64_t cb2, int code_a,
                            const void* d_core_a, int code_b, const void* d_core_b, int64_t n, const double* d_E,
                            double* d_out, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Rounding of K weighted sums of T chains by a randomised sketch (no reference counterpart; core/sumsketch.py,
 * csrc/sumsketch.hip).  All chains have the L site dims h_dims; h_bonds: T x (L + 1) bonds, frame a at a (L + 1)
 * (outer ones 1, at most 4096; a frame with a bond above 64 leaves the resident kernels for a general route through
 * ndmps_dgemm on its cores widened to fp64); h_ell: the L + 1 sketch bonds l_k, l_0 = l_L = 1,
 * 1 <= l_k <= 512.
 * ndmps_sumsketch_layout (host only): returns the element count of the fp64 output arena for K chains, K times the
 * count of one chain; h_out_off (L + 1): inside a chain site k starts at element h_out_off[k] and has the capacity
 * l_k d_k l_{k+1}; chain j starts at j h_out_off[L]; the sketch cores R_k (l_k, d_k, l_{k+1}) are laid out like one chain
 * in h_R.  *h_ws_bytes, with m_k = sum_a chi_{a,k}, every piece rounded up to 256 bytes, plus 256: 8 times
 *     sum_k l_k d_k l_{k+1}  (R)  |  1  (W_{a,L})  |  max(1, sum_{k=1..L-1} l_k m_k)  (environments)  |  max_{k<L} l_k m_k
 *     (M, twice)  |  max_k l_k d_k l_{k+1}  (S and Q, one piece each)  |  max_k nsplit_k l_k d_k l_{k+1}  (partials of the sketch
 *     form, nsplit_k = min(max(1, 512 / (d_k ceil(l_k / 64) ceil(l_{k+1} / 64))), max(1, min(16, T / 4))), integer
 *     divisions)  |  lmax^2  (G and V, one piece each)  |  lmax  (w)
 * then max(1, ndmps_syevj_workspace_bytes(lmax)) bytes, 64 T L bytes (records) and 8 T bytes (frame lists), and, when
 * some frame has a bond above 64, 8 times the sum of those frames' core sizes and 8 max l_k d_k chi_{a,k+1} over them.
 * ndmps_sumsketch_sketch: for each output row j of h_weights (K x T, HOST) the left-orthonormal fp64 chain of bonds
 * h_ranks[j (L + 1) + k] <= l_k that sketches sum_a h_weights[j, a] chain_a (site k written contiguously as
 * (r_k, d_k, r_{k+1}) at its offset).  h_codes: T storage codes (0 fp32, 1 bf16, 2 fp64); h_cores: T x L device
 * pointers, frame a site k at a L + k; h_R: r_len = h_out_off[L] HOST doubles.  h_zero[j] = 1 where output j is zero
 * (a row of zero weights, or s_0 = 0 at some bond): its ranks are 1 and its part of d_out is undefined.  A frame
 * whose weights are zero in every row is read in neither pass; a zero entry is skipped in that row's forward pass.
 * Sums over frames run in ascending order without atomics.  Synchronises the stream.
 * ndmps_sumsketch_step: the kernel family alone on one site for T frames with cores (chi_a, d, chi2_a); per-frame
 * matrices are row-major fp64, concatenated in frame order:
 *   form 0 (env):      d_out: W_a (chi_a x l0) = sum_i A_a[:, i, :] (Wn_a R[:, i, :]^T),   d_in: Wn_a (chi2_a x l1), d_mat: R (l0, d, l1)
 *   form 1 (sketch):   d_out: S ((l0 d) x l1) = sum_a (M_a A_a[:, i, :]) Wn_a,             d_in: M_a (l0 x chi_a), d_in2: Wn_a (chi2_a x l1)
 *   form 2 (project):  d_out: Mn_a (l1 x chi2_a) = sum_i Q[(., i), :]^T (M_a A_a[:, i, :]), d_in: M_a (l0 x chi_a), d_mat: Q ((l0 d) x l1)
 * l0, l1 <= 512.  d_ws: 68 T bytes plus 8 nsplit l0 d l1 (form 1, nsplit as above with l_k = l0, l_{k+1} = l1) plus 1024;
 * with frames of a bond above 64 (general route) also 8 (chi_a d chi2_a) + 256 for each of them, 8 l0 d max chi2_a and
 * (form 1) 8 l0 d l1.
 * Only the elements of each result are written.  Synchronises the stream.
 * Every argument error (NULL pointers, bad codes, outer bonds != 1, a frame bond > 4096, l_k > 512, a non-finite
 * weight, a short arena or workspace) is NDMPS_EINVAL before anything is launched.
 * --------------------------------------------------------------------------------- */
int64_t ndmps_sumsketch_layout(int T, int K, int L, const int64_t* h_dims, const int64_t* h_bonds, const int64_t* h_ell,
                               int64_t* h_out_off, int64_t* h_ws_bytes);
int ndmps_sumsketch_sketch(int T, int K, int L, const int64_t* h_dims, const int64_t* h_bonds, const int* h_codes,
                           const void* const* h_cores, const double* h_weights, const int64_t* h_ell, const double* h_R,
                           int64_t r_len, double* d_out, int64_t out_elems, int64_t* h_ranks, int* h_zero, void* d_ws,
                           int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_sumsketch_step(int form, int T, int64_t d, const int64_t* h_chi, const int64_t* h_chi2, const int* h_codes,
                         const void* const* h_cores, int64_t l0, int64_t l1, const double* d_in, const double* d_in2,
                         const double* d_mat, double* d_out, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Overlap: replaces `mps @ mps` (core/ndmps.py:76,86; utils/metrics.py:160), real data,
 * no conjugation, fp64 transfer matrices.  Synchronises the stream.
 * --------------------------------------------------------------------------------- */
int64_t ndmps_overlap_workspace_bytes(int L, const int64_t* h_dims, const int64_t* h_bonds_a,
                                      const int64_t* h_bonds_b);
int ndmps_overlap_f32(int L, const int64_t* h_dims, const int64_t* h_bonds_a,
                      const float* const* h_cores_a, const int64_t* h_bonds_b,
                      const float* const* h_cores_b, double* h_out, void* d_ws,
                      int64_t ws_bytes, ndmps_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Core quantisation: utils/filetools.py:20-39 scale_to_dtype/scale_back
 * with the reference's truncating cast.  bits = 8 or 16.
 * --------------------------------------------------------------------------------- */
int ndmps_quantize_f32(const float* d_x, int64_t n, float lo, float hi, int bits, void* d_q,
                       ndmps_stream_t stream);
int ndmps_dequantize_f32(const void* d_q, int64_t n, float lo, float hi, int bits, float* d_x,
                         ndmps_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Quality metrics on device-resident volumes, semantics of utils/metrics.py:
 * ndmps_ssim_f32 = compute_ssim_by_dim(a, b) (metrics.py:108-129; 2-D / 3-D / 4-D, uniform window,
 * per-slice joint data_range, second argument clipped at 0), ndmps_psnr_f32 = compute_psnr(a, b)
 * (metrics.py:132-146).  fp32 inputs, fp64 arithmetic.  Both synchronise the stream.
 * --------------------------------------------------------------------------------- */
int64_t ndmps_ssim_workspace_bytes(int ndim, const int64_t* h_shape);
int ndmps_ssim_f32(const float* d_a, const float* d_b, int ndim, const int64_t* h_shape,
                   double* h_out, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);
/* ssim_3d_axis(a, b, axis) (utils/metrics.py:35-65): the SSIM of every 2-D slice along `axis` (0, 1, 2) of a 3-D
 * volume, h_out[shape[axis]]; the 3-D value of ndmps_ssim_f32 is the mean over the axes of the means of these lists. */
int64_t ndmps_ssim_slices_workspace_bytes(const int64_t* h_shape, int axis);
int ndmps_ssim_slices_f32(const float* d_a, const float* d_b, const int64_t* h_shape, int axis, double* h_out,
                          void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);
int64_t ndmps_psnr_workspace_bytes(void);
int ndmps_psnr_f32(const float* d_a, const float* d_b, int64_t n, double* h_out, void* d_ws,
                   int64_t ws_bytes, ndmps_stream_t stream);

/* ---------------------------------------------------------------------------------
 * fp64 storage -- the reference's own element type (core/ndmps.py:56 `tensor.astype(np.float64)`): volume, carried
 * matrices and cores are fp64 in HBM and every product runs on the fp64 MFMA, so that the reference's own
 * tolerances hold (tests/core/test_ndmps.py:35-38 round trip atol 1e-10; :41-44, :63-66 norm rel 1e-12).  Same
 * argument meaning as the _f32 twins; layout offsets (ndmps_tt_layout) are in elements and shared.  Singular values
 * come from fp64 Gram matrices: the relative cutoff of the sweep is clamped below at 1e-8 (sqrt(eps) s_0).
 *   ndmps_gram_f64                  G = A^T A, A fp64                    (core/ndmps.py:74, the SVD of from_dense)
 *   ndmps_tt_sweep_batched_f64      MatrixProductState.from_dense        (core/ndmps.py:74)
 *   ndmps_compress_bond_f64         tensor_compress_bond                 (core/ndmps.py:104-106)
 *   ndmps_chain_contract_f64        mps ^ ...                            (core/ndmps.py:140)
 *   ndmps_overlap_f64               mps @ mps                            (core/ndmps.py:76,86)
 *   ndmps_sumsq_f64 / _scale_f64    tensor /= np.linalg.norm(tensor)     (core/ndmps.py:60-61)
 *   ndmps_minmax_many_f64           boundary_list                        (core/ndmps.py:75,80-82)
 *   ndmps_dct_basis_f64 / _dct_last_f64 / _idct_last_f64  scipy dct / idct, norm="ortho" (core/ndmps.py:62-63,152-153)
 *   ndmps_quantize_f64 / _dequantize_f64  scale_to_dtype / scale_back    (utils/filetools.py:20-39)
 * --------------------------------------------------------------------------------- */
int64_t ndmps_gram_f64_workspace_bytes(int64_t m, int64_t n);
int ndmps_gram_f64(const double* d_A, int64_t m, int64_t n, int64_t lda, double* d_G, void* d_ws,
                   int64_t ws_bytes, ndmps_stream_t stream);
int64_t ndmps_tt_sweep_batched_workspace_bytes_f64(int batch, int L, const int64_t* h_dims, int64_t max_bond);
int ndmps_tt_sweep_batched_f64(int batch, double* const* h_dense, int L, const int64_t* h_dims,
                               double cutoff, int64_t max_bond, double* const* h_cores,
                               const int64_t* h_core_offsets, int64_t* h_bonds_out, double* h_spectra,
                               const int64_t* h_spec_offsets, void* d_ws, int64_t ws_bytes,
                               ndmps_stream_t stream);
int ndmps_compress_bond_f64(const double* d_t1, const double* d_t2, int64_t chi_l, int64_t d1,
                            int64_t chi, int64_t d2, int64_t chi_r, double cutoff, int64_t max_bond,
                            double* d_new1, double* d_new2, int64_t* h_new_chi, double* h_s, void* d_ws,
                            int64_t ws_bytes, ndmps_stream_t stream);
int64_t ndmps_chain_workspace_bytes_f64(int L, const int64_t* h_dims, const int64_t* h_bonds);
int ndmps_chain_contract_f64(int L, const int64_t* h_dims, const int64_t* h_bonds,
                             const double* const* h_cores, double* d_dense, void* d_ws, int64_t ws_bytes,
                             ndmps_stream_t stream);
int ndmps_overlap_f64(int L, const int64_t* h_dims, const int64_t* h_bonds_a,
                      const double* const* h_cores_a, const int64_t* h_bonds_b,
                      const double* const* h_cores_b, double* h_out, void* d_ws, int64_t ws_bytes,
                      ndmps_stream_t stream);
int ndmps_sumsq_f64(const double* d_x, int64_t n, double* h_out, void* d_ws, int64_t ws_bytes,
                    ndmps_stream_t stream);
int ndmps_scale_f64(double* d_x, int64_t n, double factor, ndmps_stream_t stream);
/* h_out: 2 * count doubles (min, max); h_sumsq may be NULL; workspace: ndmps_minmax_many_workspace_bytes */
int ndmps_minmax_many_f64(int count, const double* const* h_ptrs, const int64_t* h_lens, double* h_out,
                          double* h_sumsq, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream);
int ndmps_dct_basis_f64(double* d_basis, int64_t n, ndmps_stream_t stream);
int ndmps_dct_last_f64(const double* d_x, double* d_y, int64_t rows, int64_t n, const double* d_basis,
                       ndmps_stream_t stream);
int ndmps_idct_last_f64(const double* d_y, double* d_x, int64_t rows, int64_t n, const double* d_basis,
                        ndmps_stream_t stream);
int ndmps_quantize_f64(const double* d_x, int64_t n, double lo, double hi, int bits, void* d_q,
                       ndmps_stream_t stream);
int ndmps_dequantize_f64(const void* d_q, int64_t n, double lo, double hi, int bits, double* d_x,
                         ndmps_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NDMPS_HIP_H */
