// Launch helpers shared by the sweep (tt.hip) and the decode (chain.hip): the widening copy to fp64 and the GEMM of
// each storage type behind one name.  Internal linkage: each of the two gets its own copy, as when these lived in
// tt.hip's anonymous namespace.
#pragma once
#include "common.h"

namespace {
using ndmps::grid1d;

// y <- x widened to fp64; the body is shared with the sweep's batched twin, which resolves the volume's pointers first
template <typename T>
__device__ __forceinline__ void f32_to_f64_body(const T* __restrict__ x, int64_t n, double* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = ndmps::to_f64(x[i]);
}
template <typename T>
__global__ void __launch_bounds__(256) f32_to_f64_kernel(const T* __restrict__ x, int64_t n, double* y) {
  f32_to_f64_body(x, n, y);
}

// C (m, n) = A (m, k) op(B);  tws: scratch of the bf16 path (transposed copy of a (k, n) right operand)
inline int gemm_T(int transB, int64_t m, int64_t n, int64_t k, const float* A, const float* B, int64_t ldb, float* C,
                  void*, int64_t, hipStream_t s) {
  return ndmps_sgemm(0, transB, m, n, k, A, k, B, ldb, C, n, s);
}
inline int gemm_T(int transB, int64_t m, int64_t n, int64_t k, const __bf16* A, const __bf16* B, int64_t ldb, __bf16* C,
                  void* tws, int64_t tws_bytes, hipStream_t s) {
  return ndmps_gemm_bf16(transB, m, n, k, A, k, B, ldb, C, n, tws, tws_bytes, s);
}

inline int gemm_T(int transB, int64_t m, int64_t n, int64_t k, const double* A, const double* B, int64_t ldb, double* C,
                  void*, int64_t, hipStream_t s) {
  return ndmps_dgemm(0, transB, m, n, k, A, k, B, ldb, C, n, s);
}

// general product with explicit leading dimensions (fp32 / fp64)
inline int gemm_any(int tA, int tB, int64_t m, int64_t n, int64_t k, const float* A, int64_t lda, const float* B, int64_t ldb,
                    float* C, int64_t ldc, hipStream_t s) {
  return ndmps_sgemm(tA, tB, m, n, k, A, lda, B, ldb, C, ldc, s);
}
inline int gemm_any(int tA, int tB, int64_t m, int64_t n, int64_t k, const double* A, int64_t lda, const double* B,
                    int64_t ldb, double* C, int64_t ldc, hipStream_t s) {
  return ndmps_dgemm(tA, tB, m, n, k, A, lda, B, ldb, C, ldc, s);
}

// products of a whole lockstep group in one launch (fp32 / fp64 storage; bf16 storage goes volume by volume)
inline bool gemm_batched_T(int batch, int transB, int64_t m, int64_t n, int64_t k, double* const* A, double* const* B,
                           int64_t ldb, double* const* C, hipStream_t s, int* rc) {
  if (batch > ndmps_gemm_batched_max()) return false;
  *rc = ndmps_dgemm_batched(batch, 0, transB, m, n, k, (const double* const*)A, k, (const double* const*)B, ldb, C, n, s);
  return true;
}
inline bool gemm_batched_T(int batch, int transB, int64_t m, int64_t n, int64_t k, float* const* A, float* const* B,
                           int64_t ldb, float* const* C, hipStream_t s, int* rc) {
  if (batch > ndmps_gemm_batched_max()) return false;
  *rc = ndmps_sgemm_batched(batch, 0, transB, m, n, k, (const float* const*)A, k, (const float* const*)B, ldb, C, n, s);
  return true;
}
inline bool gemm_batched_T(int, int, int64_t, int64_t, int64_t, __bf16* const*, __bf16* const*, int64_t, __bf16* const*,
                           hipStream_t, int*) {
  return false;
}

}  // namespace
