// Dense building blocks on the CDNA4 matrix cores.
//
//   ndmps_sgemm  : C = op(A) op(B), fp32 in / fp32 accumulate, v_mfma_f32_32x32x2_f32
//   ndmps_dgemm  : same in fp64, v_mfma_f64_16x16x4_f64
//   ndmps_sgemm_indexed*, ndmps_sgemm_gathered64_stream_batched : products whose operands are read
//                  through offset tables (the index permutation of the reshape stage), tiled or streamed
//
// They stand in for the LAPACK/BLAS calls NumPy makes inside quimb for the reference
// (dgemm via tensordot in `mps ^ ...`, core/ndmps.py:140; the SVD's internal products in
// from_dense, core/ndmps.py:74).  GEMMs here are genuine dense GEMMs (bond x bond x phys);
// nothing is reshaped to reach the matrix cores.
//
// Layout notes (wave64): for the f32 32x32x2 MFMA lane l feeds A[i=l&31][k=l>>5] and
// B[k=l>>5][j=l&31]; for the f64 16x16x4 MFMA A[i=l&15][k=l>>4], B[k=l>>4][j=l&15].  Both
// operand tiles are therefore staged k-major in LDS (As[k][m], Bs[k][n]) so a fragment
// read is 32 (16) consecutive words per half (quarter) wave: conflict-free ds_read.
#include <stdlib.h>

#include <algorithm>

#include "common.h"
#include "gemm_plan.h"

namespace {

using ndmps::f64x4;
using ndmps::load4_stream_f32;
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <typename T>
struct Mfma;

template <>
struct Mfma<float> {
  static constexpr int MT = 32;   // tile edge
  static constexpr int KS = 2;    // k per instruction
  static constexpr int NACC = 16; // accumulator registers per lane
  typedef f32x16 acc_t;
  static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int acc_row(int reg, int lane) {
    return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
  }
  static __device__ __forceinline__ int acc_col(int lane) { return lane & 31; }
  static __device__ __forceinline__ int frag_idx(int lane) { return lane & 31; }
  static __device__ __forceinline__ int frag_k(int lane) { return lane >> 5; }
};

template <>
struct Mfma<double> {
  static constexpr int MT = 16;
  static constexpr int KS = 4;
  static constexpr int NACC = 4;
  typedef f64x4 acc_t;
  static __device__ __forceinline__ acc_t mma(double a, double b, acc_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int acc_row(int reg, int lane) { return (lane >> 4) + 4 * reg; }
  static __device__ __forceinline__ int acc_col(int lane) { return lane & 15; }
  static __device__ __forceinline__ int frag_idx(int lane) { return lane & 15; }
  static __device__ __forceinline__ int frag_k(int lane) { return lane >> 4; }
};

// ----------------------------------------------------------------------------------
// Generic tiled GEMM.  256 threads = 4 waves laid out WAVES_M x WAVES_N over a BM x BN
// block tile; BK-deep k-tiles staged through LDS (k-major for both operands).  The next
// k-tile is fetched into registers while the current one is consumed (one LDS buffer, two
// barriers per k-tile).  VEC: every operand row is a multiple of 4 elements and 16-byte
// (32-byte for fp64) aligned, so a thread moves 4 consecutive elements per global access;
// otherwise element-wise guarded loads (any shape, any leading dimension).
// ----------------------------------------------------------------------------------
template <typename T>
struct alignas(sizeof(T) * 4) Quad {
  T v[4];
};

// Optional table-driven addressing (IDX): element (m, k) of A at A[a_row[m] + a_col[k]], element (m, n) of C
// at C[c_row[m] + c_col[n]]; a NULL pair means dense row-major for that operand.  This is how the index
// permutation of the reshape stage rides on a product: the offset of a site-order element is additive over
// sites (permute.hip), so for any split of the sites into a row part and a column part it is
// RowOff[r] + ColOff[c].  With VEC, a_col must come in aligned runs of 4 consecutive offsets.
struct GemmIndex {
  const int64_t* a_row;
  const int64_t* a_col;
  const int64_t* c_row;
  const int64_t* c_col;
  int guarded;  // A/B (NDMPS_GEMM_GUARDED): every tile through the guarded fetch
};
inline int gemm_guarded_env() { return getenv("NDMPS_GEMM_GUARDED") ? 1 : 0; }

// operands of a batch of products of one shape: product blockIdx.z uses a[z], b[z], c[z] (kernel arguments)
constexpr int kGemmMaxBatch = 64;
struct GemmBatchPtrs {
  const void* a[kGemmMaxBatch];
  const void* b[kGemmMaxBatch];
  void* c[kGemmMaxBatch];
};

template <typename T, int BM, int BN, int WAVES_M, int WAVES_N, bool TA, bool TB, bool VEC, bool IDX>
__device__ __forceinline__ void
gemm_body(int64_t M, int64_t N, int64_t K, const T* __restrict__ A, int64_t lda, const T* __restrict__ B, int64_t ldb,
          T* __restrict__ C, int64_t ldc, const GemmIndex& ix) {
  using MF = Mfma<T>;
  constexpr int BK = 16;
  constexpr int MT = MF::MT;
  constexpr int TM = BM / (WAVES_M * MT);
  constexpr int TN = BN / (WAVES_N * MT);
  constexpr int PAD = 4;
  constexpr int A_PER = BM * BK / 256, B_PER = BN * BK / 256;  // elements per thread and k-tile
  static_assert(WAVES_M * WAVES_N == 4, "4 waves per workgroup");
  static_assert(TM >= 1 && TN >= 1, "tile too small");
  constexpr bool VA = VEC && A_PER % 4 == 0, VB = VEC && B_PER % 4 == 0;  // per-operand vector staging

  __shared__ T As[BK][BM + PAD];
  __shared__ T Bs[BK][BN + PAD];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WAVES_N;
  const int wn = wave % WAVES_N;
  const int64_t m0 = (int64_t)blockIdx.x * BM;  // x: row blocks (can exceed 65535)
  const int64_t n0 = (int64_t)blockIdx.y * BN;

  typename MF::acc_t acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < MF::NACC; ++r) acc[i][j][r] = (T)0;

  T ra[A_PER], rb[B_PER];

  // table-addressed A (the volume read through the index permutation): the row offsets of this thread's quads
  // are loop-invariant (registers) and the column offsets of the whole K range sit in LDS -- looked up in global
  // memory per k-tile they put two dependent L2 round trips in front of every tile (first projection of a group:
  // 1.14 ms for 2.1 GB)
  constexpr int kIdxK = 1024;
  __shared__ int64_t acol_s[(IDX && !TA && VEC) ? kIdxK : 1];
  int64_t arow_q[(A_PER / 4) > 0 ? (A_PER / 4) : 1];
  const bool idx_fast = IDX && !TA && VA && ix.a_row != nullptr && K <= kIdxK;
  if (IDX && !TA && VA) {
    if (idx_fast) {
      for (int64_t kk = tid; kk < K; kk += 256) acol_s[kk] = ix.a_col[kk];
#pragma unroll
      for (int i = 0; i < A_PER / 4; ++i) {
        const int m = (tid + 256 * i) / (BK / 4);
        arow_q[i] = m0 + m < M ? ix.a_row[m0 + m] : 0;
      }
      __syncthreads();
    }
  }

  // Tiles that lie inside the matrices (and k-tiles inside K) are fetched by straight-line code: a load inside a
  // per-lane guard sits in an exec-masked block behind its own s_waitcnt vmcnt(0) (see gram128_kernel), so the
  // guarded quads of a k-tile went out one memory round trip after the other.
  const bool inner_a = VA && m0 + BM <= M && !ix.guarded, inner_b = VB && n0 + BN <= N && !ix.guarded;
  // op(A)[m][k]: stored (M, K) unless TA (then (K, M)).  contiguous axis: k unless TA (then m)
  auto fetch_a = [&](int64_t k0) {
    if (VA && inner_a && k0 + BK <= K) {
#pragma unroll
      for (int i = 0; i < A_PER / 4; ++i) {
        const int e = tid + 256 * i;  // quad index
        const T* src;
        if (TA) {
          src = A + (k0 + e / (BM / 4)) * lda + m0 + (e % (BM / 4)) * 4;
        } else {
          const int m = e / (BK / 4), k = (e % (BK / 4)) * 4;
          if (IDX && idx_fast) src = A + arow_q[i] + acol_s[k0 + k];
          else if (IDX && ix.a_row) src = A + ix.a_row[m0 + m] + ix.a_col[k0 + k];
          else src = A + (m0 + m) * lda + k0 + k;
        }
        const Quad<T> q = *reinterpret_cast<const Quad<T>*>(src);
#pragma unroll
        for (int j = 0; j < 4; ++j) ra[4 * i + j] = q.v[j];
      }
    } else if (VA) {
#pragma unroll
      for (int i = 0; i < A_PER / 4; ++i) {
        const int e = tid + 256 * i;  // quad index
        Quad<T> q;
        q.v[0] = q.v[1] = q.v[2] = q.v[3] = (T)0;
        if (TA) {
          const int k = e / (BM / 4), m = (e % (BM / 4)) * 4;
          if (k0 + k < K && m0 + m < M) q = *reinterpret_cast<const Quad<T>*>(A + (k0 + k) * lda + m0 + m);
        } else {
          const int m = e / (BK / 4), k = (e % (BK / 4)) * 4;
          if (k0 + k < K && m0 + m < M) {
            if (IDX && idx_fast) q = *reinterpret_cast<const Quad<T>*>(A + arow_q[i] + acol_s[k0 + k]);
            else if (IDX && ix.a_row) q = *reinterpret_cast<const Quad<T>*>(A + ix.a_row[m0 + m] + ix.a_col[k0 + k]);
            else q = *reinterpret_cast<const Quad<T>*>(A + (m0 + m) * lda + k0 + k);
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) ra[4 * i + j] = q.v[j];
      }
    } else {
#pragma unroll
      for (int i = 0; i < A_PER; ++i) {
        const int e = tid + 256 * i;
        int m, k;
        if (TA) {
          k = e / BM;
          m = e % BM;
        } else {
          m = e / BK;
          k = e % BK;
        }
        const int64_t gk = k0 + k, gm = m0 + m;
        if (IDX && ix.a_row) ra[i] = (gk < K && gm < M) ? A[ix.a_row[gm] + ix.a_col[gk]] : (T)0;
        else ra[i] = (gk < K && gm < M) ? (TA ? A[gk * lda + gm] : A[gm * lda + gk]) : (T)0;
      }
    }
  };
  auto fetch_b = [&](int64_t k0) {
    if (VB && inner_b && k0 + BK <= K) {
#pragma unroll
      for (int i = 0; i < B_PER / 4; ++i) {
        const int e = tid + 256 * i;
        const T* src = TB ? B + (n0 + e / (BK / 4)) * ldb + k0 + (e % (BK / 4)) * 4
                          : B + (k0 + e / (BN / 4)) * ldb + n0 + (e % (BN / 4)) * 4;
        const Quad<T> q = *reinterpret_cast<const Quad<T>*>(src);
#pragma unroll
        for (int j = 0; j < 4; ++j) rb[4 * i + j] = q.v[j];
      }
    } else if (VB) {
#pragma unroll
      for (int i = 0; i < B_PER / 4; ++i) {
        const int e = tid + 256 * i;
        Quad<T> q;
        q.v[0] = q.v[1] = q.v[2] = q.v[3] = (T)0;
        if (TB) {
          const int n = e / (BK / 4), k = (e % (BK / 4)) * 4;
          if (k0 + k < K && n0 + n < N) q = *reinterpret_cast<const Quad<T>*>(B + (n0 + n) * ldb + k0 + k);
        } else {
          const int k = e / (BN / 4), n = (e % (BN / 4)) * 4;
          if (k0 + k < K && n0 + n < N) q = *reinterpret_cast<const Quad<T>*>(B + (k0 + k) * ldb + n0 + n);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) rb[4 * i + j] = q.v[j];
      }
    } else {
#pragma unroll
      for (int i = 0; i < B_PER; ++i) {
        const int e = tid + 256 * i;
        int n, k;
        if (TB) {
          n = e / BK;
          k = e % BK;
        } else {
          k = e / BN;
          n = e % BN;
        }
        const int64_t gk = k0 + k, gn = n0 + n;
        rb[i] = (gk < K && gn < N) ? (TB ? B[gn * ldb + gk] : B[gk * ldb + gn]) : (T)0;
      }
    }
  };
  auto commit = [&]() {
    if (VA) {
#pragma unroll
      for (int i = 0; i < A_PER / 4; ++i) {
        const int e = tid + 256 * i;
        if (TA) {
          const int k = e / (BM / 4), m = (e % (BM / 4)) * 4;
#pragma unroll
          for (int j = 0; j < 4; ++j) As[k][m + j] = ra[4 * i + j];
        } else {
          const int m = e / (BK / 4), k = (e % (BK / 4)) * 4;
#pragma unroll
          for (int j = 0; j < 4; ++j) As[k + j][m] = ra[4 * i + j];
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < A_PER; ++i) {
        const int e = tid + 256 * i;
        if (TA) As[e / BM][e % BM] = ra[i];
        else As[e % BK][e / BK] = ra[i];
      }
    }
    if (VB) {
#pragma unroll
      for (int i = 0; i < B_PER / 4; ++i) {
        const int e = tid + 256 * i;
        if (TB) {
          const int n = e / (BK / 4), k = (e % (BK / 4)) * 4;
#pragma unroll
          for (int j = 0; j < 4; ++j) Bs[k + j][n] = rb[4 * i + j];
        } else {
          const int k = e / (BN / 4), n = (e % (BN / 4)) * 4;
#pragma unroll
          for (int j = 0; j < 4; ++j) Bs[k][n + j] = rb[4 * i + j];
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < B_PER; ++i) {
        const int e = tid + 256 * i;
        if (TB) Bs[e % BK][e / BK] = rb[i];
        else Bs[e / BN][e % BN] = rb[i];
      }
    }
  };

  fetch_a(0);
  fetch_b(0);
  const int fi = MF::frag_idx(lane);
  const int fk = MF::frag_k(lane);
  for (int64_t k0 = 0; k0 < K; k0 += BK) {
    __syncthreads();  // previous k-tile fully consumed
    commit();
    __syncthreads();
    if (k0 + BK < K) {  // next k-tile in flight under the MFMAs
      fetch_a(k0 + BK);
      fetch_b(k0 + BK);
    }
#pragma unroll
    for (int kk = 0; kk < BK; kk += MF::KS) {
      T a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = As[kk + fk][(wm * TM + i) * MT + fi];
#pragma unroll
      for (int j = 0; j < TN; ++j) b[j] = Bs[kk + fk][(wn * TN + j) * MT + fi];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = MF::mma(a[i], b[j], acc[i][j]);
    }
  }

  // ---- epilogue
  if constexpr (IDX && MF::MT == 32 && BM == 128 && BN == 128 && sizeof(T) == 4) {
    if (ix.c_row) {
      // table-addressed C of the big tile (the last chain product: the reconstructed volume, written once): every
      // 32 x 32 accumulator tile goes through a wave-private LDS patch so that a lane owns FOUR consecutive columns
      // of a row -- 16-byte stores wherever the four column offsets are consecutive (64-byte runs at 256^3)
      // instead of 4-byte ones.  All offsets are requested before the first store.
      __shared__ float cstage[4][32][36];
      float (*st)[36] = cstage[wave];
      const int rl0 = lane >> 3, cl = (lane & 7) * 4;
      int64_t roff[TM][4], coff[TN][4];
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int64_t col = n0 + (wn * TN + j) * MT + cl;
#pragma unroll
        for (int e = 0; e < 4; ++e) coff[j][e] = col + e < N ? ix.c_col[col + e] : -1;
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
          const int64_t row = m0 + (wm * TM + i) * MT + rl0 + 8 * ps;
          roff[i][ps] = row < M ? ix.c_row[row] : -1;
        }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
#pragma unroll
          for (int r = 0; r < MF::NACC; ++r) st[MF::acc_row(r, lane)][MF::acc_col(lane)] = acc[i][j][r];
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          const bool run = coff[j][0] >= 0 && coff[j][3] == coff[j][0] + 3 && coff[j][1] == coff[j][0] + 1 &&
                           coff[j][2] == coff[j][0] + 2;
#pragma unroll
          for (int ps = 0; ps < 4; ++ps) {
            const float4 v = *reinterpret_cast<const float4*>(&st[rl0 + 8 * ps][cl]);
            const int64_t ro = roff[i][ps];
            if (ro < 0) continue;
            if (run && ((ro + coff[j][0]) & 3) == 0) {
              *reinterpret_cast<float4*>(C + ro + coff[j][0]) = v;
            } else {
              if (coff[j][0] >= 0) C[ro + coff[j][0]] = v.x;
              if (coff[j][1] >= 0) C[ro + coff[j][1]] = v.y;
              if (coff[j][2] >= 0) C[ro + coff[j][2]] = v.z;
              if (coff[j][3] >= 0) C[ro + coff[j][3]] = v.w;
            }
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();  // the patch is rewritten by the next tile
        }
      return;
    }
  }
  if (IDX && ix.c_row) {
    // table-addressed C: every offset this lane needs is requested first (TM * NACC row offsets, TN column offsets),
    // then the stores go out -- one dependent table load in front of every store made the epilogue a chain of
    // L2 round trips (the last chain product wrote the volume at 1 TB/s)
    int64_t roff[TM][MF::NACC], coff[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int64_t col = n0 + (wn * TN + j) * MT + MF::acc_col(lane);
      coff[j] = col < N ? ix.c_col[col] : -1;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < MF::NACC; ++r) {
        const int64_t row = m0 + (wm * TM + i) * MT + MF::acc_row(r, lane);
        roff[i][r] = row < M ? ix.c_row[row] : -1;
      }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < MF::NACC; ++r)
          if (roff[i][r] >= 0 && coff[j] >= 0) C[roff[i][r] + coff[j]] = acc[i][j][r];
    return;
  }
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int64_t col = n0 + (wn * TN + j) * MT + MF::acc_col(lane);
#pragma unroll
      for (int r = 0; r < MF::NACC; ++r) {
        const int64_t row = m0 + (wm * TM + i) * MT + MF::acc_row(r, lane);
        if (row < M && col < N) C[row * ldc + col] = acc[i][j][r];
      }
    }
}

template <typename T, int BM, int BN, int WAVES_M, int WAVES_N, bool TA, bool TB, bool VEC, bool IDX = false>
__global__ void __launch_bounds__(256, 2)
gemm_kernel(int64_t M, int64_t N, int64_t K, const T* __restrict__ A, int64_t lda,
            const T* __restrict__ B, int64_t ldb, T* __restrict__ C, int64_t ldc, GemmIndex ix = GemmIndex()) {
  gemm_body<T, BM, BN, WAVES_M, WAVES_N, TA, TB, VEC, IDX>(M, N, K, A, lda, B, ldb, C, ldc, ix);
}

// the same product for every operand triple of a batch (grid.z): what a lockstep group of volumes needs at a site
// of the sweep or a stage of the chain -- one launch instead of one per volume
template <typename T, int BM, int BN, int WAVES_M, int WAVES_N, bool TA, bool TB, bool VEC, bool IDX = false>
__global__ void __launch_bounds__(256, 2)
gemm_batched_kernel(int64_t M, int64_t N, int64_t K, GemmBatchPtrs p, int64_t lda, int64_t ldb, int64_t ldc,
                    GemmIndex ix = GemmIndex()) {
  gemm_body<T, BM, BN, WAVES_M, WAVES_N, TA, TB, VEC, IDX>(M, N, K, static_cast<const T*>(p.a[blockIdx.z]), lda,
                                                           static_cast<const T*>(p.b[blockIdx.z]), ldb,
                                                           static_cast<T*>(p.c[blockIdx.z]), ldc, ix);
}

template <typename T, int BM, int BN, int WAVES_M, int WAVES_N>
int launch_gemm(const ndmps::GemmPlan& plan, int transA, int transB, int64_t m, int64_t n, int64_t k, const T* A,
                int64_t lda, const T* B, int64_t ldb, T* C, int64_t ldc, hipStream_t stream, const GemmBatchPtrs* bp,
                int batch) {
  dim3 grid((unsigned)plan.grid_x, (unsigned)plan.grid_y, (unsigned)batch);
  dim3 block(256);
  GemmIndex gi{nullptr, nullptr, nullptr, nullptr, plan.guarded};
#define NDMPS_GEMM_LAUNCH(TA_, TB_, V_)                                                                            \
  do {                                                                                                              \
    if (bp)                                                                                                         \
      hipLaunchKernelGGL((gemm_batched_kernel<T, BM, BN, WAVES_M, WAVES_N, TA_, TB_, V_>), grid, block, 0, stream,  \
                         m, n, k, *bp, lda, ldb, ldc, gi);                                                          \
    else                                                                                                            \
      hipLaunchKernelGGL((gemm_kernel<T, BM, BN, WAVES_M, WAVES_N, TA_, TB_, V_>), grid, block, 0, stream, m, n, k,  \
                         A, lda, B, ldb, C, ldc, gi);                                                               \
  } while (0)
#define NDMPS_GEMM_TRANS(V_)                                     \
  do {                                                           \
    if (transA && transB) NDMPS_GEMM_LAUNCH(true, true, V_);     \
    else if (transA) NDMPS_GEMM_LAUNCH(true, false, V_);         \
    else if (transB) NDMPS_GEMM_LAUNCH(false, true, V_);         \
    else NDMPS_GEMM_LAUNCH(false, false, V_);                    \
  } while (0)
  if (plan.vec) NDMPS_GEMM_TRANS(true);
  else NDMPS_GEMM_TRANS(false);
#undef NDMPS_GEMM_TRANS
#undef NDMPS_GEMM_LAUNCH
  NDMPS_LAUNCH_CHECK();
  return NDMPS_OK;
}

template <typename T>
constexpr ndmps::GemmElem gemm_elem() {
  return sizeof(T) == 8 ? ndmps::GemmElem::F64 : ndmps::GemmElem::F32;
}

inline int64_t gemm_misalignment(const void* p) { return (int64_t)((uintptr_t)p % 64); }

template <typename T>
int gemm_check(int64_t m, int64_t n, int64_t k, const T* A, int64_t lda, int transA, const T* B,
               int64_t ldb, int transB, T* C, int64_t ldc) {
  NDMPS_REQUIRE(A && B && C, "NULL GEMM operand");
  const char* why = ndmps::gemm_refusal(gemm_elem<T>(), transA, transB, m, n, k, lda, ldb, ldc);
  NDMPS_REQUIRE(!why, "%s (m=%lld n=%lld k=%lld lda=%lld ldb=%lld ldc=%lld)", why, (long long)m, (long long)n,
                (long long)k, (long long)lda, (long long)ldb, (long long)ldc);
  return NDMPS_OK;
}

// One product, or the same product for every triple of a batch (bp): checked, planned (gemm_plan.h) and launched on
// the plan's tile.  The four dense entries are this function.
template <typename T>
int gemm_run(int transA, int transB, int64_t m, int64_t n, int64_t k, const T* A, int64_t lda, const T* B, int64_t ldb,
             T* C, int64_t ldc, ndmps_stream_t stream, const GemmBatchPtrs* bp, int batch) {
  if (bp) {
    A = static_cast<const T*>(bp->a[0]);
    B = static_cast<const T*>(bp->b[0]);
    C = static_cast<T*>(bp->c[0]);
  }
  NDMPS_TRY(gemm_check(m, n, k, A, lda, transA, B, ldb, transB, C, ldc));
  int64_t mis_a = gemm_misalignment(A), mis_b = gemm_misalignment(B), mis_c = gemm_misalignment(C);
  for (int z = 1; bp && z < batch; ++z) {  // one unaligned member takes the whole batch off the vector path
    mis_a |= gemm_misalignment(bp->a[z]);
    mis_b |= gemm_misalignment(bp->b[z]);
    mis_c |= gemm_misalignment(bp->c[z]);
  }
  const ndmps::GemmPlan plan = ndmps::gemm_plan(gemm_elem<T>(), transA, transB, m, n, k, lda, ldb, ldc, mis_a, mis_b,
                                                mis_c, gemm_guarded_env() != 0);
  if (plan.launches == 0) return NDMPS_OK;
  hipStream_t s = (hipStream_t)stream;
  if (bp) A = B = nullptr, C = nullptr;  // the batched kernels take their operands from bp
#define NDMPS_GEMM_TILE(BM_, BN_, WM_, WN_)  \
  if (plan.bm == BM_ && plan.bn == BN_)      \
  return launch_gemm<T, BM_, BN_, WM_, WN_>(plan, transA, transB, m, n, k, A, lda, B, ldb, C, ldc, s, bp, batch)
  if constexpr (sizeof(T) == 4) {
    NDMPS_GEMM_TILE(128, 32, 4, 1);
    NDMPS_GEMM_TILE(64, 64, 2, 2);
    NDMPS_GEMM_TILE(128, 128, 2, 2);
  } else {
    NDMPS_GEMM_TILE(64, 16, 4, 1);
    NDMPS_GEMM_TILE(32, 32, 2, 2);
    NDMPS_GEMM_TILE(64, 64, 2, 2);
  }
#undef NDMPS_GEMM_TILE
  ndmps::set_error("no kernel for the planned tile %d x %d", plan.bm, plan.bn);
  return NDMPS_EINVAL;
}

// table-addressed product on the plan's tile (64 x 64 or 128 x 128), one operand triple or a batch
int launch_gemm_indexed(const ndmps::GemmPlan& plan, int64_t m, int64_t n, int64_t k, const float* A, int64_t lda,
                        const float* B, int64_t ldb, float* C, int64_t ldc, const GemmIndex& ix, hipStream_t s,
                        const GemmBatchPtrs* bp, int batch) {
  const dim3 block(256);
  const dim3 grid((unsigned)plan.grid_x, (unsigned)plan.grid_y, (unsigned)batch);
#define NDMPS_GEMM_IDX(BM_, V_)                                                                                        \
  do {                                                                                                                  \
    if (bp)                                                                                                             \
      hipLaunchKernelGGL((gemm_batched_kernel<float, BM_, BM_, 2, 2, false, false, V_, true>), grid, block, 0, s, m, n,  \
                         k, *bp, lda, ldb, ldc, ix);                                                                    \
    else                                                                                                                \
      hipLaunchKernelGGL((gemm_kernel<float, BM_, BM_, 2, 2, false, false, V_, true>), grid, block, 0, s, m, n, k, A,    \
                         lda, B, ldb, C, ldc, ix);                                                                      \
  } while (0)
  if (plan.bm == 64) {
    if (plan.vec) NDMPS_GEMM_IDX(64, true);
    else NDMPS_GEMM_IDX(64, false);
  } else {
    if (plan.vec) NDMPS_GEMM_IDX(128, true);
    else NDMPS_GEMM_IDX(128, false);
  }
#undef NDMPS_GEMM_IDX
  NDMPS_LAUNCH_CHECK();
  return NDMPS_OK;
}

}  // namespace

extern "C" int ndmps_sgemm(int transA, int transB, int64_t m, int64_t n, int64_t k, const float* d_A,
                           int64_t lda, const float* d_B, int64_t ldb, float* d_C, int64_t ldc,
                           ndmps_stream_t stream) {
  return gemm_run<float>(transA, transB, m, n, k, d_A, lda, d_B, ldb, d_C, ldc, stream, nullptr, 1);
}

// C = A B (no transposes) with table-driven addressing of A and / or C (see GemmIndex): the reshape stage fused
// into a product of the sweep (A = the volume read through the permutation) or of the chain (C = the
// reconstructed volume written through the inverse permutation).  a_vec4: every aligned group of four
// consecutive k has consecutive offsets in d_a_col (16-byte loads allowed).
extern "C" int ndmps_sgemm_indexed(int64_t m, int64_t n, int64_t k, const float* d_A, int64_t lda,
                                   const int64_t* d_a_row, const int64_t* d_a_col, int a_vec4, const float* d_B,
                                   int64_t ldb, float* d_C, int64_t ldc, const int64_t* d_c_row,
                                   const int64_t* d_c_col, ndmps_stream_t stream) {
  NDMPS_REQUIRE(m >= 0 && n >= 0 && k >= 0 && d_A && d_B && d_C, "bad indexed GEMM argument");
  NDMPS_REQUIRE((d_a_row == nullptr) == (d_a_col == nullptr) && (d_c_row == nullptr) == (d_c_col == nullptr),
                "offset tables come in (row, column) pairs");
  NDMPS_REQUIRE(ldb >= n && (d_a_row || lda >= k) && (d_c_row || ldc >= n), "leading dimension too small");
  const ndmps::GemmPlan plan = ndmps::gemm_plan_indexed(m, n, k, lda, ldb, d_a_row != nullptr, a_vec4 != 0,
                                                        gemm_misalignment(d_A), gemm_misalignment(d_B),
                                                        gemm_guarded_env() != 0);
  if (plan.launches == 0) return NDMPS_OK;
  GemmIndex ix{d_a_row, d_a_col, d_c_row, d_c_col, plan.guarded};
  return launch_gemm_indexed(plan, m, n, k, d_A, lda, d_B, ldb, d_C, ldc, ix, (hipStream_t)stream, nullptr, 1);
}

extern "C" int ndmps_dgemm(int transA, int transB, int64_t m, int64_t n, int64_t k, const double* d_A,
                           int64_t lda, const double* d_B, int64_t ldb, double* d_C, int64_t ldc,
                           ndmps_stream_t stream) {
  return gemm_run<double>(transA, transB, m, n, k, d_A, lda, d_B, ldb, d_C, ldc, stream, nullptr, 1);
}

namespace {
template <typename T>
int gemm_batched_check(int batch, const T* const* h_A, const T* const* h_B, T* const* h_C, GemmBatchPtrs& bp) {
  NDMPS_REQUIRE(batch >= 1 && batch <= kGemmMaxBatch && h_A && h_B && h_C, "batched GEMM: batch=%d outside [1, %d] or NULL array",
                batch, kGemmMaxBatch);
  for (int z = 0; z < batch; ++z) {
    NDMPS_REQUIRE(h_A[z] && h_B[z] && h_C[z], "batched GEMM: NULL operand %d", z);
    bp.a[z] = h_A[z];
    bp.b[z] = h_B[z];
    bp.c[z] = h_C[z];
  }
  return NDMPS_OK;
}
}  // namespace

// `batch` (<= ndmps_gemm_batched_max()) products of one shape in one launch; h_A / h_B / h_C: HOST arrays of device
// pointers.  Same tiles and arithmetic as ndmps_sgemm / ndmps_dgemm on each triple.
extern "C" int ndmps_gemm_batched_max(void) { return kGemmMaxBatch; }

extern "C" int ndmps_sgemm_batched(int batch, int transA, int transB, int64_t m, int64_t n, int64_t k,
                                   const float* const* h_A, int64_t lda, const float* const* h_B, int64_t ldb,
                                   float* const* h_C, int64_t ldc, ndmps_stream_t stream) {
  GemmBatchPtrs bp;
  NDMPS_TRY(gemm_batched_check(batch, h_A, h_B, h_C, bp));
  return gemm_run<float>(transA, transB, m, n, k, nullptr, lda, nullptr, ldb, nullptr, ldc, stream, &bp, batch);
}

extern "C" int ndmps_dgemm_batched(int batch, int transA, int transB, int64_t m, int64_t n, int64_t k,
                                   const double* const* h_A, int64_t lda, const double* const* h_B, int64_t ldb,
                                   double* const* h_C, int64_t ldc, ndmps_stream_t stream) {
  GemmBatchPtrs bp;
  NDMPS_TRY(gemm_batched_check(batch, h_A, h_B, h_C, bp));
  return gemm_run<double>(transA, transB, m, n, k, nullptr, lda, nullptr, ldb, nullptr, ldc, stream, &bp, batch);
}

// The plan a dense product would launch by, for tests and tools (slot order: include/ndmps_hip.h).  Host arithmetic
// only: no GPU call.  The entries above go through the same gemm_plan.
extern "C" int ndmps_gemm_plan_query(int elem, int transA, int transB, int64_t m, int64_t n, int64_t k, int64_t lda,
                                     int64_t ldb, int64_t ldc, int64_t mis_a, int64_t mis_b, int64_t mis_c, int guarded,
                                     int64_t* h_out) {
  NDMPS_REQUIRE(h_out && elem >= 0 && elem <= 2, "bad GEMM plan query (elem=%d)", elem);
  NDMPS_REQUIRE(mis_a >= 0 && mis_b >= 0 && mis_c >= 0, "a misalignment is a byte count");
  const ndmps::GemmElem e = (ndmps::GemmElem)elem;
  const char* why = ndmps::gemm_refusal(e, transA, transB, m, n, k, lda, ldb, ldc);
  NDMPS_REQUIRE(!why, "%s", why);
  const ndmps::GemmPlan p = ndmps::gemm_plan(e, transA, transB, m, n, k, lda, ldb, ldc, mis_a, mis_b, mis_c, guarded != 0);
  const int64_t out[NDMPS_GEMM_PLAN_SLOTS] = {p.bm,      p.bn,      p.vec,    p.va,      p.vb,         p.grid_x,  p.grid_y,
                                              p.inner_a, p.inner_b, p.vec_in, p.vec_out, p.transposes, p.launches};
  std::copy(out, out + NDMPS_GEMM_PLAN_SLOTS, h_out);
  return NDMPS_OK;
}

// ----------------------------------------------------------------------------------
// C = A W for A = a lockstep group's volumes read through the permutation tables as (m x 64) matrices -- the first
// projection of a bond cap of 32 (BASELINE configs 2 and 4): a 64 MB stream per 256^3 volume, 96 MB with the result.
// The tile kernel reads it at 2.8 TB/s (1.1 ms per group of 32).  Here, as in gram64_stream_kernel, a lane's 16-byte
// load is four MFMA operands: lane (i, h) = (lane % 32, lane / 32) of v_mfma_f32_32x32x2_f32 takes columns
// 8q + 4h .. 8q + 4h + 3 of row i of a 32-row tile (columns in memory order: aligned quads are contiguous), its
// component c is the A operand of the k-pair {8q + c, 8q + 4 + c}; the matching W rows sit in LDS as 16-byte records
// [q][h][j] = (W[8q + 4h + c][j])_c.  Rows are visited in ascending order of their offsets (d_row_sorted): the 32
// lanes of a half-wave read 512 contiguous bytes; row s of that order is row d_row_order[s] of C.  No barrier in the
// loop; the eight loads of the next tile are issued slot by slot as the current tile's steps consume theirs.
// NB = n / 32 (n = 32 or 64 columns of W).
namespace {
template <int NB>
__global__ void __launch_bounds__(256, 2)
proj64_stream_kernel(GemmBatchPtrs ptrs, int64_t m, int64_t ldb, int64_t ldc, const int64_t* __restrict__ row_sorted,
                     const int32_t* __restrict__ row_order, const int64_t* __restrict__ col_off, int64_t tiles_per_wg) {
  constexpr int N = 32 * NB, Q = 8;
  const float* A = static_cast<const float*>(ptrs.a[blockIdx.z]);
  const float* W = static_cast<const float*>(ptrs.b[blockIdx.z]);
  float* C = static_cast<float*>(ptrs.c[blockIdx.z]);
  __shared__ __attribute__((aligned(16))) float Wp[Q * 2 * N * 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int e = tid; e < 64 * N; e += 256) {
    const int kidx = e / N, j = e % N;
    const int q = kidx >> 3, h = (kidx >> 2) & 1, c = kidx & 3;
    Wp[((q * 2 + h) * N + j) * 4 + c] = W[(int64_t)kidx * ldb + j];
  }
  __syncthreads();
  const int li = lane & 31, h = lane >> 5;
  int64_t coff[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) coff[q] = col_off[8 * q + 4 * h];
  const int64_t n_tiles = (m + 31) / 32;
  const int64_t t_begin = (int64_t)blockIdx.y * tiles_per_wg, t_end = min(n_tiles, t_begin + tiles_per_wg);
  // this wave's tiles: t_begin + wave, + 4, ...; a tile index beyond the end repeats the last row (never stored)
  auto row_offset = [&](int64_t t) { return row_sorted[min(32 * t + li, m - 1)]; };
  int64_t t = t_begin + wave;
  if (t >= t_end) return;
  float4 ring[Q];
  int64_t roff = row_offset(t), roff_next = row_offset(t + 4);
#pragma unroll
  for (int q = 0; q < Q; ++q) ring[q] = load4_stream_f32(A + roff + coff[q]);
  for (; t < t_end; t += 4) {
    f32x16 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nb][r] = 0.0f;
    const int64_t roff_after = row_offset(t + 8);
    // the tile's sixteen output rows of this lane, requested before the next tile's loads (a load issued behind them,
    // inside the guarded stores, would make every store wait for the whole ring)
    int crow_of[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) crow_of[r] = row_order[min(32 * t + (r & 3) + 8 * (r >> 2) + 4 * h, m - 1)];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      // the step's operands leave the slot BEFORE it is reloaded in place (opaque copies: used from the slot itself, the
      // last MFMAs of the step would read registers an already issued load may overwrite, and the compiler answers
      // with a second set of registers and copies that wait for the loads they follow)
      float4 a = ring[q];
      asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z), "+v"(a.w));
      float4 bq[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) bq[nb] = *reinterpret_cast<const float4*>(&Wp[((q * 2 + h) * N + 32 * nb + li) * 4]);
      __builtin_amdgcn_sched_barrier(0);
      ring[q] = load4_stream_f32(A + roff_next + coff[q]);  // the same step of the wave's next tile
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bq[nb].x, acc[nb], 0, 0, 0);
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bq[nb].y, acc[nb], 0, 0, 0);
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bq[nb].z, acc[nb], 0, 0, 0);
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bq[nb].w, acc[nb], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    roff_next = roff_after;
    // accumulator register r of lane (j, h) is row (r & 3) + 8 (r >> 2) + 4 h of the tile, column j
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t s = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (s < m) {
        float* crow = C + (int64_t)crow_of[r] * ldc + li;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) crow[32 * nb] = acc[nb][r];
      }
    }
  }
}

}  // namespace

// batched C = A B with table-driven addressing (one set of tables for the whole batch: the volumes of a lockstep
// group share the index permutation); see ndmps_sgemm_indexed
extern "C" int ndmps_sgemm_indexed_batched(int batch, int64_t m, int64_t n, int64_t k, const float* const* h_A,
                                           int64_t lda, const int64_t* d_a_row, const int64_t* d_a_col, int a_vec4,
                                           const float* const* h_B, int64_t ldb, float* const* h_C, int64_t ldc,
                                           const int64_t* d_c_row, const int64_t* d_c_col, ndmps_stream_t stream) {
  GemmBatchPtrs bp;
  NDMPS_TRY(gemm_batched_check(batch, h_A, h_B, h_C, bp));
  NDMPS_REQUIRE(m >= 0 && n >= 0 && k >= 0, "bad indexed GEMM extent");
  NDMPS_REQUIRE((d_a_row == nullptr) == (d_a_col == nullptr) && (d_c_row == nullptr) == (d_c_col == nullptr),
                "offset tables come in (row, column) pairs");
  NDMPS_REQUIRE(ldb >= n && (d_a_row || lda >= k) && (d_c_row || ldc >= n), "leading dimension too small");
  int64_t mis_a = 0, mis_b = 0;
  for (int z = 0; z < batch; ++z) {
    mis_a |= gemm_misalignment(bp.a[z]);
    mis_b |= gemm_misalignment(bp.b[z]);
  }
  const ndmps::GemmPlan plan =
      ndmps::gemm_plan_indexed(m, n, k, lda, ldb, d_a_row != nullptr, a_vec4 != 0, mis_a, mis_b, gemm_guarded_env() != 0);
  if (plan.launches == 0) return NDMPS_OK;
  GemmIndex ix{d_a_row, d_a_col, d_c_row, d_c_col, plan.guarded};
  return launch_gemm_indexed(plan, m, n, k, nullptr, lda, nullptr, ldb, nullptr, ldc, ix, (hipStream_t)stream, &bp, batch);
}

// The first projection of the fused sweep for 64 gathered columns, as a stream (proj64_stream_kernel): C[b] (m x n,
// n = 32 or 64, row-major with leading dimension ldc) = A[b] W[b], element (r, c) of A[b] at
// h_A[b][d_row_off[r] + d_col_off[c]].  d_row_sorted: d_row_off in ascending order; d_row_order[s]: the row whose offset
// is d_row_sorted[s].  NDMPS_EINVAL for shapes the kernel does not take (the caller keeps ndmps_sgemm_indexed_batched).
extern "C" int ndmps_sgemm_gathered64_stream_batched(int batch, int64_t m, int64_t n, const float* const* h_A,
                                                     const int64_t* d_row_sorted, const int32_t* d_row_order,
                                                     const int64_t* d_col_off, const float* const* h_B, int64_t ldb,
                                                     float* const* h_C, int64_t ldc, ndmps_stream_t stream) {
  GemmBatchPtrs bp;
  NDMPS_TRY(gemm_batched_check(batch, h_A, h_B, h_C, bp));
  NDMPS_REQUIRE(d_row_sorted && d_row_order && d_col_off, "NULL table");
  NDMPS_REQUIRE(m >= 1 && (n == 32 || n == 64) && ldb >= n && ldc >= n, "the stream takes 32 or 64 result columns");
  for (int z = 0; z < batch; ++z) NDMPS_REQUIRE((uintptr_t)bp.a[z] % 16 == 0, "operand %d is not 16-byte aligned", z);
  hipStream_t s = (hipStream_t)stream;
  const int64_t n_tiles = ndmps::ceil_div(m, 32);
  // ~4 workgroups per CU over the batch (two resident), whole multiples of the four tiles a workgroup's waves take
  const int64_t want = std::max<int64_t>(1, ndmps::ceil_div((int64_t)4 * ndmps::kNumCU, batch));
  const int64_t tiles_per_wg = ndmps::round_up(std::max<int64_t>(ndmps::ceil_div(n_tiles, want), 4), 4);
  const dim3 grid(1, (unsigned)ndmps::ceil_div(n_tiles, tiles_per_wg), (unsigned)batch);
  if (n == 32)
    hipLaunchKernelGGL(proj64_stream_kernel<1>, grid, dim3(256), 0, s, bp, m, ldb, ldc, d_row_sorted, d_row_order, d_col_off,
                       tiles_per_wg);
  else
    hipLaunchKernelGGL(proj64_stream_kernel<2>, grid, dim3(256), 0, s, bp, m, ldb, ldc, d_row_sorted, d_row_order, d_col_off,
                       tiles_per_wg);
  NDMPS_LAUNCH_CHECK();
  return NDMPS_OK;
}
