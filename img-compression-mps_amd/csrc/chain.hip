// Decode: the chain contraction and the overlap of two MPS.
//
//   ndmps_chain_contract_f32  <- `mps ^ ...`                           (core/ndmps.py:140)
//   ndmps_overlap_f32         <- `mps @ mps`                           (core/ndmps.py:76,86)
//
// Chain: left->right like quimb's structured contraction, with the tail pre-contracted (chain_plan.h), so the tensor
// itself is written ONCE, by the last GEMM Left (M_{j0} x k_{j0}) R.  The cumulative chain alone would write an
// N-element intermediate per trailing site and read it back (2 x 64 MB per site at 256^3 for multiplications by
// 64 x 64 and 8 x 8 matrices).  Same fp32 products, different association.  Every decision -- the tail, the order of
// the products, the buffer each one reads and writes, the workspace layout -- is made by chain_plan; every entry
// plans, checks its arguments against the plan (chain_check) and runs it (run_chain).
#include <type_traits>
#include <vector>

#include "chain_plan.h"
#include "common.h"
#include "typed.h"

using ndmps::Arena;
using ndmps::ChainKind;
using ndmps::ChainPlan;
using ndmps::ChainProduct;

namespace {
struct ChainScatter {          // inverse permutation in the epilogue of the last product (fp32 only)
  const int64_t* row_off;      // [numel / n_cols] offset of tail-block r in the C-order volume
  const int64_t* col_off;      // [n_cols] offsets inside a block, ASCENDING (memory order)
  const int32_t* col_perm;     // [n_cols] site-order column of the c-th smallest offset
  int64_t n_cols;
};

constexpr int kChainGroup = 64;  // volumes of one batched launch
struct PtrPairs {                // operands of a small per-volume kernel run for a whole group (grid.y)
  const void* in[kChainGroup];
  void* out[kChainGroup];
};
// out (rows x cols) <- the columns perm[0], perm[1], ... of in, for volume blockIdx.y
__global__ void __launch_bounds__(256)
gather_cols_kernel(PtrPairs pp, int64_t rows, int64_t cols, const int32_t* __restrict__ perm) {
  const float* in = static_cast<const float*>(pp.in[blockIdx.y]);
  float* out = static_cast<float*>(pp.out[blockIdx.y]);
  const int64_t total = rows * cols;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256)
    out[e] = in[(e / cols) * cols + perm[e % cols]];
}

// The argument check of every chain entry, before its first launch: `count` volumes with the bonds of the plan,
// volume b with cores[b L ..] and outs[b]; ws_each: bytes of workspace each volume may use.
template <typename T>
int chain_check(const ChainPlan& p, int count, const int64_t* dims, const int64_t* bonds, const T* const* cores,
                T* const* outs, const void* d_ws, int64_t ws_each, const ChainScatter* scatter) {
  const int L = p.L;
  NDMPS_REQUIRE(cores && outs && outs[0], "bad chain argument");
  NDMPS_REQUIRE(bonds[0] == 1 && bonds[L] == 1, "open boundary bonds must be 1");
  for (int i = 0; i < L; ++i)
    NDMPS_REQUIRE(dims[i] >= 1 && cores[i], "dims[%d] must be positive and core %d non-NULL", i, i);
  for (int b = 1; b < count; ++b) {
    NDMPS_REQUIRE(outs[b], "NULL output %d", b);
    for (int i = 0; i < L; ++i) NDMPS_REQUIRE(cores[(int64_t)b * L + i], "core %d of volume %d is NULL", i, b);
  }
  // every intermediate lands in the workspace or in the output (N = prod(dims) elements): every bond must be at most
  // the product of the site dims on either side of it, as any MPS of a dense tensor has
  int64_t left = 1;
  for (int i = 0; i < L; ++i) {
    left *= dims[i];
    NDMPS_REQUIRE(bonds[i + 1] >= 1 && bonds[i + 1] <= left && bonds[i + 1] <= p.numel / left,
                  "bond %d = %lld exceeds min(%lld, %lld), the rank any unfolding can have", i + 1,
                  (long long)bonds[i + 1], (long long)left, (long long)(p.numel / left));
  }
  if (!d_ws || ws_each < p.total_bytes) {
    ndmps::set_error("chain workspace too small: %lld < %lld", (long long)ws_each, (long long)p.total_bytes);
    return NDMPS_EWORKSPACE;
  }
  // the cumulative products may already write the output (a single site is copied and has no use for the tables)
  if (scatter && L > 1)
    NDMPS_REQUIRE(p.has_tail() && scatter->n_cols == p.tail_cols,
                  "scatter tables are for %lld tail columns, the chain's tail has %lld", (long long)scatter->n_cols,
                  (long long)p.tail_cols);
  return NDMPS_OK;
}

// Runs the plan for `count` checked volumes, volume b in the workspace slice d_ws + b ws_each.  One volume: one GEMM
// of the storage type per product.  A group (fp32 with the scatter epilogue only; the last group of a batch may hold
// one volume): one batched GEMM per product, the same products in the same order on each volume, so the results are
// bit-identical to one volume at a time.
template <typename T>
int run_chain(const ChainPlan& p, int count, bool group, const T* const* cores, T* const* outs, void* d_ws,
              int64_t ws_each, const ChainScatter* scatter, hipStream_t s) {
  constexpr bool kF32 = std::is_same<T, float>::value;
  NDMPS_REQUIRE(group ? kF32 && scatter && count <= kChainGroup : count == 1, "internal: a group is fp32 with scatter");
  if (p.L == 1) {
    NDMPS_CHECK_HIP(hipMemcpyAsync(outs[0], cores[0], p.numel * sizeof(T), hipMemcpyDeviceToDevice, s));
    return NDMPS_OK;
  }
  NDMPS_REQUIRE(p.products.back().c == ndmps::kChainOut, "internal: chain result landed in the wrong buffer");
  auto at = [&](int id, int b) -> T* {
    char* ws = (char*)d_ws + (int64_t)b * ws_each;
    switch (id) {
      case ndmps::kChainLeft: return (T*)(ws + p.off_left);
      case ndmps::kChainTail0: return (T*)(ws + p.off_tail0);
      case ndmps::kChainTail1: return (T*)(ws + p.off_tail1);
      case ndmps::kChainOut: return outs[b];
      default: return const_cast<T*>(cores[(int64_t)b * p.L + id]);
    }
  };
  // scratch behind the three buffers (bf16: transposed right operands)
  char* tws = (char*)d_ws + p.off_scratch;
  tws += (256 - ((uintptr_t)tws & 255)) & 255;
  const int64_t tws_bytes = ((char*)d_ws + ws_each) - tws;
  std::vector<const T*> A(count), B(count);
  std::vector<T*> C(count);
  for (const ChainProduct& q : p.products) {
    for (int b = 0; b < count; ++b) {
      A[b] = at(q.a, b);
      B[b] = at(q.b, b);
      C[b] = at(q.c, b);
    }
    if constexpr (kF32) {
      if (q.kind == ChainKind::Final && scatter) {
        // columns of R in memory order of the volume, then every element goes straight to its voxel
        PtrPairs pp;
        for (int b = 0; b < count; ++b) {
          float* spare = at(q.spare, b);
          pp.in[b] = B[b];
          pp.out[b] = spare;
          B[b] = spare;
        }
        hipLaunchKernelGGL(gather_cols_kernel, dim3(grid1d(q.k * q.n), count), dim3(256), 0, s, pp, q.k, q.n,
                           scatter->col_perm);
        NDMPS_LAUNCH_CHECK();
        if (!group)
          return ndmps_sgemm_indexed(q.m, q.n, q.k, A[0], q.k, nullptr, nullptr, 0, B[0], q.n, C[0], 0, scatter->row_off,
                                     scatter->col_off, s);
        return ndmps_sgemm_indexed_batched(count, q.m, q.n, q.k, A.data(), q.k, nullptr, nullptr, 0, B.data(), q.n,
                                           C.data(), 0, scatter->row_off, scatter->col_off, s);
      }
      if (group) {
        NDMPS_TRY(ndmps_sgemm_batched(count, 0, 0, q.m, q.n, q.k, A.data(), q.k, B.data(), q.n, C.data(), q.n, s));
        continue;
      }
    }
    NDMPS_TRY(gemm_T(0, q.m, q.n, q.k, A[0], B[0], q.n, C[0], tws, tws_bytes, s));
  }
  return NDMPS_OK;
}

// check, plan and run one volume
template <typename T>
int chain_one(int L, const int64_t* h_dims, const int64_t* h_bonds, const T* const* h_cores, T* d_out, void* d_ws,
              int64_t ws_bytes, ndmps_stream_t stream, const ChainScatter* scatter = nullptr) {
  NDMPS_REQUIRE(L >= 1 && h_dims && h_bonds, "bad chain argument");
  const ChainPlan p = ndmps::chain_plan(L, h_dims, h_bonds, sizeof(T) == 8 ? 8 : 4);  // bf16: the fp32 layout
  NDMPS_TRY(chain_check(p, 1, h_dims, h_bonds, h_cores, &d_out, d_ws, ws_bytes, scatter));
  return run_chain(p, 1, false, h_cores, &d_out, d_ws, ws_bytes, scatter, (hipStream_t)stream);
}

int64_t chain_workspace(int L, const int64_t* h_dims, const int64_t* h_bonds, int64_t elem_bytes) {
  if (L < 1 || !h_dims || !h_bonds) return 0;
  return ndmps::chain_plan(L, h_dims, h_bonds, elem_bytes).total_bytes;
}

// Workspace slices of a batch: MPS that share their bonds run min(batch, 64) at a time, each in a slice of *each
// bytes; any other batch runs one volume at a time in one slice that fits the largest.
int chain_slices(int batch, int L, const int64_t* h_dims, const int64_t* h_bonds, int64_t* each) {
  bool same = true;
  for (int b = 1; b < batch && same; ++b)
    for (int i = 0; i <= L; ++i) same = same && h_bonds[(int64_t)b * (L + 1) + i] == h_bonds[i];
  *each = 0;
  for (int b = 0; b < (same ? 1 : batch); ++b)
    *each = std::max(*each, chain_workspace(L, h_dims, h_bonds + (int64_t)b * (L + 1), sizeof(float)));
  *each = ndmps::round_up(*each, 256);
  return same ? std::min(batch, kChainGroup) : 1;
}
}  // namespace

extern "C" int64_t ndmps_chain_workspace_bytes(int L, const int64_t* h_dims, const int64_t* h_bonds) {
  return chain_workspace(L, h_dims, h_bonds, sizeof(float));
}
extern "C" int64_t ndmps_chain_workspace_bytes_f64(int L, const int64_t* h_dims, const int64_t* h_bonds) {
  return chain_workspace(L, h_dims, h_bonds, sizeof(double));
}
// number of trailing columns the chain pre-contracts (product of the dims of the tail sites), 0 if none
extern "C" int64_t ndmps_chain_tail_columns(int L, const int64_t* h_dims) {
  if (L < 2 || !h_dims) return 0;
  const std::vector<int64_t> ones(L + 1, 1);  // the tail depends on the dims alone
  return ndmps::chain_plan(L, h_dims, ones.data(), sizeof(float)).tail_cols;
}
extern "C" int64_t ndmps_chain_batched_workspace_bytes(int batch, int L, const int64_t* h_dims, const int64_t* h_bonds) {
  if (batch < 1 || L < 1 || !h_dims || !h_bonds) return 0;
  int64_t each = 0;
  const int slices = chain_slices(batch, L, h_dims, h_bonds, &each);
  return each * slices;
}

// The plan of a chain, for tests and tools (slot order: include/ndmps_hip.h).  Host arithmetic only: no GPU call.
extern "C" int ndmps_chain_plan_query(int elem, int L, const int64_t* h_dims, const int64_t* h_bonds, int64_t* h_out) {
  NDMPS_REQUIRE(h_out && elem >= 0 && elem <= 2 && L >= 1 && h_dims && h_bonds, "bad chain plan query (elem=%d)", elem);
  const ChainPlan p = ndmps::chain_plan(L, h_dims, h_bonds, elem == 2 ? 8 : 4);
  const int64_t head[6] = {p.j0, p.tail_cols, (int64_t)p.products.size(), p.left_elems, p.tail_elems, p.total_bytes};
  h_out = std::copy(head, head + 6, h_out);
  for (const ChainProduct& q : p.products) {
    const int64_t row[8] = {(int64_t)q.kind, q.m, q.n, q.k, q.a, q.b, q.c, q.spare};
    h_out = std::copy(row, row + 8, h_out);
  }
  return NDMPS_OK;
}

extern "C" int ndmps_chain_contract_f32(int L, const int64_t* h_dims, const int64_t* h_bonds,
                                        const float* const* h_cores, float* d_dense, void* d_ws,
                                        int64_t ws_bytes, ndmps_stream_t stream) {
  return chain_one<float>(L, h_dims, h_bonds, h_cores, d_dense, d_ws, ws_bytes, stream);
}
extern "C" int ndmps_chain_contract_bf16(int L, const int64_t* h_dims, const int64_t* h_bonds,
                                         const void* const* h_cores, void* d_dense, void* d_ws,
                                         int64_t ws_bytes, ndmps_stream_t stream) {
  return chain_one<__bf16>(L, h_dims, h_bonds, (const __bf16* const*)h_cores, (__bf16*)d_dense, d_ws, ws_bytes, stream);
}
// fp64 cores: every product on the fp64 MFMA (workspace: ndmps_chain_workspace_bytes_f64)
extern "C" int ndmps_chain_contract_f64(int L, const int64_t* h_dims, const int64_t* h_bonds,
                                        const double* const* h_cores, double* d_dense, void* d_ws,
                                        int64_t ws_bytes, ndmps_stream_t stream) {
  return chain_one<double>(L, h_dims, h_bonds, h_cores, d_dense, d_ws, ws_bytes, stream);
}

// Chain contraction that writes the C-order VOLUME: the inverse index permutation (core/ndmps.py:144-148) rides
// on the last product, every element goes from the accumulator to its voxel (d_row_off / d_col_off /
// d_col_perm: ndmps_plan_split_offsets for n_cols = ndmps_chain_tail_columns, columns sorted by offset).  The
// site-order tensor is never written.
extern "C" int ndmps_chain_contract_scatter_f32(int L, const int64_t* h_dims, const int64_t* h_bonds,
                                                const float* const* h_cores, float* d_out,
                                                const int64_t* d_row_off, const int64_t* d_col_off,
                                                const int32_t* d_col_perm, int64_t n_cols, void* d_ws,
                                                int64_t ws_bytes, ndmps_stream_t stream) {
  NDMPS_REQUIRE(d_row_off && d_col_off && d_col_perm && n_cols >= 1, "NULL scatter table");
  const ChainScatter sc{d_row_off, d_col_off, d_col_perm, n_cols};
  return chain_one<float>(L, h_dims, h_bonds, h_cores, d_out, d_ws, ws_bytes, stream, &sc);
}

// The same for a list of MPS over the same sites (conv_to_tensors, evaluation/benchmark.py:80-100): volume b has
// bonds h_bonds[b (L + 1) ..], cores h_cores[b L ..] and goes to h_out[b].  MPS that share their bonds (a lockstep
// group whose caps bind) go through the chain TOGETHER, one batched launch per product, each in its own slice of
// d_ws (ndmps_chain_batched_workspace_bytes); otherwise, or in a workspace without room for the slices, the volumes
// are contracted in turn.  Bit-identical to ndmps_chain_contract_scatter_f32 on each volume either way.
extern "C" int ndmps_chain_contract_scatter_batched_f32(int batch, int L, const int64_t* h_dims, const int64_t* h_bonds,
                                                        const float* const* h_cores, float* const* h_out,
                                                        const int64_t* d_row_off, const int64_t* d_col_off,
                                                        const int32_t* d_col_perm, int64_t n_cols, void* d_ws,
                                                        int64_t ws_bytes, ndmps_stream_t stream) {
  NDMPS_REQUIRE(batch >= 1 && L >= 1 && h_dims && h_bonds && h_cores && h_out, "bad batched chain argument");
  NDMPS_REQUIRE(d_row_off && d_col_off && d_col_perm && n_cols >= 1, "NULL scatter table");
  const ChainScatter sc{d_row_off, d_col_off, d_col_perm, n_cols};
  int64_t each = 0;
  const int slices = chain_slices(batch, L, h_dims, h_bonds, &each);
  const ChainPlan p = ndmps::chain_plan(L, h_dims, h_bonds, sizeof(float));
  if (slices > 1 && p.has_tail() && d_ws && ws_bytes >= each * slices) {
    NDMPS_TRY(chain_check(p, batch, h_dims, h_bonds, h_cores, h_out, d_ws, each, &sc));
    for (int base = 0; base < batch; base += kChainGroup)
      NDMPS_TRY(run_chain(p, std::min(kChainGroup, batch - base), true, h_cores + (int64_t)base * L, h_out + base, d_ws, each,
                          &sc, (hipStream_t)stream));
    return NDMPS_OK;
  }
  for (int b = 0; b < batch; ++b)
    NDMPS_TRY(chain_one<float>(L, h_dims, h_bonds + (int64_t)b * (L + 1), h_cores + (int64_t)b * L, h_out[b], d_ws, ws_bytes,
                               stream, &sc));
  return NDMPS_OK;
}

// =================================================================== overlap
namespace {
__global__ void set_scalar_f64_kernel(double* p, double v) { *p = v; }

struct OverlapBuffers {
  double* E[2];    // transfer matrix, ping and pong
  double *A, *B;   // one core of either state in fp64
  double* X;       // E^T A
};
void carve_overlap(Arena& ar, int L, const int64_t* dims, const int64_t* bonds_a, const int64_t* bonds_b, OverlapBuffers& o) {
  int64_t emax = 1, amax = 1, bmax = 1, xmax = 1;
  for (int i = 0; i < L; ++i) {
    emax = std::max(emax, bonds_a[i + 1] * bonds_b[i + 1]);
    amax = std::max(amax, bonds_a[i] * dims[i] * bonds_a[i + 1]);
    bmax = std::max(bmax, bonds_b[i] * dims[i] * bonds_b[i + 1]);
    xmax = std::max(xmax, bonds_b[i] * dims[i] * bonds_a[i + 1]);
  }
  o.E[0] = ar.take<double>(emax);
  o.E[1] = ar.take<double>(emax);
  o.A = ar.take<double>(amax);
  o.B = ar.take<double>(bmax);
  o.X = ar.take<double>(xmax);
}
}  // namespace
extern "C" int64_t ndmps_overlap_workspace_bytes(int L, const int64_t* h_dims, const int64_t* h_bonds_a,
                                                 const int64_t* h_bonds_b) {
  if (L < 1 || !h_dims || !h_bonds_a || !h_bonds_b) return 0;
  Arena sizing(nullptr, 0);
  OverlapBuffers unused;
  carve_overlap(sizing, L, h_dims, h_bonds_a, h_bonds_b, unused);
  return ndmps::round_up(sizing.used, 256) + 256;
}

namespace {
template <typename T>
int overlap_impl(int L, const int64_t* h_dims, const int64_t* h_bonds_a, const T* const* h_cores_a,
                 const int64_t* h_bonds_b, const T* const* h_cores_b, double* h_out, void* d_ws, int64_t ws_bytes,
                 ndmps_stream_t stream) {
  NDMPS_REQUIRE(L >= 1 && h_dims && h_bonds_a && h_bonds_b && h_cores_a && h_cores_b && h_out,
                "bad overlap argument");
  const int64_t need = ndmps_overlap_workspace_bytes(L, h_dims, h_bonds_a, h_bonds_b);
  if (!d_ws || ws_bytes < need) {
    ndmps::set_error("overlap workspace too small: %lld < %lld", (long long)ws_bytes, (long long)need);
    return NDMPS_EWORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  Arena ar(d_ws, ws_bytes);
  OverlapBuffers o;
  carve_overlap(ar, L, h_dims, h_bonds_a, h_bonds_b, o);
  NDMPS_REQUIRE(ar.fits(), "workspace carve failed");
  double *const *E = o.E, *A = o.A, *B = o.B, *X = o.X;

  hipLaunchKernelGGL(set_scalar_f64_kernel, dim3(1), dim3(1), 0, s, E[0], 1.0);  // no copy from pageable host memory
  int cur = 0;
  for (int i = 0; i < L; ++i) {
    const int64_t ca = h_bonds_a[i], ca2 = h_bonds_a[i + 1];
    const int64_t cb = h_bonds_b[i], cb2 = h_bonds_b[i + 1];
    const int64_t d = h_dims[i];
    hipLaunchKernelGGL(f32_to_f64_kernel<T>, dim3(grid1d(ca * d * ca2)), dim3(256), 0, s, h_cores_a[i], ca * d * ca2, A);
    hipLaunchKernelGGL(f32_to_f64_kernel<T>, dim3(grid1d(cb * d * cb2)), dim3(256), 0, s, h_cores_b[i], cb * d * cb2, B);
    NDMPS_LAUNCH_CHECK();
    // X (cb, d ca2) = E^T (cb, ca) A (ca, d ca2)
    NDMPS_TRY(ndmps_dgemm(1, 0, cb, d * ca2, ca, E[cur], cb, A, d * ca2, X, d * ca2, s));
    // E' (ca2, cb2) = X'^T B' with X' = (cb d, ca2), B' = (cb d, cb2)
    NDMPS_TRY(ndmps_dgemm(1, 0, ca2, cb2, cb * d, X, ca2, B, cb2, E[cur ^ 1], cb2, s));
    cur ^= 1;
  }
  NDMPS_CHECK_HIP(hipMemcpyAsync(h_out, E[cur], sizeof(double), hipMemcpyDeviceToHost, s));
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));
  return NDMPS_OK;
}
}  // namespace

extern "C" int ndmps_overlap_f32(int L, const int64_t* h_dims, const int64_t* h_bonds_a,
                                 const float* const* h_cores_a, const int64_t* h_bonds_b,
                                 const float* const* h_cores_b, double* h_out, void* d_ws,
                                 int64_t ws_bytes, ndmps_stream_t stream) {
  return overlap_impl<float>(L, h_dims, h_bonds_a, h_cores_a, h_bonds_b, h_cores_b, h_out, d_ws, ws_bytes, stream);
}
// fp64 cores (same workspace query)
extern "C" int ndmps_overlap_f64(int L, const int64_t* h_dims, const int64_t* h_bonds_a,
                                 const double* const* h_cores_a, const int64_t* h_bonds_b,
                                 const double* const* h_cores_b, double* h_out, void* d_ws,
                                 int64_t ws_bytes, ndmps_stream_t stream) {
  return overlap_impl<double>(L, h_dims, h_bonds_a, h_cores_a, h_bonds_b, h_cores_b, h_out, d_ws, ws_bytes, stream);
}
