// Region decode: the values of a set of voxels straight from the cores, without the full volume.
// Replaces to_tensor()[key] (core/ndmps.py:131-153 of the reference decodes everything, then indexes).
//
// The host planner (core/region.py) lists, per site s < L-1, the live prefixes after site s: node k has a parent
// node of the previous level (the root, a 1 x 1 matrix holding 1, for s = 0) and the physical index phys[k] of
// site s.  Level s is one gathered product
//     E_s[k, :] = E_{s-1}[parent[k], :] . A_s[:, phys[k], :]
// with the nodes sorted by phys and cut into tiles of up to 32 rows that share phys, so a tile is a 32 x chi_r
// GEMM over gathered rows on the matrix cores (v_mfma_f32_32x32x2_f32 / v_mfma_f64_16x16x4_f64, A/B lane maps as
// in gemm.hip).  The last site has chi_{L} = 1: each output element is a dot product of its parent row with a
// column of A_{L-1}, written straight to its place in the C-order result.
//
// Tables (int32, one buffer, in this order): for s = 0 .. L-2, parent[nodes_s] then (phys, row0, count) for each of
// tiles_s tiles; then leaf_parent[n_out], leaf_phys[n_out].  The kernels do not trust them: a parent, a phys or a
// row outside its range reads zeros / writes nothing.
//
// A series of T frames over the same sites (ndmps_region_series_contract_*) runs the same plan with a frame dimension
// in every launch; see "series" below.
#include <algorithm>

#include "common.h"

namespace {

using ndmps::ceil_div;
using ndmps::round_up;

typedef float f32x16 __attribute__((ext_vector_type(16)));
using ndmps::f64x4;

constexpr int kTileRows = 32;

// One wavefront per (tile, 32-column block): the tile body of region_level_f32 and of region_series_level<float> (one
// body, so a frame of a series is contracted by the arithmetic of the single-object call: the same MFMA, the same k
// order, the same batches of loads).  prev == nullptr: level 0, the parent row is the root [1].
__device__ __forceinline__ void level_tile_f32(const float* __restrict__ prev, int64_t n_prev, int64_t chi_l,
                                               const float* __restrict__ core, int64_t d, int64_t chi_r,
                                               const int32_t* __restrict__ parent, int64_t n_nodes,
                                               const int32_t* __restrict__ tiles, float* __restrict__ next) {
  const int lane = threadIdx.x;
  const int32_t* t = tiles + 3 * (int64_t)blockIdx.x;
  const int64_t p = t[0], row0 = t[1], cnt = t[2];
  if (p < 0 || p >= d || row0 < 0 || cnt < 1 || cnt > kTileRows) return;
  const int64_t col0 = (int64_t)blockIdx.y * 32;
  const int i = lane & 31, h = lane >> 5;
  const int64_t node = row0 + i;
  int64_t par = -1;
  if (i < cnt && node < n_nodes) {
    par = parent[node];
    if (par >= n_prev) par = -1;
  }
  const int64_t col = col0 + i;
  const bool col_ok = col < chi_r;
  const float* arow = prev ? prev + (par < 0 ? 0 : par) * chi_l : nullptr;
  const float* bcol = core + p * chi_r + col;  // A_s[k, p, col] = core[(k d + p) chi_r + col]
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  // kU MFMA steps per batch: all their operand loads are issued before the first product (one memory latency per
  // batch, not one per step)
  constexpr int kU = 16;
  for (int64_t k0 = 0; k0 < chi_l; k0 += 2 * kU) {
    float a[kU], b[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int64_t k = k0 + 2 * u + h;
      a[u] = (par >= 0 && k < chi_l) ? (arow ? arow[k] : 1.f) : 0.f;
      b[u] = (col_ok && k < chi_l) ? bcol[k * d * chi_r] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
  }
  if (!col_ok) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = (r & 3) + 8 * (r >> 2) + 4 * h;
    if (row < cnt && row0 + row < n_nodes) next[(row0 + row) * chi_r + col] = acc[r];
  }
}

__global__ void __launch_bounds__(64)
region_level_f32(const float* __restrict__ prev, int64_t n_prev, int64_t chi_l, const float* __restrict__ core,
                 int64_t d, int64_t chi_r, const int32_t* __restrict__ parent, int64_t n_nodes,
                 const int32_t* __restrict__ tiles, float* __restrict__ next) {
  level_tile_f32(prev, n_prev, chi_l, core, d, chi_r, parent, n_nodes, tiles, next);
}

// fp64: the same 32 x 32 tile as 2 x 2 MFMA tiles of 16 x 16, k in steps of 4.
__device__ __forceinline__ void level_tile_f64(const double* __restrict__ prev, int64_t n_prev, int64_t chi_l,
                                               const double* __restrict__ core, int64_t d, int64_t chi_r,
                                               const int32_t* __restrict__ parent, int64_t n_nodes,
                                               const int32_t* __restrict__ tiles, double* __restrict__ next) {
  const int lane = threadIdx.x;
  const int32_t* t = tiles + 3 * (int64_t)blockIdx.x;
  const int64_t p = t[0], row0 = t[1], cnt = t[2];
  if (p < 0 || p >= d || row0 < 0 || cnt < 1 || cnt > kTileRows) return;
  const int64_t col0 = (int64_t)blockIdx.y * 32;
  const int i = lane & 15, q = lane >> 4;
  int64_t par[2];
  for (int m = 0; m < 2; ++m) {
    const int64_t node = row0 + 16 * m + i;
    par[m] = -1;
    if (16 * m + i < cnt && node < n_nodes) {
      par[m] = parent[node];
      if (par[m] >= n_prev) par[m] = -1;
    }
  }
  f64x4 acc[2][2];
  for (int m = 0; m < 2; ++m)
    for (int n = 0; n < 2; ++n)
      for (int r = 0; r < 4; ++r) acc[m][n][r] = 0.0;
  constexpr int kU = 8;  // MFMA k-steps per batch of loads, as in the fp32 kernel
  for (int64_t k0 = 0; k0 < chi_l; k0 += 4 * kU) {
    double a[kU][2], b[kU][2];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int64_t k = k0 + 4 * u + q;
#pragma unroll
      for (int m = 0; m < 2; ++m)
        a[u][m] = (par[m] >= 0 && k < chi_l) ? (prev ? prev[par[m] * chi_l + k] : 1.0) : 0.0;
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const int64_t col = col0 + 16 * n + i;
        b[u][n] = (col < chi_r && k < chi_l) ? core[(k * d + p) * chi_r + col] : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][m], b[u][n], acc[m][n], 0, 0, 0);
  }
  for (int n = 0; n < 2; ++n) {
    const int64_t col = col0 + 16 * n + i;
    if (col >= chi_r) continue;
    for (int m = 0; m < 2; ++m)
      for (int r = 0; r < 4; ++r) {
        const int64_t row = 16 * m + q + 4 * r;
        if (row < cnt && row0 + row < n_nodes) next[(row0 + row) * chi_r + col] = acc[m][n][r];
      }
  }
}

__global__ void __launch_bounds__(64)
region_level_f64(const double* __restrict__ prev, int64_t n_prev, int64_t chi_l, const double* __restrict__ core,
                 int64_t d, int64_t chi_r, const int32_t* __restrict__ parent, int64_t n_nodes,
                 const int32_t* __restrict__ tiles, double* __restrict__ next) {
  level_tile_f64(prev, n_prev, chi_l, core, d, chi_r, parent, n_nodes, tiles, next);
}

// Last site (chi_r = 1): out[e] = E[leaf_parent[e], :] . A_{L-1}[:, leaf_phys[e], 0].  The body of region_leaves and
// of region_series_leaves.
template <typename T>
__device__ __forceinline__ void leaves_body(const T* __restrict__ prev, int64_t n_prev, int64_t chi_l,
                                            const T* __restrict__ core, int64_t d,
                                            const int32_t* __restrict__ leaf_parent,
                                            const int32_t* __restrict__ leaf_phys, int64_t n_out, T* __restrict__ out) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n_out; e += (int64_t)gridDim.x * 256) {
    const int64_t par = leaf_parent[e], p = leaf_phys[e];
    T v = 0;
    if (p >= 0 && p < d && par >= 0 && par < n_prev) {
      if (prev) {
        const T* row = prev + par * chi_l;
        for (int64_t k = 0; k < chi_l; ++k) v += row[k] * core[k * d + p];
      } else {
        v = core[p];  // L == 1: the root times the only core (1, d, 1)
      }
    }
    out[e] = v;
  }
}

template <typename T>
__global__ void __launch_bounds__(256)
region_leaves(const T* __restrict__ prev, int64_t n_prev, int64_t chi_l, const T* __restrict__ core, int64_t d,
              const int32_t* __restrict__ leaf_parent, const int32_t* __restrict__ leaf_phys, int64_t n_out,
              T* __restrict__ out) {
  leaves_body<T>(prev, n_prev, chi_l, core, d, leaf_parent, leaf_phys, n_out, out);
}

// ------------------------------------------------------------------------------------------------ series
// T frames of one shape and one plan (NDMPS.decode_regions / values_at_many): the launches of the single-object call
// with a frame dimension.  The frame records are one device buffer, T * L core pointers then T * (L + 1) int64 bonds;
// frame t works in its own slab of the two ping-pong buffers, at t * frame_stride elements, its rows packed at its
// own chi_r.  The records are trusted no more than the tables: a frame with a bond below 1 or above the cap of its
// level (the largest host bond there, which sized the slab) or with a null core is skipped by every level and gets
// zeros from the leaf kernel, so nothing is read or written outside a slab or the frame's rows of the output.
constexpr int kSeriesMaxSites = 64;
constexpr int kSeriesMaxFrames = 65535;  // gridDim.z of the level kernels, gridDim.y of the leaf kernel

struct SeriesCaps {
  int64_t cap[kSeriesMaxSites + 1];
};

__device__ __forceinline__ bool series_frame_ok(const void* const* __restrict__ cores,
                                                const int64_t* __restrict__ bonds, int L, const SeriesCaps& caps) {
  bool ok = true;
  for (int s = 0; s <= L; ++s) ok = ok && bonds[s] >= 1 && bonds[s] <= caps.cap[s];
  for (int s = 0; s < L; ++s) ok = ok && cores[s] != nullptr;
  return ok;
}

// grid (tiles, ceil(cap_{lvl+1} / 32), T): one wavefront per (tile, 32-column block, frame); a wavefront whose
// column block lies beyond its frame's chi_r leaves at once
template <typename T>
__global__ void __launch_bounds__(64)
region_series_level(const T* __restrict__ prev, int64_t n_prev, int64_t d, int lvl, int L,
                    const void* const* __restrict__ rec_cores, const int64_t* __restrict__ rec_bonds,
                    const SeriesCaps caps, int64_t frame_stride, const int32_t* __restrict__ parent, int64_t n_nodes,
                    const int32_t* __restrict__ tiles, T* __restrict__ next) {
  const int64_t t = blockIdx.z;
  const void* const* cores = rec_cores + t * L;
  const int64_t* bonds = rec_bonds + t * (L + 1);
  if (!series_frame_ok(cores, bonds, L, caps)) return;
  const int64_t chi_l = bonds[lvl], chi_r = bonds[lvl + 1];
  if ((int64_t)blockIdx.y * 32 >= chi_r) return;
  const T* prev_t = prev ? prev + t * frame_stride : nullptr;
  if constexpr (sizeof(T) == 4)
    level_tile_f32(prev_t, n_prev, chi_l, (const float*)cores[lvl], d, chi_r, parent, n_nodes, tiles,
                   next + t * frame_stride);
  else
    level_tile_f64(prev_t, n_prev, chi_l, (const double*)cores[lvl], d, chi_r, parent, n_nodes, tiles,
                   next + t * frame_stride);
}

// grid (blocks, T): out[t * n_out + e]
template <typename T>
__global__ void __launch_bounds__(256)
region_series_leaves(const T* __restrict__ prev, int64_t n_prev, int64_t d, int L,
                     const void* const* __restrict__ rec_cores, const int64_t* __restrict__ rec_bonds,
                     const SeriesCaps caps, int64_t frame_stride, const int32_t* __restrict__ leaf_parent,
                     const int32_t* __restrict__ leaf_phys, int64_t n_out, T* __restrict__ out) {
  const int64_t t = blockIdx.y;
  const void* const* cores = rec_cores + t * L;
  const int64_t* bonds = rec_bonds + t * (L + 1);
  T* out_t = out + t * n_out;
  if (!series_frame_ok(cores, bonds, L, caps)) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n_out; e += (int64_t)gridDim.x * 256) out_t[e] = 0;
    return;
  }
  leaves_body<T>(prev ? prev + t * frame_stride : nullptr, n_prev, bonds[L - 1], (const T*)cores[L - 1], d,
                 leaf_parent, leaf_phys, n_out, out_t);
}

// workspace: two ping-pong buffers of the largest level
int64_t region_buffer_elems(int L, const int64_t* h_bonds, const int64_t* h_nodes) {
  int64_t m = 1;
  for (int s = 0; s + 1 < L; ++s) m = std::max(m, h_nodes[s] * h_bonds[s + 1]);
  return m;
}

// the level counts and the table length of a plan (both entry families)
int region_check_plan(int L, const int64_t* h_dims, const int64_t* h_nodes, const int64_t* h_tiles, int64_t table_len,
                      int64_t n_out) {
  NDMPS_REQUIRE(L == 1 || (h_nodes && h_tiles), "region: missing level counts");
  NDMPS_REQUIRE(n_out >= 1 && n_out < INT32_MAX, "region: output size %lld out of range", (long long)n_out);
  int64_t expect = 2 * n_out;
  for (int s = 0; s < L; ++s) {
    NDMPS_REQUIRE(h_dims[s] >= 1, "region: bad site %d", s);
    if (s + 1 < L) {
      NDMPS_REQUIRE(h_nodes[s] >= 1 && h_nodes[s] < INT32_MAX && h_tiles[s] >= 1 && h_tiles[s] <= h_nodes[s],
                    "region: bad level %d", s);
      expect += h_nodes[s] + 3 * h_tiles[s];
    }
  }
  NDMPS_REQUIRE(table_len == expect, "region: table length %lld, expected %lld", (long long)table_len,
                (long long)expect);
  return NDMPS_OK;
}

template <typename T>
int region_impl(int L, const int64_t* h_dims, const int64_t* h_bonds, const T* const* h_cores, const int64_t* h_nodes,
                const int64_t* h_tiles, const int32_t* d_tables, int64_t table_len, int64_t n_out, T* d_out,
                void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  NDMPS_REQUIRE(L >= 1 && h_dims && h_bonds && h_cores && d_tables && d_out, "region: bad arguments");
  NDMPS_REQUIRE(h_bonds[0] == 1 && h_bonds[L] == 1, "region: open chain expected (outer bonds 1)");
  for (int s = 0; s < L; ++s) NDMPS_REQUIRE(h_bonds[s + 1] >= 1 && h_cores[s], "region: bad site %d", s);
  NDMPS_TRY(region_check_plan(L, h_dims, h_nodes, h_tiles, table_len, n_out));
  const int64_t buf = round_up(region_buffer_elems(L, h_bonds, h_nodes) * (int64_t)sizeof(T), 256);
  if (L > 1 && (d_ws == nullptr || ws_bytes < 2 * buf)) {
    ndmps::set_error("region: workspace %lld bytes, need %lld", (long long)ws_bytes, (long long)(2 * buf));
    return NDMPS_EWORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  T* bufs[2] = {(T*)d_ws, (T*)((char*)d_ws + buf)};
  const T* prev = nullptr;
  int64_t n_prev = 1;
  const int32_t* tab = d_tables;
  for (int lvl = 0; lvl + 1 < L; ++lvl) {
    const int32_t* parent = tab;
    const int32_t* tiles = tab + h_nodes[lvl];
    tab = tiles + 3 * h_tiles[lvl];
    T* next = bufs[lvl & 1];
    dim3 grid((unsigned)h_tiles[lvl], (unsigned)ceil_div(h_bonds[lvl + 1], 32));
    NDMPS_REQUIRE(h_tiles[lvl] <= INT32_MAX && grid.y <= 65535, "region: level %d too large", lvl);
    if constexpr (sizeof(T) == 4)
      region_level_f32<<<grid, 64, 0, s>>>(prev, n_prev, h_bonds[lvl], h_cores[lvl], h_dims[lvl], h_bonds[lvl + 1],
                                           parent, h_nodes[lvl], tiles, next);
    else
      region_level_f64<<<grid, 64, 0, s>>>(prev, n_prev, h_bonds[lvl], h_cores[lvl], h_dims[lvl], h_bonds[lvl + 1],
                                           parent, h_nodes[lvl], tiles, next);
    NDMPS_LAUNCH_CHECK();
    prev = next;
    n_prev = h_nodes[lvl];
  }
  const int64_t blocks = std::min<int64_t>(ceil_div(n_out, 256), 16 * ndmps::kNumCU);
  region_leaves<T><<<(unsigned)blocks, 256, 0, s>>>(prev, n_prev, h_bonds[L - 1], h_cores[L - 1], h_dims[L - 1], tab,
                                                    tab + n_out, n_out, d_out);
  NDMPS_LAUNCH_CHECK();
  return NDMPS_OK;
}

// caps[s] = max_t bonds[t][s]; returns the slab of one frame in elements: max_s nodes_s * cap_{s+1} (at least 1)
int64_t series_frame_stride(int T, int L, const int64_t* h_bonds, const int64_t* h_nodes, SeriesCaps* caps) {
  for (int s = 0; s <= L; ++s) {
    caps->cap[s] = 1;
    for (int t = 0; t < T; ++t) caps->cap[s] = std::max(caps->cap[s], h_bonds[(int64_t)t * (L + 1) + s]);
  }
  int64_t m = 1;
  for (int s = 0; s + 1 < L; ++s) m = std::max(m, h_nodes[s] * caps->cap[s + 1]);
  return m;
}

template <typename T>
int region_series_impl(int n_frames, int L, const int64_t* h_dims, const int64_t* h_bonds, const int64_t* h_nodes,
                       const int64_t* h_tiles, const int32_t* d_tables, int64_t table_len, const void* d_records,
                       int64_t n_out, T* d_out, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  NDMPS_REQUIRE(L >= 1 && L <= kSeriesMaxSites && h_dims && h_bonds && d_tables && d_records && d_out,
                "region series: bad arguments");
  NDMPS_REQUIRE(n_frames >= 1 && n_frames <= kSeriesMaxFrames, "region series: %d frames outside [1, %d]", n_frames,
                kSeriesMaxFrames);
  for (int t = 0; t < n_frames; ++t) {
    const int64_t* b = h_bonds + (int64_t)t * (L + 1);
    NDMPS_REQUIRE(b[0] == 1 && b[L] == 1, "region series: frame %d: open chain expected (outer bonds 1)", t);
    for (int s = 1; s < L; ++s) NDMPS_REQUIRE(b[s] >= 1, "region series: frame %d: bad bond %d", t, s);
  }
  NDMPS_TRY(region_check_plan(L, h_dims, h_nodes, h_tiles, table_len, n_out));
  SeriesCaps caps;
  memset(&caps, 0, sizeof caps);
  const int64_t stride = series_frame_stride(n_frames, L, h_bonds, h_nodes, &caps);
  const int64_t buf = round_up(n_frames * stride * (int64_t)sizeof(T), 256);
  if (L > 1 && (d_ws == nullptr || ws_bytes < 2 * buf)) {
    ndmps::set_error("region series: workspace %lld bytes, need %lld", (long long)ws_bytes, (long long)(2 * buf));
    return NDMPS_EWORKSPACE;
  }
  for (int lvl = 0; lvl + 1 < L; ++lvl)
    NDMPS_REQUIRE(ceil_div(caps.cap[lvl + 1], 32) <= 65535, "region series: level %d too large", lvl);
  hipStream_t s = (hipStream_t)stream;
  const void* const* rec_cores = (const void* const*)d_records;
  const int64_t* rec_bonds = (const int64_t*)(rec_cores + (int64_t)n_frames * L);
  T* bufs[2] = {(T*)d_ws, (T*)((char*)d_ws + buf)};
  const T* prev = nullptr;
  int64_t n_prev = 1;
  const int32_t* tab = d_tables;
  for (int lvl = 0; lvl + 1 < L; ++lvl) {
    const int32_t* parent = tab;
    const int32_t* tiles = tab + h_nodes[lvl];
    tab = tiles + 3 * h_tiles[lvl];
    T* next = bufs[lvl & 1];
    dim3 grid((unsigned)h_tiles[lvl], (unsigned)ceil_div(caps.cap[lvl + 1], 32), (unsigned)n_frames);
    region_series_level<T><<<grid, 64, 0, s>>>(prev, n_prev, h_dims[lvl], lvl, L, rec_cores, rec_bonds, caps, stride,
                                               parent, h_nodes[lvl], tiles, next);
    NDMPS_LAUNCH_CHECK();
    prev = next;
    n_prev = h_nodes[lvl];
  }
  const int64_t blocks = std::min<int64_t>(ceil_div(n_out, 256), 16 * ndmps::kNumCU);
  region_series_leaves<T><<<dim3((unsigned)blocks, (unsigned)n_frames), 256, 0, s>>>(
      prev, n_prev, h_dims[L - 1], L, rec_cores, rec_bonds, caps, stride, tab, tab + n_out, n_out, d_out);
  NDMPS_LAUNCH_CHECK();
  return NDMPS_OK;
}

}  // namespace

extern "C" int64_t ndmps_region_workspace_bytes(int L, const int64_t* h_bonds, const int64_t* h_nodes,
                                                int64_t elem_bytes) {
  if (L <= 1) return 0;
  if (!h_bonds || !h_nodes || elem_bytes <= 0) return -1;
  return 2 * round_up(region_buffer_elems(L, h_bonds, h_nodes) * elem_bytes, 256);
}

extern "C" int ndmps_region_contract_f32(int L, const int64_t* h_dims, const int64_t* h_bonds,
                                         const float* const* h_cores, const int64_t* h_nodes, const int64_t* h_tiles,
                                         const int32_t* d_tables, int64_t table_len, int64_t n_out, float* d_out,
                                         void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  return region_impl<float>(L, h_dims, h_bonds, h_cores, h_nodes, h_tiles, d_tables, table_len, n_out, d_out, d_ws,
                            ws_bytes, stream);
}

extern "C" int ndmps_region_contract_f64(int L, const int64_t* h_dims, const int64_t* h_bonds,
                                         const double* const* h_cores, const int64_t* h_nodes, const int64_t* h_tiles,
                                         const int32_t* d_tables, int64_t table_len, int64_t n_out, double* d_out,
                                         void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  return region_impl<double>(L, h_dims, h_bonds, h_cores, h_nodes, h_tiles, d_tables, table_len, n_out, d_out, d_ws,
                             ws_bytes, stream);
}

extern "C" int64_t ndmps_region_series_workspace_bytes(int T, int L, const int64_t* h_bonds, const int64_t* h_nodes,
                                                       int64_t elem_bytes) {
  if (T < 1 || T > kSeriesMaxFrames || L < 1 || L > kSeriesMaxSites || elem_bytes <= 0) return -1;
  if (L == 1) return 0;
  if (!h_bonds || !h_nodes) return -1;
  SeriesCaps caps;
  return 2 * round_up(T * series_frame_stride(T, L, h_bonds, h_nodes, &caps) * elem_bytes, 256);
}

extern "C" int ndmps_region_series_contract_f32(int T, int L, const int64_t* h_dims, const int64_t* h_bonds,
                                                const int64_t* h_nodes, const int64_t* h_tiles,
                                                const int32_t* d_tables, int64_t table_len, const void* d_records,
                                                int64_t n_out, float* d_out, void* d_ws, int64_t ws_bytes,
                                                ndmps_stream_t stream) {
  return region_series_impl<float>(T, L, h_dims, h_bonds, h_nodes, h_tiles, d_tables, table_len, d_records, n_out,
                                   d_out, d_ws, ws_bytes, stream);
}

extern "C" int ndmps_region_series_contract_f64(int T, int L, const int64_t* h_dims, const int64_t* h_bonds,
                                                const int64_t* h_nodes, const int64_t* h_tiles,
                                                const int32_t* d_tables, int64_t table_len, const void* d_records,
                                                int64_t n_out, double* d_out, void* d_ws, int64_t ws_bytes,
                                                ndmps_stream_t stream) {
  return region_series_impl<double>(T, L, h_dims, h_bonds, h_nodes, h_tiles, d_tables, table_len, d_records, n_out,
                                    d_out, d_ws, ws_bytes, stream);
}
