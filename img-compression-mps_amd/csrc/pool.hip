// Block-averaged decode: the cores of the coarse volume (block means or sums of the voxels) straight from the cores
// of the volume.  No reference counterpart (there: to_tensor() at core/ndmps.py:131-153, then a reshape and a mean).
//
// Site l of the chain carries digit l of every axis, so reducing the volume over blocks is a site-local linear map on
// the cores (host planner: core/pool.py):
//     out_l[x, q, y] = w_l * sum_r A_l[x, qoff_l[q] + roff_l[r], y]
// The sites from L_keep on reduce over every axis (d'_l = 1): they collapse to matrices that are applied right to left
// to a vector, and the last kept site absorbs that vector into its right bond, (chi, d', chi_r) -> (chi, d', 1).
//
//   pool_sites_kernel     every reduced kept site (before the absorbing one) in ONE launch per 32 sites: a thread per
//                         output element, consecutive threads along y, so reads and writes are rows of chi_r.
//   pool_contract_kernel  one launch per collapsed site and one for the absorbing site: a workgroup per output row
//                         (x, q) sums w A_l[x, p(q, r), y] v[y] over (r, y), again along y; the collapsed site of an
//                         exact sweep (512 x 8 x 4096 at 256^3) is spread over its 512 rows, never one workgroup.
//
// Sums run in fp64 from fp32, bf16 or fp64 cores; outputs are fp32 (fp64 for fp64 cores), the carried vector fp64.
// The offset tables (int32, uploaded by the caller) are not trusted: an index outside the core reads nothing.
#include <algorithm>
#include <math.h>

#include "common.h"

namespace {

using ndmps::ceil_div;
using ndmps::round_up;

constexpr int kSitesPerLaunch = 32;
constexpr int kBlock = 256;

struct SiteDesc {
  const void* in;
  void* out;
  const int32_t* qoff;
  const int32_t* roff;
  int64_t chi_l, d_in, chi_r, dq, n_red;
  double w;
  int64_t blk0;  // first workgroup of this site
};
struct SiteChunk {
  SiteDesc s[kSitesPerLaunch];
  int64_t blk_end;  // workgroups of the whole launch
};

template <typename Tin, typename Tout>
__global__ void __launch_bounds__(kBlock) pool_sites_kernel(SiteChunk c, int n_sites) {
  int i = 0;
  while (i + 1 < n_sites && (int64_t)blockIdx.x >= c.s[i + 1].blk0) ++i;
  const SiteDesc& d = c.s[i];
  const int64_t blk_next = i + 1 < n_sites ? c.s[i + 1].blk0 : c.blk_end;
  const int64_t n_blk = blk_next - d.blk0;
  const int64_t total = d.chi_l * d.dq * d.chi_r;
  const Tin* __restrict__ in = static_cast<const Tin*>(d.in);
  Tout* __restrict__ out = static_cast<Tout*>(d.out);
  for (int64_t e = ((int64_t)blockIdx.x - d.blk0) * kBlock + threadIdx.x; e < total; e += n_blk * kBlock) {
    const int64_t y = e % d.chi_r, xq = e / d.chi_r;
    const int64_t q = xq % d.dq, x = xq / d.dq;
    const int64_t base = d.qoff[q];
    double acc = 0.0;
    for (int64_t r = 0; r < d.n_red; ++r) {
      const int64_t p = base + d.roff[r];
      if (p >= 0 && p < d.d_in) acc += ndmps::to_f64(in[(x * d.d_in + p) * d.chi_r + y]);
    }
    out[e] = ndmps::from_f64<Tout>(d.w * acc);
  }
}

// out[x dq + q] = w sum_{r, y} A[x, qoff[q] + roff[r], y] v[y]  (v == nullptr: chi_r == 1, v = [1])
template <typename Tin, typename Tout>
__global__ void __launch_bounds__(kBlock)
pool_contract_kernel(const Tin* __restrict__ in, int64_t chi_l, int64_t d_in, int chi_r, const int32_t* __restrict__ qoff,
                     int64_t dq, const int32_t* __restrict__ roff, int n_red, double w, const double* __restrict__ v,
                     Tout* __restrict__ out) {
  __shared__ double part[kBlock / 64];
  const int n = n_red * chi_r;
  const int64_t rows = chi_l * dq;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t x = row / dq, q = row % dq;
    const int64_t base = qoff[q];
    double acc = 0.0;
    for (int e = threadIdx.x; e < n; e += kBlock) {
      const int r = e / chi_r, y = e - r * chi_r;
      const int64_t p = base + roff[r];
      if (p >= 0 && p < d_in) acc += ndmps::to_f64(in[(x * d_in + p) * chi_r + y]) * (v ? v[y] : 1.0);
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
      for (int k = 0; k < kBlock / 64; ++k) t += part[k];
      out[row] = ndmps::from_f64<Tout>(w * t);
    }
    __syncthreads();
  }
}

// W[j, k] = w sum_{m = jB}^{jB + B - 1} B_dct[m][k]: the orthonormal DCT-II basis (dct_basis_kernel) summed over the
// rows of output block j, so that x pooled = y W^T
template <typename T>
__global__ void __launch_bounds__(kBlock) pool_dct_basis_kernel(T* __restrict__ W, int64_t n, int64_t block, double w) {
  const int64_t total = (n / block) * n;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
    const int64_t j = e / n, k = e % n;
    const double sk = (k == 0) ? sqrt(1.0 / (double)n) : sqrt(2.0 / (double)n);
    double acc = 0.0;
    for (int64_t m = j * block; m < (j + 1) * block; ++m) {
      const int64_t num = ((2 * m + 1) * k) % (4 * n);
      acc += cospi((double)num / (double)(2 * n));
    }
    W[e] = (T)(w * sk * acc);
  }
}

inline unsigned grid_for(int64_t work) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(work, kBlock), 2048)); }

template <typename Tin, typename Tout>
int pool_impl(int L, const int64_t* h_dims, const int64_t* h_bonds, const void* const* h_cores, int L_keep,
              const int64_t* h_sites, const double* h_weight, const int32_t* d_offs, int64_t offs_len,
              void* const* h_out, void* d_ws, int64_t ws_bytes, hipStream_t s) {
  NDMPS_REQUIRE(L >= 1 && L <= 64 && h_dims && h_bonds && h_cores && h_sites && h_weight && d_offs && h_out,
                "pool: bad arguments");
  NDMPS_REQUIRE(L_keep >= 0 && L_keep <= L, "pool: L_keep = %d outside [0, %d]", L_keep, L);
  NDMPS_REQUIRE(h_bonds[0] == 1 && h_bonds[L] == 1, "pool: open chain expected (outer bonds 1)");
  int64_t max_bond = 1;
  for (int l = 0; l < L; ++l) {
    const int64_t dq = h_sites[4 * l], nr = h_sites[4 * l + 1], q0 = h_sites[4 * l + 2], r0 = h_sites[4 * l + 3];
    NDMPS_REQUIRE(h_cores[l] && h_dims[l] >= 1 && h_bonds[l + 1] >= 1, "pool: bad site %d", l);
    NDMPS_REQUIRE(dq >= 1 && nr >= 1 && dq * nr <= h_dims[l], "pool: site %d keeps %lld x %lld of %lld", l,
                  (long long)dq, (long long)nr, (long long)h_dims[l]);
    NDMPS_REQUIRE(q0 >= 0 && r0 >= 0 && q0 + dq <= offs_len && r0 + nr <= offs_len, "pool: site %d tables out of range", l);
    NDMPS_REQUIRE(l < L_keep || dq == 1, "pool: collapsed site %d keeps %lld indices", l, (long long)dq);
    NDMPS_REQUIRE(nr * h_bonds[l + 1] < INT32_MAX, "pool: site %d too wide", l);
    max_bond = std::max(max_bond, h_bonds[l + 1]);
  }
  const bool collapse = L_keep < L;
  const int absorb = collapse ? L_keep - 1 : -1;  // site that absorbs the vector (-1: none, or the scalar)
  const int n_partial = collapse ? std::max(L_keep - 1, 0) : L;
  if (collapse) NDMPS_REQUIRE(h_out[std::max(absorb, 0)], "pool: no output for the absorbing site");
  const int64_t vec = round_up(max_bond * (int64_t)sizeof(double), 256);
  if (collapse && (d_ws == nullptr || ws_bytes < 2 * vec)) {
    ndmps::set_error("pool: workspace %lld bytes, need %lld", (long long)ws_bytes, (long long)(2 * vec));
    return NDMPS_EWORKSPACE;
  }
  // ---- kept sites before the absorbing one: one launch per 32 reduced sites (NULL output: passed through)
  SiteChunk chunk;
  int n = 0;
  int64_t blk = 0;
  auto flush = [&]() -> int {
    if (n == 0) return NDMPS_OK;
    chunk.blk_end = blk;
    NDMPS_REQUIRE(blk <= INT32_MAX, "pool: grid too large");
    hipLaunchKernelGGL((pool_sites_kernel<Tin, Tout>), dim3((unsigned)blk), dim3(kBlock), 0, s, chunk, n);
    NDMPS_LAUNCH_CHECK();
    n = 0;
    blk = 0;
    return NDMPS_OK;
  };
  for (int l = 0; l < n_partial; ++l) {
    if (!h_out[l]) continue;
    SiteDesc& d = chunk.s[n++];
    d.in = h_cores[l];
    d.out = h_out[l];
    d.qoff = d_offs + h_sites[4 * l + 2];
    d.roff = d_offs + h_sites[4 * l + 3];
    d.chi_l = h_bonds[l];
    d.d_in = h_dims[l];
    d.chi_r = h_bonds[l + 1];
    d.dq = h_sites[4 * l];
    d.n_red = h_sites[4 * l + 1];
    d.w = h_weight[l];
    d.blk0 = blk;
    blk += grid_for(d.chi_l * d.dq * d.chi_r);
    if (n == kSitesPerLaunch) NDMPS_TRY(flush());
  }
  NDMPS_TRY(flush());
  if (!collapse) return NDMPS_OK;
  // ---- suffix, right to left: v_l = M_l v_{l+1}; the absorbing site (or, for L_keep == 0, site 0) writes Tout
  double* bufs[2] = {(double*)d_ws, (double*)((char*)d_ws + vec)};
  const double* v = nullptr;
  int t = 0;
  for (int l = L - 1; l >= std::max(absorb, 0); --l) {
    const int64_t dq = h_sites[4 * l], rows = h_bonds[l] * dq;
    const int32_t* qoff = d_offs + h_sites[4 * l + 2];
    const int32_t* roff = d_offs + h_sites[4 * l + 3];
    const unsigned grid = (unsigned)std::min<int64_t>(rows, 65535);
    const Tin* in = static_cast<const Tin*>(h_cores[l]);
    const int chi_r = (int)h_bonds[l + 1], nr = (int)h_sites[4 * l + 1];
    if (l == std::max(absorb, 0)) {
      hipLaunchKernelGGL((pool_contract_kernel<Tin, Tout>), dim3(grid), dim3(kBlock), 0, s, in, h_bonds[l], h_dims[l],
                         chi_r, qoff, dq, roff, nr, h_weight[l], v, static_cast<Tout*>(h_out[std::max(absorb, 0)]));
    } else {
      hipLaunchKernelGGL((pool_contract_kernel<Tin, double>), dim3(grid), dim3(kBlock), 0, s, in, h_bonds[l],
                         h_dims[l], chi_r, qoff, dq, roff, nr, h_weight[l], v, bufs[t]);
      v = bufs[t];
      t ^= 1;
    }
    NDMPS_LAUNCH_CHECK();
  }
  return NDMPS_OK;
}

}  // namespace

extern "C" int64_t ndmps_pool_workspace_bytes(int L, const int64_t* h_bonds) {
  if (L < 1 || !h_bonds) return -1;
  int64_t m = 1;
  for (int l = 0; l <= L; ++l) m = std::max(m, h_bonds[l]);
  return 2 * round_up(m * (int64_t)sizeof(double), 256);
}

extern "C" int ndmps_pool_cores(int dtype, int L, const int64_t* h_dims, const int64_t* h_bonds,
                                const void* const* h_cores, int L_keep, const int64_t* h_sites, const double* h_weight,
                                const int32_t* d_offs, int64_t offs_len, void* const* h_out, void* d_ws, int64_t ws_bytes,
                                ndmps_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case 0:
      return pool_impl<float, float>(L, h_dims, h_bonds, h_cores, L_keep, h_sites, h_weight, d_offs, offs_len, h_out,
                                     d_ws, ws_bytes, s);
    case 1:
      return pool_impl<__bf16, float>(L, h_dims, h_bonds, h_cores, L_keep, h_sites, h_weight, d_offs, offs_len, h_out,
                                      d_ws, ws_bytes, s);
    case 2:
      return pool_impl<double, double>(L, h_dims, h_bonds, h_cores, L_keep, h_sites, h_weight, d_offs, offs_len, h_out,
                                       d_ws, ws_bytes, s);
    default:
      break;
  }
  ndmps::set_error("pool: storage type %d is not fp32 (0), bf16 (1) or fp64 (2)", dtype);
  return NDMPS_EINVAL;
}

extern "C" int ndmps_pool_dct_basis_f32(float* d_W, int64_t n, int64_t block, double weight, ndmps_stream_t stream) {
  NDMPS_REQUIRE(d_W && n >= 1 && n <= 16384 && block >= 1 && n % block == 0, "pool: bad pooled DCT basis %lld / %lld",
                (long long)n, (long long)block);
  hipLaunchKernelGGL(pool_dct_basis_kernel<float>, dim3(grid_for(n / block * n)), dim3(kBlock), 0, (hipStream_t)stream,
                     d_W, n, block, weight);
  NDMPS_LAUNCH_CHECK();
  return NDMPS_OK;
}

extern "C" int ndmps_pool_dct_basis_f64(double* d_W, int64_t n, int64_t block, double weight, ndmps_stream_t stream) {
  NDMPS_REQUIRE(d_W && n >= 1 && n <= 16384 && block >= 1 && n % block == 0, "pool: bad pooled DCT basis %lld / %lld",
                (long long)n, (long long)block);
  hipLaunchKernelGGL(pool_dct_basis_kernel<double>, dim3(grid_for(n / block * n)), dim3(kBlock), 0, (hipStream_t)stream,
                     d_W, n, block, weight);
  NDMPS_LAUNCH_CHECK();
  return NDMPS_OK;
}
