// Axis operators on the cores (core/axisop.py, NDMPS.roll / shift / correlate1d / cumsum): a matrix-product operator
// that acts on one axis's digit per site, applied to a chain in one launch.
//
// Site k of the input is X (chi, d, chi'), d = pre f post, its physical index (p f + digit) post + q; the operator's
// core is M (D, f, f, D') indexed [c, o, i, c'].  The site of the wide chain is
//     Z[c chi + a, (p f + o) post + q, c' chi' + a'] = sum_i M[c, o, i, c'] X[a, (p f + i) post + q, a']
// with the bonds D chi and D' chi', carry-major.  X is read in its storage type (0 fp32, 1 bf16, 2 fp64), the sum is
// taken in fp64 over the entries of M that are not exactly 0 (a single-term operator copies its input values bit for
// bit) and Z is written in the work type: fp64 for fp64 input, fp32 otherwise.
// One launch for all sites: blockIdx.y is the site (a task table uploaded once together with the operator's cores),
// blockIdx.x a tile of 1024 consecutive elements of Z, so lanes walk a' and both the reads of X and the writes of Z are
// contiguous along it.  M is a few hundred doubles and is staged in LDS; a core too large for it (a large prime
// radix) is read from the table directly.
#include <vector>

#include "common.h"

namespace {

using ndmps::ceil_div;
using ndmps::load_any;

constexpr int kThreads = 256, kPerThread = 4, kTileElems = kThreads * kPerThread;
constexpr int64_t kLdsDoubles = 4096;  // 32 KiB of LDS for one site's M

struct SiteTask {
  const void* X;
  void* Z;
  int64_t chi, chi2, pre, f, post, D, D2;
  int64_t m_off;  // the site's M in the table, D f f D2 doubles
  int64_t total;  // elements of Z: D chi pre f post D2 chi2
};

// TZ: the work type.  A task or tile outside its range does nothing.
template <typename TZ>
__global__ void __launch_bounds__(kThreads)
axisop_kernel(const SiteTask* __restrict__ tasks, int ntasks, const double* __restrict__ mpo, int code) {
  if ((int)blockIdx.y >= ntasks) return;
  const SiteTask t = tasks[blockIdx.y];
  if (t.total <= 0 || !t.X || !t.Z) return;
  const int64_t e0 = (int64_t)blockIdx.x * kTileElems;
  if (e0 >= t.total) return;

  __shared__ double Ms[kLdsDoubles];
  const int64_t msize = t.D * t.f * t.f * t.D2;
  const bool staged = msize <= kLdsDoubles;  // uniform over the block
  if (staged) {
    for (int64_t j = threadIdx.x; j < msize; j += kThreads) Ms[j] = mpo[t.m_off + j];
    __syncthreads();
  }
  const double* Mg = mpo + t.m_off;
  const int64_t ncol = t.D2 * t.chi2, d = t.pre * t.f * t.post;
  TZ* Z = (TZ*)t.Z;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const int64_t e = e0 + (int64_t)j * kThreads + threadIdx.x;
    if (e >= t.total) break;
    const int64_t row = e / ncol, col = e - row * ncol;
    const int64_t c2 = col / t.chi2, a2 = col - c2 * t.chi2;
    int64_t r = row;
    const int64_t q = r % t.post;
    r /= t.post;
    const int64_t o = r % t.f;
    r /= t.f;
    const int64_t p = r % t.pre;
    r /= t.pre;
    const int64_t a = r % t.chi, c = r / t.chi;  // c < D since row < D chi d
    const int64_t mrow = ((c * t.f + o) * t.f) * t.D2 + c2;  // + i D2
    const int64_t xbase = (a * d + p * t.f * t.post + q) * t.chi2 + a2;  // + i post chi2
    double acc = 0.0;
    for (int64_t i = 0; i < t.f; ++i) {
      const double m = staged ? Ms[mrow + i * t.D2] : Mg[mrow + i * t.D2];
      if (m != 0.0) acc = fma(m, load_any(t.X, code, xbase + i * t.post * t.chi2), acc);
    }
    Z[e] = ndmps::from_f64<TZ>(acc);
  }
}

struct Plan {
  int L = 0;
  std::vector<int64_t> wide, out_off, m_off;  // wide[j] = D_j chi_j; site j of Z starts at out_off[j]; M_j at m_off[j]
  int64_t m_total = 0, max_total = 1;
};

int make_plan(int L, const int64_t* h_dims, const int64_t* h_bonds, const int64_t* h_factors, const int64_t* h_mpo_bonds,
              Plan& p) {
  NDMPS_REQUIRE(L >= 1 && L <= 65535 && h_dims && h_bonds && h_factors && h_mpo_bonds, "bad axisop argument (L = %d)", L);
  NDMPS_REQUIRE(h_bonds[0] == 1 && h_bonds[L] == 1 && h_mpo_bonds[0] == 1 && h_mpo_bonds[L] == 1,
                "the outer bonds of the chain and of the operator must be 1");
  const int64_t limit = ndmps_syevd_topk_max_n();
  p.L = L;
  p.wide.assign(L + 1, 1);
  for (int j = 0; j <= L; ++j) {
    NDMPS_REQUIRE(h_bonds[j] >= 1 && h_bonds[j] <= limit && h_mpo_bonds[j] >= 1 && h_mpo_bonds[j] <= limit,
                  "bond %d: bad bond %lld or operator bond %lld", j, (long long)h_bonds[j], (long long)h_mpo_bonds[j]);
    p.wide[j] = h_bonds[j] * h_mpo_bonds[j];
    NDMPS_REQUIRE(p.wide[j] <= limit, "bond %d: the widened bond %lld exceeds %lld; recompress the input first", j,
                  (long long)p.wide[j], (long long)limit);
  }
  p.out_off.assign(L + 1, 0);
  p.m_off.assign(L + 1, 0);
  for (int j = 0; j < L; ++j) {
    NDMPS_REQUIRE(h_dims[j] >= 1 && h_dims[j] <= INT32_MAX && h_factors[j] >= 1 && h_dims[j] % h_factors[j] == 0,
                  "site %d: bad physical dim %lld or digit radix %lld", j, (long long)h_dims[j], (long long)h_factors[j]);
    const int64_t total = p.wide[j] * h_dims[j] * p.wide[j + 1];  // < 2^24 * 2^31
    p.out_off[j + 1] = p.out_off[j] + total;
    p.m_off[j + 1] = p.m_off[j] + h_mpo_bonds[j] * h_factors[j] * h_factors[j] * h_mpo_bonds[j + 1];
    p.max_total = std::max(p.max_total, total);
  }
  p.m_total = p.m_off[L];
  return NDMPS_OK;
}

int64_t ws_bytes_of(const Plan& p) {
  ndmps::Arena ar(nullptr, 0);
  ar.take<SiteTask>(p.L);
  ar.take<double>(p.m_total);
  return ar.query_bytes();
}

}  // namespace

extern "C" int64_t ndmps_axisop_layout(int L, const int64_t* h_dims, const int64_t* h_bonds, const int64_t* h_factors,
                                       const int64_t* h_mpo_bonds, int64_t* h_out_off, int64_t* h_ws_bytes) {
  Plan p;
  NDMPS_TRY(make_plan(L, h_dims, h_bonds, h_factors, h_mpo_bonds, p));
  if (h_out_off)
    for (int j = 0; j <= L; ++j) h_out_off[j] = p.out_off[j];
  if (h_ws_bytes) *h_ws_bytes = ws_bytes_of(p);
  return p.out_off[L];
}

extern "C" int ndmps_axisop_apply(int L, const int64_t* h_dims, const int64_t* h_bonds, int code,
                                  const void* const* h_cores, const int64_t* h_factors, const int64_t* h_strides,
                                  const int64_t* h_mpo_bonds, const double* h_mpo, int64_t mpo_len, void* d_out,
                                  int64_t out_elems, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  Plan p;
  NDMPS_TRY(make_plan(L, h_dims, h_bonds, h_factors, h_mpo_bonds, p));
  NDMPS_REQUIRE(code >= 0 && code <= 2, "bad dtype code %d", code);
  NDMPS_REQUIRE(h_cores && h_strides && h_mpo && mpo_len == p.m_total, "bad operator table: %lld entries, %lld expected",
                (long long)mpo_len, (long long)p.m_total);
  NDMPS_REQUIRE(d_out && out_elems >= p.out_off[L], "output arena too small: %lld < %lld", (long long)out_elems,
                (long long)p.out_off[L]);
  ndmps::Arena ar(d_ws, ws_bytes);
  SiteTask* d_tasks = ar.take<SiteTask>(L);
  double* d_mpo = ar.take<double>(p.m_total);
  if (!ar.fits()) {
    ndmps::set_error("axisop workspace too small: %lld < %lld", (long long)ws_bytes, (long long)ar.used);
    return NDMPS_EWORKSPACE;
  }
  const int64_t esize = code == 2 ? 8 : 4;
  std::vector<SiteTask> tasks(L);
  for (int j = 0; j < L; ++j) {
    const int64_t f = h_factors[j], post = h_strides[j];
    NDMPS_REQUIRE(h_cores[j], "site %d: NULL core", j);
    NDMPS_REQUIRE(post >= 1 && h_dims[j] % (f * post) == 0, "site %d: digit stride %lld does not divide the site (d = %lld, f = %lld)",
                  j, (long long)post, (long long)h_dims[j], (long long)f);
    SiteTask& t = tasks[j];
    t.X = h_cores[j];
    t.Z = (char*)d_out + p.out_off[j] * esize;
    t.chi = h_bonds[j];
    t.chi2 = h_bonds[j + 1];
    t.pre = h_dims[j] / (f * post);
    t.f = f;
    t.post = post;
    t.D = h_mpo_bonds[j];
    t.D2 = h_mpo_bonds[j + 1];
    t.m_off = p.m_off[j];
    t.total = p.out_off[j + 1] - p.out_off[j];
  }
  const int64_t tiles = ceil_div(p.max_total, kTileElems);
  NDMPS_REQUIRE(tiles <= INT32_MAX, "axisop launch too large");
  hipStream_t s = (hipStream_t)stream;
  NDMPS_CHECK_HIP(hipMemcpyAsync(d_tasks, tasks.data(), L * sizeof(SiteTask), hipMemcpyHostToDevice, s));
  NDMPS_CHECK_HIP(hipMemcpyAsync(d_mpo, h_mpo, p.m_total * sizeof(double), hipMemcpyHostToDevice, s));
  if (code == 2)
    hipLaunchKernelGGL(axisop_kernel<double>, dim3((unsigned)tiles, (unsigned)L), dim3(kThreads), 0, s, d_tasks, L, d_mpo, code);
  else
    hipLaunchKernelGGL(axisop_kernel<float>, dim3((unsigned)tiles, (unsigned)L), dim3(kThreads), 0, s, d_tasks, L, d_mpo, code);
  NDMPS_LAUNCH_CHECK();
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));  // the host tables go out of scope
  return NDMPS_OK;
}
