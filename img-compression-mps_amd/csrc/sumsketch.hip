// Rounding of a weighted sum of many MPS by a randomised sketch (core/sumsketch.py, NDMPS.linear_combinations /
// pca_sketched).
//
// The formal sum chain of T frames is block-diagonal with the bonds m_k = sum_a chi_{a,k}.  It is never formed, and no
// eigenproblem has its order: random cores R_k (l_k, d_k, l_{k+1}), fp64, drawn on the host, sketch it down to a
// left-orthonormal fp64 chain of bonds r_k <= l_k <= 512 ("randomise then orthogonalise", Al Daas et al., SISC 2023,
// sum of TT tensors), which ndmps_lincomb_round then rounds at that small order.  Every step is a batch of small
// independent products over the frames:
//   1. right environments, once per call (they do not depend on the weights), k = L-1 .. 1, W_{a,L} = [1]:
//        W_{a,k} (chi_{a,k} x l_k) = sum_i A_{a,k}[:, i, :] ( W_{a,k+1} R_k[:, i, :]^T )                    form env
//   2. forward, per output row j, k = 0 .. L-2, M_{a,0} = [w_{j,a}], r_0 = 1:
//        S ((r_k d_k) x l_{k+1}) = sum_a (M_{a,k} A_{a,k}[:, i, :]) W_{a,k+1},  a ascending                   form sketch
//        twice: the Gram orthonormalisation pass of gram_pass.h;  site k = the result Q, rank r_{k+1}
//        M_{a,k+1} (r_{k+1} x chi_{a,k+1}) = sum_i Q[(., i), :]^T ( M_{a,k} A_{a,k}[:, i, :] )                form project
//      the last site is the sketch form at k = L-1 (W_{a,L} = [1]);  s_0 = 0 at some bond: that output is zero.
//
// All three forms are two-phase products on v_mfma_f64_16x16x4_f64 with a 64 x 64 fp64 half product in LDS, in the
// structure of pair_product.h: the XOR-swizzled 512-byte rows (pair_img), the operands of the cores loaded in their
// storage type one phase ahead (pair_load_operands).  Workgroups of four waves, 64 KiB of LDS, two per CU.
//   project  is the step of pair_product_step.inc itself: E = a 64-row tile of M_a, the core as B, Q as the last factor.
//   env      contracts over the sketch bond l_{k+1} <= 512 in k-tiles of 64 in phase 1 (W_{a,k+1} through LDS, R_k from
//            global memory), then multiplies by the core from the left.
//   sketch   has the core in the middle: phase 1 forms Z^T = A_i^T M^T (core as the A operand, M^T from LDS), phase 2
//            S += Z W (Z^T from LDS as the A operand, W from global memory), result in the accumulators over all
//            frames of the workgroup's share.  Where one workgroup per tile would leave the chip idle the frames are
//            split into `nsplit` contiguous shares (a function of the layout alone) and a second kernel adds the
//            partials in ascending order.  No atomics anywhere; the same arguments give the same bits.
// Bonds that are not multiples of 16 are zero-padded in registers and LDS; tiles past the bonds are skipped and never
// stored.  That is the resident route, for frames whose bonds are all <= 64.
// General route (a frame with some bond > 64): its cores widened to fp64 once per call, then per site ndmps_dgemm on
// the same buffers, X_a = M_a A_a as ((r d) x chi') in a scratch:
//   env      Yt ((l_k d) x chi') = R_k Wn^T;  W_a = A_a (chi x d chi') Yt^T
//   sketch   S += X_a Wn, added after the resident frames' sum, general frames ascending (a fixed order as well)
//   project  Mn_a = Q^T X_a
#include <math.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "gram_pass.h"
#include "pair_host.h"
#include "pair_product.h"

namespace {

using ndmps::Arena;
using ndmps::f64x4;
using ndmps::grid1d;
using ndmps::pair_img;

constexpr int kResident = ndmps::kPairResident;  // largest frame bond of the resident route
constexpr int kMaxBond = 4096;                   // largest frame bond
constexpr int kMaxSketch = 512;                  // largest sketch bond (order of the eigenproblems)
constexpr int kLd = ndmps::kPairLd;
constexpr int kMaxSplit = 16;                    // most shares of the frames in the sketch form
constexpr int64_t kMaxGrid = (int64_t)1 << 30;   // workgroups of one launch

// One frame at one site.
struct FrameRec {
  const void* core;  // A_{a,k} (chi, d, chi2) in storage type `code`
  const double* Wn;  // W_{a,k+1} (chi2 x l_{k+1})
  double* W;         // W_{a,k}   (chi x l_k)
  const double* M;   // M_{a,k}   (r_k x chi)
  double* Mn;        // M_{a,k+1} (r_{k+1} x chi2)
  int code, chi, chi2, pad[3];  // 64 bytes
};

struct StepArgs {
  const FrameRec* rec;  // the site's records, by frame
  const int* list;      // the frames to run, ascending
  const double* mat;    // env: R_k (l0, d, l1);  project: Q ((l0 d) x l1)
  double* out;          // sketch: S ((l0 d) x l1), or the partials (nsplit of them)
  int n, d, l0, l1;     // env: l0 = l_k, l1 = l_{k+1};  sketch: l0 = r_k, l1 = l_{k+1};  project: l0 = r_k, l1 = r_{k+1}
  int slot0, nsplit;    // first slot of `list` of this launch;  shares of the frames (sketch)
};

// q[ks] = src[(4 ks + lr) * stride + c_off], zero where 4 ks + lr >= klim or the lane is inactive
__device__ __forceinline__ void load_strided(double (&q)[16], const double* __restrict__ src, int stride, int c_off, int klim,
                                             int lr, bool active) {
  asm volatile("" : "+v"(lr));  // as in pair_load_et
  double raw[16];
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) raw[ks] = src[(active && 4 * ks + lr < klim) ? (4 * ks + lr) * stride + c_off : 0];
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) q[ks] = (active && 4 * ks + lr < klim) ? raw[ks] : 0.0;
}

// env: one workgroup per (frame, 64-column chunk of lam).  W_a[:, chunk] = sum_i A_i ( Wn R_k[chunk, i, :]^T ).
__global__ void __launch_bounds__(256, 2) sumsketch_env_kernel(StepArgs g) {
  __shared__ double Et[kLd * kLd];
  __shared__ double Z[kLd * kLd];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lc = lane & 15, lr = lane >> 4;
  const int col = wave * 16 + lc;
  const int chunks = (g.l0 + 63) >> 6;
  const int slot = g.slot0 + (int)(blockIdx.x / chunks), lam0 = 64 * (int)(blockIdx.x % chunks);
  if (slot >= g.n) return;
  const FrameRec f = g.rec[g.list[slot]];
  const int d = g.d, l1 = g.l1, chi = f.chi, chi2 = f.chi2;
  const int nl = min(64, g.l0 - lam0);
  const int tiles_b = (chi2 + 15) >> 4, tiles_l = (nl + 15) >> 4, tiles_a = (chi + 15) >> 4;
  const int ktiles = (l1 + 63) >> 6, steps2 = (chi2 + 3) >> 2;
  const bool own1 = wave < tiles_l, own2 = wave < tiles_a;

  f64x4 acc[4];  // rows 16 wave + lr + 4 r of W_a, columns lam0 + 16 nt + lc
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) acc[nt] = (f64x4){0.0, 0.0, 0.0, 0.0};
  double bq[16], aq[16];
  for (int i = 0; i < d; ++i) {
    ndmps::pair_load_operands<true>(aq, f.core, f.code, chi, d, chi2, i, lr, col, own2);
    // ---- phase 1: Z_i (chi2 x nl) = Wn R_k[chunk, i, :]^T, over l1 in k-tiles of 64
    f64x4 z[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) z[mt] = (f64x4){0.0, 0.0, 0.0, 0.0};
    for (int kt = 0; kt < ktiles; ++kt) {
      const int mu0 = 64 * kt, nm = min(64, l1 - mu0), steps1 = (nm + 3) >> 2;
      load_strided(bq, g.mat, 1, ((lam0 + col) * d + i) * l1 + mu0, nm, lr, own1 && col < nl);
      if (ktiles > 1 || i == 0) {  // one k-tile: Wn stays in Et for every i
        if (kt > 0) __syncthreads();
        ndmps::pair_load_et(Et, f.Wn + mu0, chi2, nm, l1, tid);
        __syncthreads();
      }
      if (own1) {
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
          if (ks < steps1) {
            const int k = 4 * ks + lr;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
              if (mt < tiles_b) z[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(Et[pair_img(k, 16 * mt + lc)], bq[ks], z[mt], 0, 0, 0);
          }
          if (ks & 1) __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) Z[pair_img(16 * mt + lr + 4 * r, col)] = z[mt][r];
    __syncthreads();
    // ---- phase 2: acc[16 wave .., :] += A_i[16 wave .., :] Z_i
    if (own2) {
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        if (ks < steps2) {
          const int k = 4 * ks + lr;
#pragma unroll
          for (int nt = 0; nt < 4; ++nt)
            if (nt < tiles_l) acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(aq[ks], Z[pair_img(k, 16 * nt + lc)], acc[nt], 0, 0, 0);
        }
        if (ks & 1) __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();  // Z and Et are rewritten by the next i
  }
  ndmps::pair_store_strip(f.W + lam0, g.l0, acc, chi, nl, wave, lr, lc);
}

// sketch: one workgroup per (share of the frames, i, 64-row tile of rho, 64-column chunk of lam).
//   blockIdx.x = ((i * rtiles + rt) * chunks + chunk),  blockIdx.y = share
__global__ void __launch_bounds__(256, 2) sumsketch_sketch_kernel(StepArgs g) {
  __shared__ double Mt[kLd * kLd];
  __shared__ double Z[kLd * kLd];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lc = lane & 15, lr = lane >> 4;
  const int col = wave * 16 + lc;
  const int d = g.d, l1 = g.l1;
  const int chunks = (l1 + 63) >> 6, rtiles = (g.l0 + 63) >> 6;
  const int lam0 = 64 * (int)(blockIdx.x % chunks), rho0 = 64 * (int)((blockIdx.x / chunks) % rtiles);
  const int i = (int)(blockIdx.x / (chunks * rtiles));
  const int share = blockIdx.y;
  const int s0 = (int)((int64_t)g.n * share / g.nsplit), s1 = (int)((int64_t)g.n * (share + 1) / g.nsplit);
  const int nl = min(64, l1 - lam0), nr = min(64, g.l0 - rho0);
  const int tiles_r = (nr + 15) >> 4, tiles_l = (nl + 15) >> 4;
  const bool own2 = wave < tiles_l;

  f64x4 acc[4];  // rows rho0 + 16 mt + lr + 4 r of S, columns lam0 + 16 wave + lc
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) acc[mt] = (f64x4){0.0, 0.0, 0.0, 0.0};
  double aq[16], bq[16];
  for (int s = s0; s < s1; ++s) {
    const FrameRec f = g.rec[g.list[s]];
    const int chi = f.chi, chi2 = f.chi2;
    const int tiles_b = (chi2 + 15) >> 4, steps1 = (chi + 3) >> 2, steps2 = (chi2 + 3) >> 2;
    const bool own1 = wave < tiles_b;
    ndmps::pair_load_et(Mt, f.M + (int64_t)rho0 * chi, nr, chi, chi, tid);
    ndmps::pair_load_operands<false>(aq, f.core, f.code, chi, d, chi2, i, lr, col, own1);
    load_strided(bq, f.Wn, l1, lam0 + col, chi2, lr, own2 && col < nl);
    __syncthreads();
    // ---- phase 1: Z^T[16 wave .., :] (chi2 x nr) = A_i^T[16 wave .., :] M^T
    f64x4 z[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) z[nt] = (f64x4){0.0, 0.0, 0.0, 0.0};
    if (own1) {
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        if (ks < steps1) {
          const int k = 4 * ks + lr;
#pragma unroll
          for (int nt = 0; nt < 4; ++nt)
            if (nt < tiles_r) z[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(aq[ks], Mt[pair_img(k, 16 * nt + lc)], z[nt], 0, 0, 0);
        }
        if (ks & 1) __builtin_amdgcn_sched_barrier(0);
      }
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) Z[pair_img(16 * wave + lr + 4 * r, 16 * nt + lc)] = z[nt][r];
    __syncthreads();
    // ---- phase 2: acc[:, 16 wave ..] += Z W_a[:, lam0 + 16 wave ..]
    if (own2) {
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        if (ks < steps2) {
          const int k = 4 * ks + lr;
#pragma unroll
          for (int mt = 0; mt < 4; ++mt)
            if (mt < tiles_r) acc[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(Z[pair_img(k, 16 * mt + lc)], bq[ks], acc[mt], 0, 0, 0);
        }
        if (ks & 1) __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();  // Mt and Z are rewritten by the next frame
  }
  double* out = g.out + (int64_t)share * g.l0 * d * l1;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * mt + lr + 4 * r;
      if (row < nr && col < nl) out[((int64_t)(rho0 + row) * d + i) * l1 + lam0 + col] = acc[mt][r];
    }
}

// S[e] = sum of the nsplit partials, ascending
__global__ void __launch_bounds__(256) sumsketch_reduce_kernel(const double* __restrict__ P, int nsplit, int64_t elems,
                                                               double* __restrict__ S) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < elems; e += (int64_t)gridDim.x * 256) {
    double v = P[e];
    for (int q = 1; q < nsplit; ++q) v += P[q * elems + e];
    S[e] = v;
  }
}

// S[e] += X[e]
__global__ void __launch_bounds__(256) sumsketch_add_kernel(double* __restrict__ S, const double* __restrict__ X, int64_t elems) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < elems; e += (int64_t)gridDim.x * 256) S[e] += X[e];
}

// project: one workgroup per (frame, 64-row chunk of rho').  Mn_a[chunk, :] = sum_{rho tiles} sum_i Q_i^T ( M_a A_i ).
__global__ void __launch_bounds__(256, 2) sumsketch_project_kernel(StepArgs g) {
  constexpr bool kTrans = false;
  __shared__ double Et[kLd * kLd];
  __shared__ double Z[kLd * kLd];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lc = lane & 15;
  int lr = lane >> 4, col = wave * 16 + lc;
  const int chunks = (g.l1 + 63) >> 6;
  const int slot = g.slot0 + (int)(blockIdx.x / chunks), rp0 = 64 * (int)(blockIdx.x % chunks);
  if (slot >= g.n) return;
  const FrameRec f = g.rec[g.list[slot]];
  const int d = g.d, r1 = g.l1, cb = f.chi, cb2 = f.chi2, code_b = f.code;
  const void* B = f.core;
  const int np = min(64, r1 - rp0);
  const int tiles_co = (cb2 + 15) >> 4, tiles_p = (np + 15) >> 4;
  const int steps1 = (cb + 3) >> 2;
  const bool own1 = wave < tiles_co, own2 = wave < tiles_p;
  const int i1 = d;

  f64x4 acc[4];  // rows rp0 + 16 wave + lr + 4 r of Mn_a, columns 16 nt + lc
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) acc[nt] = (f64x4){0.0, 0.0, 0.0, 0.0};
  double bq[16], aq[16];
  // one loop over (rho tile, i): a new tile of M_a enters Et, with the core's operands of i = 0, where i wraps
  const int rtiles = (g.l0 + 63) >> 6;
  int rho0 = 0, i = 0;
  for (int t = 0; t < rtiles * d; ++t) {
    asm volatile("" : "+v"(lr), "+v"(col));  // the operand addresses are formed per step: hoisted out of the loop they spill
    const int nr = min(64, g.l0 - rho0);
    const int tiles_re = (nr + 15) >> 4, steps2 = (nr + 3) >> 2;
    if (i == 0) {
      ndmps::pair_load_et(Et, f.M + (int64_t)rho0 * cb, nr, cb, cb, tid);
      ndmps::pair_load_operands<kTrans>(bq, B, code_b, cb, d, cb2, 0, lr, col, own1);
    }
    load_strided(aq, g.mat, d * r1, (rho0 * d + i) * r1 + rp0 + col, nr, lr, own2 && col < np);
    __syncthreads();
#include "pair_product_step.inc"
    if (++i == d) i = 0, rho0 += 64;
  }
  ndmps::pair_store_strip(f.Mn + (int64_t)rp0 * cb2, cb2, acc, np, cb2, wave, lr, lc);
}

// shares of the frames in the sketch form: a function of the layout alone (capacities, not ranks)
int sketch_split(int64_t T, int64_t d, int64_t l0_cap, int64_t l1) {
  const int64_t tiles = d * ndmps::ceil_div(l0_cap, 64) * ndmps::ceil_div(l1, 64);
  const int64_t want = std::max<int64_t>(1, 512 / tiles), most = std::max<int64_t>(1, std::min<int64_t>(kMaxSplit, T / 4));
  return (int)std::min(want, most);
}

int launch_env(StepArgs g, hipStream_t s) {
  const int64_t chunks = ndmps::ceil_div(g.l0, 64), per = std::max<int64_t>(1, kMaxGrid / chunks);
  for (int64_t f0 = 0; f0 < g.n; f0 += per) {
    g.slot0 = (int)f0;
    hipLaunchKernelGGL(sumsketch_env_kernel, dim3((unsigned)(std::min<int64_t>(per, g.n - f0) * chunks)), dim3(256), 0, s, g);
    NDMPS_LAUNCH_CHECK();
  }
  return NDMPS_OK;
}

int launch_project(StepArgs g, hipStream_t s) {
  const int64_t chunks = ndmps::ceil_div(g.l1, 64), per = std::max<int64_t>(1, kMaxGrid / chunks);
  for (int64_t f0 = 0; f0 < g.n; f0 += per) {
    g.slot0 = (int)f0;
    hipLaunchKernelGGL(sumsketch_project_kernel, dim3((unsigned)(std::min<int64_t>(per, g.n - f0) * chunks)), dim3(256), 0, s, g);
    NDMPS_LAUNCH_CHECK();
  }
  return NDMPS_OK;
}

// S ((l0 d) x l1) = the sketch form over the g.n frames of g.list; P: room for nsplit partials when nsplit > 1
int launch_sketch(StepArgs g, double* S, double* P, hipStream_t s) {
  const int64_t tiles = (int64_t)g.d * ndmps::ceil_div(g.l0, 64) * ndmps::ceil_div(g.l1, 64);
  NDMPS_REQUIRE(tiles <= kMaxGrid, "internal: sketch grid");
  g.nsplit = std::max(1, std::min(g.nsplit, g.n));
  g.out = g.nsplit > 1 ? P : S;
  hipLaunchKernelGGL(sumsketch_sketch_kernel, dim3((unsigned)tiles, (unsigned)g.nsplit), dim3(256), 0, s, g);
  NDMPS_LAUNCH_CHECK();
  if (g.nsplit > 1) {
    const int64_t elems = (int64_t)g.l0 * g.d * g.l1;
    hipLaunchKernelGGL(sumsketch_reduce_kernel, dim3(grid1d(elems)), dim3(256), 0, s, P, g.nsplit, elems, S);
    NDMPS_LAUNCH_CHECK();
  }
  return NDMPS_OK;
}

// ---- general route of one frame at one site; A64: its core (chi, d, chi2) in fp64; GX: scratch of l0 d chi2 doubles
int general_env(const FrameRec& f, const double* A64, const double* R, int64_t d, int64_t l0, int64_t l1, double* GX, hipStream_t s) {
  NDMPS_TRY(ndmps_dgemm(0, 1, l0 * d, f.chi2, l1, R, l1, f.Wn, l1, GX, f.chi2, s));
  return ndmps_dgemm(0, 1, f.chi, l0, d * f.chi2, A64, d * f.chi2, GX, d * f.chi2, f.W, l0, s);
}
// X_a = M_a A_a ((r d) x chi2) into GX
int general_x(const FrameRec& f, const double* A64, int64_t d, int64_t r, double* GX, hipStream_t s) {
  return ndmps_dgemm(0, 0, r, d * f.chi2, f.chi, f.M, f.chi, A64, d * f.chi2, GX, d * f.chi2, s);
}
// S ((r d) x l1) (+)= X_a Wn;  Sg: scratch of r d l1 doubles, used when adding
int general_sketch(const FrameRec& f, const double* A64, int64_t d, int64_t r, int64_t l1, bool add, double* S, double* Sg,
                   double* GX, hipStream_t s) {
  NDMPS_TRY(general_x(f, A64, d, r, GX, s));
  NDMPS_TRY(ndmps_dgemm(0, 0, r * d, l1, f.chi2, GX, f.chi2, f.Wn, l1, add ? Sg : S, l1, s));
  if (add) {
    hipLaunchKernelGGL(sumsketch_add_kernel, dim3(grid1d(r * d * l1)), dim3(256), 0, s, S, Sg, r * d * l1);
    NDMPS_LAUNCH_CHECK();
  }
  return NDMPS_OK;
}
int general_project(const FrameRec& f, const double* A64, const double* Q, int64_t d, int64_t r, int64_t r1, double* GX,
                    hipStream_t s) {
  NDMPS_TRY(general_x(f, A64, d, r, GX, s));
  return ndmps_dgemm(1, 0, r1, f.chi2, r * d, Q, r1, GX, f.chi2, f.Mn, f.chi2, s);
}

// Host plan of a call: the checked arguments, the output layout and the workspace carve.
struct Plan : ndmps::SketchLayout {
  int T = 0, K = 0, L = 0;
  std::vector<int64_t> bonds, m, w_off;
  std::vector<int64_t> pref;  // pref[a (L + 1) + k] = sum_{b < a} chi_{b,k}
  std::vector<char> wide;          // the frame has a bond above 64: the general route
  std::vector<int64_t> wide_off;   // its site k core in the fp64 copies, at wide_off[a L + k]
  int64_t w_elems = 0, mm = 1, part = 1, wide_elems = 0, gx = 0;
  int64_t chi(int a, int k) const { return bonds[(int64_t)a * (L + 1) + k]; }
};

int make_plan(int T, int K, int L, const int64_t* h_dims, const int64_t* h_bonds, const int64_t* h_ell, Plan& p) {
  NDMPS_REQUIRE(T >= 1 && K >= 1 && L >= 1 && h_dims && h_bonds && h_ell, "bad sumsketch argument (T = %d, K = %d, L = %d)", T, K, L);
  NDMPS_REQUIRE(T <= (1 << 20) && K <= (1 << 20), "too many frames or outputs (T = %d, K = %d)", T, K);
  p.T = T, p.K = K, p.L = L;
  p.dims.assign(h_dims, h_dims + L);
  p.ell.assign(h_ell, h_ell + L + 1);
  p.bonds.assign(h_bonds, h_bonds + (int64_t)T * (L + 1));
  for (int k = 0; k < L; ++k)
    NDMPS_REQUIRE(p.dims[k] >= 1 && p.dims[k] <= (1 << 20), "site %d: bad physical dim %lld", k, (long long)p.dims[k]);
  NDMPS_REQUIRE(p.ell[0] == 1 && p.ell[L] == 1, "the outer sketch bonds must be 1");
  p.m.assign(L + 1, 0);
  p.pref.assign((int64_t)T * (L + 1), 0);
  p.wide.assign(T, 0);
  p.wide_off.assign((int64_t)T * L, 0);
  for (int a = 0; a < T; ++a) {
    NDMPS_REQUIRE(p.chi(a, 0) == 1 && p.chi(a, L) == 1, "frame %d: the outer bonds must be 1", a);
    for (int k = 0; k <= L; ++k) {
      NDMPS_REQUIRE(p.chi(a, k) >= 1 && p.chi(a, k) <= kMaxBond, "frame %d, bond %d: bond %lld outside [1, %d]", a, k,
                    (long long)p.chi(a, k), kMaxBond);
      p.pref[(int64_t)a * (L + 1) + k] = p.m[k];
      p.m[k] += p.chi(a, k);
      if (p.chi(a, k) > kResident) p.wide[a] = 1;
    }
  }
  for (int k = 0; k <= L; ++k)
    NDMPS_REQUIRE(p.ell[k] >= 1 && p.ell[k] <= kMaxSketch, "bond %d: sketch bond %lld outside [1, %d]", k, (long long)p.ell[k],
                  kMaxSketch);
  p.w_off.assign(L + 1, 0);
  for (int k = 0; k < L; ++k) {
    NDMPS_REQUIRE(p.dims[k] * ndmps::ceil_div(p.ell[k], 64) * ndmps::ceil_div(p.ell[k + 1], 64) <= kMaxGrid, "site %d: too large", k);
    p.part = std::max(p.part, sketch_split(T, p.dims[k], p.ell[k], p.ell[k + 1]) * p.ell[k] * p.dims[k] * p.ell[k + 1]);
    p.mm = std::max(p.mm, p.ell[k] * p.m[k]);
    if (k >= 1) {
      p.w_off[k] = p.w_elems;
      p.w_elems += p.ell[k] * p.m[k];
    }
  }
  for (int a = 0; a < T; ++a)
    for (int k = 0; k < L && p.wide[a]; ++k) {
      p.wide_off[(int64_t)a * L + k] = p.wide_elems;
      p.wide_elems += p.chi(a, k) * p.dims[k] * p.chi(a, k + 1);
      p.gx = std::max(p.gx, p.ell[k] * p.dims[k] * p.chi(a, k + 1));
    }
  return ndmps::fill_sketch_layout(p);
}

struct Buffers {
  double *R = nullptr, *one = nullptr, *W = nullptr, *M[2] = {nullptr, nullptr}, *S = nullptr, *Q = nullptr, *P = nullptr;
  ndmps::GramPassWs gw;
  FrameRec* rec = nullptr;
  int* list = nullptr;  // T frames of the environment pass, then T of the forward pass
  double *wcores = nullptr, *GX = nullptr;  // general route: the wide frames' cores in fp64 and the scratch
};

// Workspace, every piece 256-byte aligned, in this order (doubles unless said otherwise), m_k = sum_a chi_{a,k}:
//   R              sum_k l_k d_k l_{k+1}
//   one            1                                   W_{a,L} = [1] of every frame
//   W              sum_{k = 1 .. L-1} l_k m_k          W_{a,k} at l_k sum_{b<a} chi_{b,k} inside bond k's piece
//   M (two)        max_{k < L} l_k m_k each            M_{a,k} of even and odd k
//   S, Q           max_k l_k d_k l_{k+1} each
//   P              max_k nsplit_k l_k d_k l_{k+1}      the partials of the sketch form
//   G, V           lmax^2 each;  w  lmax;  the eigen-solver's workspace for order lmax (bytes)
//   records        T L of 64 bytes;  lists  2 T ints
//   when some frame has a bond above 64: those frames' cores in fp64, and max over them and k of l_k d_k chi_{a,k+1}
void carve(const Plan& p, Arena& ar, Buffers& b) {
  b.R = ar.take<double>(p.r_elems);
  b.one = ar.take<double>(1);
  b.W = ar.take<double>(std::max<int64_t>(p.w_elems, 1));
  b.M[0] = ar.take<double>(p.mm);
  b.M[1] = ar.take<double>(p.mm);
  b.S = ar.take<double>(p.sq);
  b.Q = ar.take<double>(p.sq);
  b.P = ar.take<double>(p.part);
  b.gw = ndmps::carve_gram_pass(ar, p.lmax, p.eig);
  b.rec = ar.take<FrameRec>((int64_t)p.T * p.L);
  b.list = ar.take<int>(2 * (int64_t)p.T);
  if (p.wide_elems > 0) {
    b.wcores = ar.take<double>(p.wide_elems);
    b.GX = ar.take<double>(p.gx);
  }
}

static_assert(sizeof(FrameRec) == 64, "the workspace formula of the header counts 64 bytes per record");

}  // namespace

extern "C" int64_t ndmps_sumsketch_layout(int T, int K, int L, const int64_t* h_dims, const int64_t* h_bonds,
                                          const int64_t* h_ell, int64_t* h_out_off, int64_t* h_ws_bytes) {
  Plan p;
  NDMPS_TRY(make_plan(T, K, L, h_dims, h_bonds, h_ell, p));
  if (h_out_off)
    for (int k = 0; k <= L; ++k) h_out_off[k] = p.out_off[k];
  if (h_ws_bytes) {
    Arena ar(nullptr, 0);
    Buffers b;
    carve(p, ar, b);
    *h_ws_bytes = ar.query_bytes();
  }
  return (int64_t)K * p.out_off[L];
}

extern "C" int ndmps_sumsketch_step(int form, int T, int64_t d, const int64_t* h_chi, const int64_t* h_chi2,
                                    const int* h_codes, const void* const* h_cores, int64_t l0, int64_t l1,
                                    const double* d_in, const double* d_in2, const double* d_mat, double* d_out, void* d_ws,
                                    int64_t ws_bytes, ndmps_stream_t stream) {
  NDMPS_REQUIRE(form >= 0 && form <= 2, "sumsketch form must be 0 (env), 1 (sketch) or 2 (project), got %d", form);
  NDMPS_REQUIRE(T >= 1 && T <= (1 << 20) && h_chi && h_chi2 && h_codes && h_cores && d_in && d_out, "bad sumsketch step argument");
  NDMPS_REQUIRE(form == 1 ? d_in2 != nullptr : d_mat != nullptr, "NULL sumsketch step argument");
  NDMPS_REQUIRE(d >= 1 && d <= (1 << 20) && l0 >= 1 && l0 <= kMaxSketch && l1 >= 1 && l1 <= kMaxSketch,
                "bad sumsketch step extents (d = %lld, l0 = %lld, l1 = %lld)", (long long)d, (long long)l0, (long long)l1);
  for (int a = 0; a < T; ++a) {
    NDMPS_REQUIRE(h_chi[a] >= 1 && h_chi[a] <= kMaxBond && h_chi2[a] >= 1 && h_chi2[a] <= kMaxBond,
                  "frame %d: bonds (%lld, %lld) outside [1, %d]", a, (long long)h_chi[a], (long long)h_chi2[a], kMaxBond);
    NDMPS_REQUIRE(h_codes[a] >= 0 && h_codes[a] <= 2, "frame %d: bad dtype code %d", a, h_codes[a]);
    NDMPS_REQUIRE(h_cores[a], "frame %d: NULL core", a);
  }
  const int nsplit = form == 1 ? sketch_split(T, d, l0, l1) : 1;
  Arena ar(d_ws, ws_bytes);
  FrameRec* rec = ar.take<FrameRec>(T);
  int* list = ar.take<int>(T);
  double* P = ar.take<double>(nsplit > 1 ? nsplit * l0 * d * l1 : 1);
  // general route: the wide frames' cores in fp64, the scratch X / Yt and (sketch) the product that is added
  std::vector<double*> w64(T, nullptr);
  int64_t gx = 0;
  for (int a = 0; a < T; ++a)
    if (std::max(h_chi[a], h_chi2[a]) > kResident) {
      w64[a] = ar.take<double>(h_chi[a] * d * h_chi2[a]);
      gx = std::max(gx, l0 * d * h_chi2[a]);
    }
  double* GX = gx ? ar.take<double>(gx) : nullptr;
  double* Sg = gx && form == 1 ? ar.take<double>(l0 * d * l1) : nullptr;
  NDMPS_REQUIRE(ar.fits(), "sumsketch step workspace too small: %lld < %lld", (long long)ws_bytes, (long long)ar.used);
  hipStream_t s = (hipStream_t)stream;
  std::vector<FrameRec> h(T);
  std::vector<int> hl;
  int64_t in_off = 0, in2_off = 0, out_off = 0;
  for (int a = 0; a < T; ++a) {
    FrameRec& f = h[a];
    f = FrameRec{};
    f.core = h_cores[a], f.code = h_codes[a], f.chi = (int)h_chi[a], f.chi2 = (int)h_chi2[a];
    if (!gx || std::max(h_chi[a], h_chi2[a]) <= kResident) hl.push_back(a);
    if (form == 0) {  // in: Wn (chi2 x l1);  out: W (chi x l0)
      f.Wn = d_in + in_off, f.W = d_out + out_off;
      in_off += h_chi2[a] * l1, out_off += h_chi[a] * l0;
    } else if (form == 1) {  // in: M (l0 x chi), in2: Wn (chi2 x l1)
      f.M = d_in + in_off, f.Wn = d_in2 + in2_off;
      in_off += l0 * h_chi[a], in2_off += h_chi2[a] * l1;
    } else {  // in: M (l0 x chi);  out: Mn (l1 x chi2)
      f.M = d_in + in_off, f.Mn = d_out + out_off;
      in_off += l0 * h_chi[a], out_off += l1 * h_chi2[a];
    }
  }
  NDMPS_CHECK_HIP(hipMemcpyAsync(rec, h.data(), T * sizeof(FrameRec), hipMemcpyHostToDevice, s));
  if (!hl.empty()) NDMPS_CHECK_HIP(hipMemcpyAsync(list, hl.data(), hl.size() * sizeof(int), hipMemcpyHostToDevice, s));
  StepArgs g;
  g.rec = rec, g.list = list, g.mat = d_mat, g.out = d_out;
  g.n = (int)hl.size(), g.d = (int)d, g.l0 = (int)l0, g.l1 = (int)l1, g.slot0 = 0, g.nsplit = nsplit;
  if (!hl.empty()) {
    int rc = form == 0 ? launch_env(g, s) : form == 1 ? launch_sketch(g, d_out, P, s) : launch_project(g, s);
    NDMPS_TRY(rc);
  }
  bool add = !hl.empty();
  for (int a = 0; a < T; ++a) {
    if (!w64[a]) continue;
    const double* A64;
    NDMPS_TRY(ndmps::core64(h_cores[a], h_codes[a], h_chi[a] * d * h_chi2[a], w64[a], s, &A64));
    if (form == 0) NDMPS_TRY(general_env(h[a], A64, d_mat, d, l0, l1, GX, s));
    if (form == 1) NDMPS_TRY(general_sketch(h[a], A64, d, l0, l1, add, d_out, Sg, GX, s));
    if (form == 2) NDMPS_TRY(general_project(h[a], A64, d_mat, d, l0, l1, GX, s));
    add = true;
  }
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));  // the host tables are read
  return NDMPS_OK;
}

extern "C" int ndmps_sumsketch_sketch(int T, int K, int L, const int64_t* h_dims, const int64_t* h_bonds, const int* h_codes,
                                      const void* const* h_cores, const double* h_weights, const int64_t* h_ell,
                                      const double* h_R, int64_t r_len, double* d_out, int64_t out_elems, int64_t* h_ranks,
                                      int* h_zero, void* d_ws, int64_t ws_bytes, ndmps_stream_t stream) {
  NDMPS_REQUIRE(h_codes && h_cores && h_weights && h_R && d_out && h_ranks && h_zero, "NULL sumsketch argument");
  Plan p;
  NDMPS_TRY(make_plan(T, K, L, h_dims, h_bonds, h_ell, p));
  for (int a = 0; a < T; ++a) {
    NDMPS_REQUIRE(h_codes[a] >= 0 && h_codes[a] <= 2, "frame %d: bad dtype code %d", a, h_codes[a]);
    for (int k = 0; k < L; ++k) NDMPS_REQUIRE(h_cores[(int64_t)a * L + k], "frame %d, site %d: NULL core", a, k);
  }
  for (int64_t e = 0; e < (int64_t)K * T; ++e) NDMPS_REQUIRE(std::isfinite(h_weights[e]), "non-finite weight");
  NDMPS_TRY(ndmps::check_sketch_cores(p, r_len));
  const int64_t chain = p.out_off[L];
  NDMPS_REQUIRE(out_elems >= K * chain, "output arena too small: %lld < %lld", (long long)out_elems, (long long)(K * chain));
  Arena ar(d_ws, ws_bytes);
  Buffers b;
  carve(p, ar, b);
  NDMPS_REQUIRE(ar.fits(), "sumsketch workspace too small: %lld < %lld", (long long)ws_bytes, (long long)ar.used);
  hipStream_t s = (hipStream_t)stream;

  // the records of every frame and site, and the frames of the environment pass (some weight is not zero)
  std::vector<FrameRec> h((int64_t)T * L);
  std::vector<int> env_list, env_wide, fwd_list(T), fwd_wide;
  for (int a = 0; a < T; ++a) {
    bool used = false;
    for (int j = 0; j < K; ++j) used = used || h_weights[(int64_t)j * T + a] != 0.0;
    if (used) (p.wide[a] ? env_wide : env_list).push_back(a);
    for (int k = 0; k < L; ++k) {
      FrameRec& f = h[(int64_t)k * T + a];
      f = FrameRec{};
      f.core = h_cores[(int64_t)a * L + k], f.code = h_codes[a], f.chi = (int)p.chi(a, k), f.chi2 = (int)p.chi(a, k + 1);
      const int64_t pk = p.pref[(int64_t)a * (L + 1) + k], pk1 = p.pref[(int64_t)a * (L + 1) + k + 1];
      f.W = k >= 1 ? b.W + p.w_off[k] + p.ell[k] * pk : nullptr;
      f.Wn = k + 1 < L ? b.W + p.w_off[k + 1] + p.ell[k + 1] * pk1 : b.one;
      f.M = b.M[k & 1] + p.ell[k] * pk;
      f.Mn = b.M[(k + 1) & 1] + p.ell[k + 1] * pk1;
    }
  }
  for (int j = 0; j < K; ++j) {
    h_zero[j] = 0;
    for (int k = 0; k <= L; ++k) h_ranks[(int64_t)j * (L + 1) + k] = 1;
  }
  const double one = 1.0;
  NDMPS_CHECK_HIP(hipMemcpyAsync(b.R, h_R, r_len * sizeof(double), hipMemcpyHostToDevice, s));
  NDMPS_CHECK_HIP(hipMemcpyAsync(b.one, &one, sizeof(double), hipMemcpyHostToDevice, s));
  NDMPS_CHECK_HIP(hipMemcpyAsync(b.rec, h.data(), h.size() * sizeof(FrameRec), hipMemcpyHostToDevice, s));
  if (!env_list.empty())
    NDMPS_CHECK_HIP(hipMemcpyAsync(b.list, env_list.data(), env_list.size() * sizeof(int), hipMemcpyHostToDevice, s));

  // general route: the fp64 cores of the wide frames that are used
  std::vector<const double*> A64((size_t)T * L, nullptr);
  for (int a : env_wide)
    for (int k = 0; k < L; ++k) {
      const int64_t e = (int64_t)a * L + k;
      NDMPS_TRY(ndmps::core64(h_cores[e], h_codes[a], p.chi(a, k) * p.dims[k] * p.chi(a, k + 1), b.wcores + p.wide_off[e], s, &A64[e]));
    }

  StepArgs g;
  g.list = b.list, g.slot0 = 0, g.nsplit = 1, g.out = nullptr;
  // ---- 1. right environments
  for (int k = L - 1; k >= 1; --k) {
    g.rec = b.rec + (int64_t)k * T, g.mat = b.R + p.out_off[k];
    g.n = (int)env_list.size(), g.d = (int)p.dims[k], g.l0 = (int)p.ell[k], g.l1 = (int)p.ell[k + 1];
    if (g.n > 0) NDMPS_TRY(launch_env(g, s));
    for (int a : env_wide)
      NDMPS_TRY(general_env(h[(int64_t)k * T + a], A64[(int64_t)a * L + k], g.mat, p.dims[k], p.ell[k], p.ell[k + 1], b.GX, s));
  }

  // ---- 2. forward pass, one output row at a time
  std::vector<double> hw(p.lmax), m0(T);
  g.list = b.list + T;
  for (int j = 0; j < K; ++j) {
    const double* w = h_weights + (int64_t)j * T;
    int n = 0;
    fwd_wide.clear();
    for (int a = 0; a < T; ++a) {
      m0[a] = w[a];
      if (w[a] == 0.0) continue;
      if (p.wide[a]) fwd_wide.push_back(a);
      else fwd_list[n++] = a;
    }
    if (n == 0 && fwd_wide.empty()) {
      h_zero[j] = 1;
      continue;
    }
    if (n > 0) NDMPS_CHECK_HIP(hipMemcpyAsync(b.list + T, fwd_list.data(), n * sizeof(int), hipMemcpyHostToDevice, s));
    NDMPS_CHECK_HIP(hipMemcpyAsync(b.M[0], m0.data(), T * sizeof(double), hipMemcpyHostToDevice, s));
    NDMPS_CHECK_HIP(hipStreamSynchronize(s));  // the host tables are read
    int64_t* ranks = h_ranks + (int64_t)j * (L + 1);
    double* out = d_out + j * chain;
    int64_t r = 1;
    bool zero = false;
    for (int k = 0; k < L && !zero; ++k) {
      g.rec = b.rec + (int64_t)k * T;
      g.n = n, g.d = (int)p.dims[k], g.l0 = (int)r, g.l1 = (int)p.ell[k + 1];
      g.nsplit = sketch_split(T, p.dims[k], p.ell[k], p.ell[k + 1]);
      g.mat = nullptr;
      // S: the resident frames in one launch, then the wide frames one by one (b.Q is free here: the added product)
      double* S = k == L - 1 ? out + p.out_off[k] : b.S;
      if (n > 0) NDMPS_TRY(launch_sketch(g, S, b.P, s));
      bool add = n > 0;
      for (int a : fwd_wide) {
        NDMPS_TRY(general_sketch(h[(int64_t)k * T + a], A64[(int64_t)a * L + k], p.dims[k], r, p.ell[k + 1], add, S, b.Q, b.GX, s));
        add = true;
      }
      if (k == L - 1) break;
      const int64_t rows = r * p.dims[k];
      int64_t r1 = 0, r2 = 0;
      NDMPS_TRY(ndmps::gram_pass(b.gw, b.S, rows, p.ell[k + 1], b.Q, &r1, hw, s));
      if (r1 > 0) NDMPS_TRY(ndmps::gram_pass(b.gw, b.Q, rows, r1, out + p.out_off[k], &r2, hw, s));
      if (r2 == 0) {
        zero = true;
        break;
      }
      ranks[k + 1] = r2;
      g.mat = out + p.out_off[k];
      g.l1 = (int)r2;
      if (n > 0) NDMPS_TRY(launch_project(g, s));
      for (int a : fwd_wide) NDMPS_TRY(general_project(h[(int64_t)k * T + a], A64[(int64_t)a * L + k], g.mat, p.dims[k], r, r2, b.GX, s));
      r = r2;
    }
    if (zero) {
      h_zero[j] = 1;
      for (int k = 0; k <= L; ++k) ranks[k] = 1;
    }
  }
  NDMPS_CHECK_HIP(hipStreamSynchronize(s));
  return NDMPS_OK;
}
