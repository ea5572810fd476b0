// Orthonormalisation of MORE than 128 eigenvectors (included by eig_tridiag.hip inside its anonymous namespace): the
// exact sweeps and compress() want every eigenpair above a cutoff -- up to all 4096 of an order-4096 Gram matrix
// (core/ndmps.py:74,104-106 of the reference: dgesdd through quimb).  Eigenvectors of T come from inverse iteration in
// column blocks of 128 (trd_invit_kernel, blockIdx.x = block), without any orthogonalisation in between; whatever is
// close in T's spectrum -- the whole noise floor of a volume's Gram matrix is, in absolute terms -- then needs it.
// As for up to 128 vectors: two Cholesky-QR passes over the whole n x k block, here across the chip:
//     S = Z^T Z                  ndmps_gram_f64 (fp64 MFMA, upper tiles x row slabs)
//     S = L L^T                  right-looking by blocks of 64: the diagonal block and its inverse by one workgroup in
//                                LDS (chol_inv_blocked), the panel below it and the trailing update on the MFMA
//     Z <- Z L^-T                block forward substitution, 16 rows of Z per workgroup: rows are independent, so the
//                                whole triangular solve is ONE launch (every workgroup streams L from L2)
// 2 n k^2 (Gram, symmetric half) + k^3 / 3 + n k^2 flops per pass.

constexpr int kWB = 64;    // Cholesky block
constexpr int kWLd = 65;   // LDS stride of chol_inv_blocked's operands
constexpr int kWOp = 68;   // LDS stride of the MFMA operands of the panel / trailing kernels

// diagonal block at p: S[p .., p ..] (lower) -> L in place, L^-1 into Linv[p .., p ..] (ld ldi); kk columns are real
__global__ void __launch_bounds__(512) wide_chol_diag_kernel(double* __restrict__ S, int ld, double* __restrict__ Linv, int ldi,
                                                             int k, int p, TrdDesc* __restrict__ d) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* Ls = lds;
  double* Li = lds + kWB * kWLd;
  const int tid = threadIdx.x;
  const int kk = min(kWB, k - p);
  for (int e = tid; e < kWB * kWB; e += 512) {
    const int i = e / kWB, j = e % kWB;
    Ls[i * kWLd + j] = (i < kk && j <= i) ? S[(int64_t)(p + i) * ld + p + j] : 0.0;
  }
  __syncthreads();
  const bool ok = chol_inv_blocked(Ls, Li, kWB, kk, kWLd, tid);
  __syncthreads();
  for (int e = tid; e < kWB * kWB; e += 512) {
    const int i = e / kWB, j = e % kWB;
    if (i < kk && j <= i) S[(int64_t)(p + i) * ld + p + j] = Ls[i * kWLd + j];
    Linv[(int64_t)(p + i) * ldi + p + j] = Li[i * kWLd + j];
  }
  if (!ok && tid == 0 && d->status != 2) d->status = 1;
}

// panel below the diagonal block at p: rows r >= p + 64: S[r][p .. p + 64) <- S[r][p ..) Linv_pp^T
__global__ void __launch_bounds__(256) wide_chol_panel_kernel(double* __restrict__ S, int ld, const double* __restrict__ Linv,
                                                              int ldi, int k, int p) {
  __shared__ __attribute__((aligned(16))) double X[kWB * kWOp], Y[kWB * kWOp];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = p + kWB * (1 + (int)blockIdx.x);
  for (int e = tid; e < kWB * kWB; e += 256) {
    const int i = e / kWB, j = e % kWB;
    X[i * kWOp + j] = (r0 + i < k && p + j < k) ? S[(int64_t)(r0 + i) * ld + p + j] : 0.0;
    Y[i * kWOp + j] = Linv[(int64_t)(p + i) * ldi + p + j];
  }
  __syncthreads();
#pragma unroll
  for (int cs = 0; cs < 4; ++cs) {
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k0 = 0; k0 < kWB; k0 += 16) acc = tile_nt(acc, X, 16 * wave, Y, 16 * cs, k0, kWOp, lane, 1.0);
    const int li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gr = r0 + 16 * wave + lk + 4 * r, gc = p + 16 * cs + li;
      if (gr < k && gc < k) S[(int64_t)gr * ld + gc] = acc[r];
    }
  }
}

// trailing update behind the panel at p: S[R][C] -= L[R][p ..] L[C][p ..]^T on the lower tiles of the blocks beyond p
__global__ void __launch_bounds__(256) wide_chol_trail_kernel(double* __restrict__ S, int ld, int k, int p) {
  __shared__ __attribute__((aligned(16))) double X[kWB * kWOp], Y[kWB * kWOp];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int R, C;
  pnl_tile(blockIdx.x, R, C);
  const int r0 = p + kWB * (1 + R), c0 = p + kWB * (1 + C);
  if (r0 >= k) return;
  for (int e = tid; e < kWB * kWB; e += 256) {
    const int i = e / kWB, j = e % kWB;
    X[i * kWOp + j] = (r0 + i < k && p + j < k) ? S[(int64_t)(r0 + i) * ld + p + j] : 0.0;
    Y[i * kWOp + j] = (c0 + i < k && p + j < k) ? S[(int64_t)(c0 + i) * ld + p + j] : 0.0;
  }
  __syncthreads();
  const int li = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int cs = 0; cs < 4; ++cs) {
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k0 = 0; k0 < kWB; k0 += 16) acc = tile_nt(acc, X, 16 * wave, Y, 16 * cs, k0, kWOp, lane, 1.0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gr = r0 + 16 * wave + lk + 4 * r, gc = c0 + 16 * cs + li;
      if (gr < k && gc < k && gc <= gr) S[(int64_t)gr * ld + gc] -= acc[r];
    }
  }
}

// Z <- Z L^-T, 16 rows of Z per workgroup (rows are independent): for block column p,
//     Z_p <- (Z_p - sum_{q < p} Z_q L[p][q]^T) Linv_pp^T
// with the finished blocks Z_q read back from global memory (the workgroup's own stores, behind a barrier) and L, Linv
// streamed from L2.  Sixteen waves: wave (w, h) takes the 16 columns 16 w .. of the block and the blocks q = h, h + 4,
// ... of the sum (four waves alone wait out every load: 7.4 ms per pass at order 4096), the four shares meet in LDS.
constexpr int kTrsmWaves = 16;
__global__ void __launch_bounds__(64 * kTrsmWaves) wide_trsm_kernel(double* __restrict__ Z, int kp, int n, int k,
                                                                  const double* __restrict__ L, int ld,
                                                                  const double* __restrict__ Linv, int ldi) {
  constexpr int NT = 64 * kTrsmWaves, NS = kTrsmWaves / 4;
  __shared__ __attribute__((aligned(16))) double Tp[NS][16 * kWOp];  // the shares of the block's 16 x 64 right-hand side
  __shared__ __attribute__((aligned(16))) double T[16 * kWOp];
  __shared__ __attribute__((aligned(16))) double Y[kWB * kWOp];      // Linv_pp
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wc = wave & 3, wh = wave >> 2;
  const int li = lane & 15, lk = lane >> 4;
  const int i0 = 16 * (int)blockIdx.x;
  const bool row_ok = i0 + li < n;
  const double* zrow = Z + (int64_t)min(i0 + li, n - 1) * kp;
  const int nblk = (k + kWB - 1) / kWB;
  for (int pb = 0; pb < nblk; ++pb) {
    const int p = kWB * pb, cw = p + 16 * wc;  // first column of this wave's tile
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    if (wh == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + lk + 4 * r, c = cw + li;
        acc[r] = (i < n && c < k) ? Z[(int64_t)i * kp + c] : 0.0;
      }
    }
    const double* lrow = L + (int64_t)min(cw + li, k - 1) * ld;
    const bool lrow_ok = cw + li < k;
    for (int q = kWB * wh; q < p; q += kWB * NS) {
      double av[16], bv[16];
#pragma unroll
      for (int s4 = 0; s4 < 16; ++s4) {
        av[s4] = load_if(zrow + q + 4 * s4 + lk, row_ok);
        bv[s4] = load_if(lrow + q + 4 * s4 + lk, lrow_ok);
      }
#pragma unroll
      for (int s4 = 0; s4 < 16; ++s4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-av[s4], bv[s4], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) Tp[wh][(lk + 4 * r) * kWOp + 16 * wc + li] = acc[r];
    for (int e = tid; e < kWB * kWB; e += NT) {
      const int i = e / kWB, j = e % kWB;
      Y[i * kWOp + j] = Linv[(int64_t)(p + i) * ldi + p + j];
    }
    __syncthreads();
    if (tid < 16 * kWB) {
      const int i = tid / kWB, j = tid % kWB;
      double sum = 0.0;
#pragma unroll
      for (int h = 0; h < NS; ++h) sum += Tp[h][i * kWOp + j];
      T[i * kWOp + j] = sum;
    }
    __syncthreads();
    if (wh == 0) {
      f64x4 out = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k0 = 0; k0 < kWB; k0 += 16) out = tile_nt(out, T, 0, Y, 16 * wc, k0, kWOp, lane, 1.0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + lk + 4 * r, c = cw + li;
        if (i < n && c < k) Z[(int64_t)i * kp + c] = out[r];
      }
    }
    __threadfence_block();
    __syncthreads();  // T, Tp and Y are reused; the block's columns are visible to the workgroup's later loads
  }
}

// largest |S[i][j] - delta_ij| of a k x k matrix (ld k): how far the block is from orthonormal after a pass
__global__ void __launch_bounds__(256) wide_defect_kernel(const double* __restrict__ S, int k, double* __restrict__ partial) {
  double m = 0.0;
  const int64_t total = (int64_t)k * k;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / k, j = e % k;
    const double v = fabs(S[e] - (i == j ? 1.0 : 0.0));
    m = v > m || v != v ? v : m;  // a NaN wins
  }
  __shared__ double red[256];
  red[threadIdx.x] = m;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      const double o = red[threadIdx.x + st];
      if (o > red[threadIdx.x] || o != o) red[threadIdx.x] = o;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// Cholesky-QR of columns 0 .. k - 1 of the n x kp block Z of matrix b; a second pass when the first one leaves
// |Z^T Z - I| above 4e-15 sqrt(n) (clusters: the first pass's error grows with the square of the block's condition
// number; well-separated spectra come out orthonormal to rounding and skip it).  Synchronises (one 8-byte read per
// pass).  S (k x k, ld k), Linv (ld kw) and gram_ws are the wide workspaces of the layout.
int wide_orthonormalise(TrdDesc* desc_b, double* Z, int n, int k, int kp, double* S, double* Linv, int kw, void* gram_ws,
                        int64_t gram_bytes, hipStream_t s) {
  const int nblk = (k + kWB - 1) / kWB;
  constexpr int kDefectBlocks = 256;
  for (int pass = 0; pass < 3; ++pass) {
    NDMPS_TRY(ndmps_gram_f64(Z, n, k, kp, S, gram_ws, gram_bytes, s));
    if (pass >= 1) {
      // partial maxima behind the Gram matrix in Linv (free between passes)
      hipLaunchKernelGGL(wide_defect_kernel, dim3(kDefectBlocks), dim3(256), 0, s, (const double*)S, k, Linv);
      NDMPS_LAUNCH_CHECK();
      double host[kDefectBlocks];
      NDMPS_CHECK_HIP(hipMemcpyAsync(host, Linv, sizeof(host), hipMemcpyDeviceToHost, s));
      NDMPS_CHECK_HIP(hipStreamSynchronize(s));
      double defect = 0.0;
      for (double v : host) defect = (v > defect || v != v) ? v : defect;
      if (defect <= 4e-15 * sqrt((double)n)) break;
      if (pass == 2) break;  // two passes are what the method has; a block that is still off is reported by its status
    }
    for (int pb = 0; pb < nblk; ++pb) {
      const int p = kWB * pb, below = nblk - pb - 1;
      hipLaunchKernelGGL(wide_chol_diag_kernel, dim3(1), dim3(512), (size_t)2 * kWB * kWLd * sizeof(double), s, S, k, Linv, kw, k,
                         p, desc_b);
      if (below > 0) {
        hipLaunchKernelGGL(wide_chol_panel_kernel, dim3((unsigned)below), dim3(256), 0, s, S, k, Linv, kw, k, p);
        hipLaunchKernelGGL(wide_chol_trail_kernel, dim3((unsigned)(below * (below + 1) / 2)), dim3(256), 0, s, S, k, k, p);
      }
    }
    hipLaunchKernelGGL(wide_trsm_kernel, dim3((unsigned)ndmps::ceil_div(n, 16)), dim3(64 * kTrsmWaves), 0, s, Z, kp, n, k, S, k,
                       Linv, kw);
    NDMPS_LAUNCH_CHECK();
  }
  return NDMPS_OK;
}

// The same for at most 128 vectors of one or two BIG matrices whose rank is known on the device only (the sweep decides
// it there and never waits for it): all kp columns are factored, with the rows and columns of S from the rank on
// replaced by the identity -- those columns of Z (zeros: trd_invit_kernel clears the columns of its block behind the
// rank, so nothing the workspace held before meets the solve) neither enter the kept columns nor are touched; the
// back-transformation zero-fills them.  Two passes, no look at the defect (that
// would be a host read); a Cholesky breakdown is reported through the status word like everywhere.
__global__ void __launch_bounds__(256) wide_mask_rank_kernel(double* __restrict__ S, int k, const TrdDesc* __restrict__ d) {
  const int r = d->k;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < k * k; e += gridDim.x * 256) {
    const int i = e / k, j = e % k;
    if (i >= r || j >= r) S[e] = i == j ? 1.0 : 0.0;
  }
}
int wide_orthonormalise_auto(TrdDesc* desc_b, double* Z, int n, int kp, double* S, double* Linv, int kw, void* gram_ws,
                             int64_t gram_bytes, hipStream_t s) {
  const int k = kp, nblk = (k + kWB - 1) / kWB;
  for (int pass = 0; pass < 2; ++pass) {
    NDMPS_TRY(ndmps_gram_f64(Z, n, k, kp, S, gram_ws, gram_bytes, s));
    hipLaunchKernelGGL(wide_mask_rank_kernel, dim3(16), dim3(256), 0, s, S, k, (const TrdDesc*)desc_b);
    for (int pb = 0; pb < nblk; ++pb) {
      const int p = kWB * pb, below = nblk - pb - 1;
      hipLaunchKernelGGL(wide_chol_diag_kernel, dim3(1), dim3(512), (size_t)2 * kWB * kWLd * sizeof(double), s, S, k, Linv, kw, k,
                         p, desc_b);
      if (below > 0) {
        hipLaunchKernelGGL(wide_chol_panel_kernel, dim3((unsigned)below), dim3(256), 0, s, S, k, Linv, kw, k, p);
        hipLaunchKernelGGL(wide_chol_trail_kernel, dim3((unsigned)(below * (below + 1) / 2)), dim3(256), 0, s, S, k, k, p);
      }
    }
    hipLaunchKernelGGL(wide_trsm_kernel, dim3((unsigned)ndmps::ceil_div(n, 16)), dim3(64 * kTrsmWaves), 0, s, Z, kp, n, k, S, k,
                       Linv, kw);
    NDMPS_LAUNCH_CHECK();
  }
  return NDMPS_OK;
}

// strict upper triangle of an n x n matrix (ld n) <- 0: the Cholesky factor as a dense operand
__global__ void __launch_bounds__(256) wide_zero_upper_kernel(double* __restrict__ S, int n) {
  const int64_t total = (int64_t)n * n;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / n, c = e % n;
    if (c > r) S[e] = 0.0;
  }
}

// ---------------------------------------------------------------------------------------- back-transformation
// V = Q Z for MANY columns (k > 128), Q = H_0 H_1 .. H_{n-2}: the reflectors in blocks of 64 in compact-WY form,
// H_{j0} .. H_{j0+63} = I - Y T Y^T (Y = the block's reflectors as columns, T upper triangular: LAPACK's dlarft,
// forward / columnwise), applied from the last block to the first.  Columns of V are independent: a workgroup owns 16
// of them and runs through ALL blocks on its own -- no launch per block, no exchange --, per block
//     W = Y^T X (64 x 16, K = the rows below the block's first reflector), W <- T W, X <- X - Y W
// on v_mfma_f64_16x16x4_f64, X (its n x 16 slab of the result, in place in V_out) and Y streamed from L2.
// 4 n^2 k flops; trd_back_kernel replays one reflector at a time on the VALU (order 4096, all vectors: 31.5 ms).
constexpr int kBwB = 64;   // reflectors per block
constexpr int kBwC = 16;   // columns per workgroup

// T factors of every block: grid (blocks, B).  S = Y^T Y on the MFMA, then the dlarft recurrence in LDS.
__global__ void __launch_bounds__(256) back_wide_t_kernel(const TrdDesc* __restrict__ desc, TrdWork w, double* __restrict__ Tw,
                                                          int64_t tw_stride) {
  const TrdDesc& d = desc[blockIdx.y];
  const int n = d.n, lda = w.lda;
  const int j0 = kBwB * (int)blockIdx.x;
  if (j0 > n - 2) return;
  const int nq = min(kBwB, n - 1 - j0);  // reflectors j0 .. j0 + nq - 1
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int64_t b = blockIdx.y;
  const double* Vh = w.Vh + b * w.n_max * lda;
  const double* tau = w.tau + b * w.n_max;
  __shared__ double S[kBwB][kBwB + 1], T[kBwB][kBwB + 1];
  // S[a][c] = sum_i Y[i][a] Y[i][c]; wave w: rows 16 w .. of S, four column tiles
  f64x4 acc[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) acc[ct] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int i_lo = (j0 + 1) & ~3;
  for (int i = i_lo; i < n; i += 16) {  // four k-steps' operands in flight (one at a time: 0.43 ms at order 2048)
    double av[4], bv[4][4];
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      const int ii = i + 4 * s4 + lk;
      av[s4] = load_if(Vh + (int64_t)(j0 + min(16 * wave + li, nq - 1)) * lda + min(ii, n - 1), 16 * wave + li < nq && ii < n);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        bv[s4][ct] = load_if(Vh + (int64_t)(j0 + min(16 * ct + li, nq - 1)) * lda + min(ii, n - 1), 16 * ct + li < nq && ii < n);
    }
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s4], bv[s4][ct], acc[ct], 0, 0, 0);
  }
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) S[16 * wave + lk + 4 * r][16 * ct + li] = acc[ct][r];
  for (int e = tid; e < kBwB * kBwB; e += 256) T[e / kBwB][e % kBwB] = 0.0;
  __syncthreads();
  // T[i][i] = tau_i;  T[0:i][i] = -tau_i T[0:i][0:i] S[0:i][i]   (column by column; thread r owns row r)
  for (int i = 0; i < nq; ++i) {
    const double ti = tau[j0 + i];
    double v = 0.0;
    if (tid < i) {
      for (int c = tid; c < i; ++c) v = fma(T[tid][c], S[c][i], v);
      v *= -ti;
    }
    __syncthreads();
    if (tid < i) T[tid][i] = v;
    if (tid == i) T[i][i] = ti;
    __syncthreads();
  }
  double* out = Tw + b * tw_stride + (int64_t)blockIdx.x * kBwB * kBwB;
  for (int e = tid; e < kBwB * kBwB; e += 256) out[e] = T[e / kBwB][e % kBwB];
}

// grid (ceil(k / 16), B), 1024 threads: X = V_out[:, c0 .. c0 + 16) of matrix b.  Sixteen waves: a wave alone on its
// SIMD waits out every load of the two streaming passes (the first version, four waves: 17 ms at order 4096, 10 % of
// the MFMA rate); W = Y^T X is split four ways over the rows and summed in LDS, the update deals its row tiles to all.
constexpr int kBwWaves = 16;
__global__ void __launch_bounds__(64 * kBwWaves) back_wide_kernel(const TrdDesc* __restrict__ desc, TrdWork w,
                                                                const double* __restrict__ Tw, int64_t tw_stride) {
  constexpr int NT = 64 * kBwWaves;
  const TrdDesc& d = desc[blockIdx.y];
  const int n = d.n, k = d.k, kp = w.kp, lda = w.lda;
  const int c0 = kBwC * (int)blockIdx.x;
  if (c0 >= k) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int wq = wave & 3, wsplit = wave >> 2;  // row tile of W, share of the rows
  const int64_t b = blockIdx.y;
  const double* Z = w.Z + b * w.n_max * kp;
  const double* Vh = w.Vh + b * w.n_max * lda;
  const double* Tb = Tw + b * tw_stride;
  double* X = d.V_out;  // ld n
  __shared__ double Ts[kBwB][kBwB + 4];
  __shared__ double Wp[kBwWaves / 4][kBwB][kBwC + 1];
  __shared__ double Ws[kBwB][kBwC + 1], W2[kBwB][kBwC + 1];
  __shared__ double sgn[kBwC];
  const bool col_ok = c0 + li < k;
  // X <- Z (the workgroup's columns)
  for (int e = tid; e < n * kBwC; e += NT) {
    const int i = e / kBwC, c = e % kBwC;
    if (c0 + c < k) X[(int64_t)i * n + c0 + c] = Z[(int64_t)i * kp + c0 + c];
  }
  __threadfence_block();
  __syncthreads();
  const int nblocks = n >= 2 ? (n - 2) / kBwB + 1 : 0;
  for (int g = nblocks - 1; g >= 0; --g) {
    const int j0 = kBwB * g, nq = min(kBwB, n - 1 - j0);
    const int i_lo = (j0 + 1) & ~15;
    for (int e = tid; e < kBwB * kBwB; e += NT) Ts[e / kBwB][e % kBwB] = Tb[(int64_t)g * kBwB * kBwB + e];
    // ---- W = Y^T X: wave (wq, wsplit): rows 16 wq .. of W over the rows i_lo + 16 wsplit, + 64, ...
    {
      f64x4 acc = {0.0, 0.0, 0.0, 0.0};
      const bool q_ok = 16 * wq + li < nq;
      const double* yrow = Vh + (int64_t)(j0 + min(16 * wq + li, nq - 1)) * lda;
      for (int i = i_lo + 16 * wsplit; i < n; i += 16 * (kBwWaves / 4)) {
        double av[4], bv[4];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
          const int ii = i + 4 * s4 + lk;
          av[s4] = load_if(yrow + min(ii, n - 1), q_ok && ii < n);
          bv[s4] = load_if(X + (int64_t)min(ii, n - 1) * n + min(c0 + li, k - 1), col_ok && ii < n);
        }
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s4], bv[s4], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) Wp[wsplit][16 * wq + lk + 4 * r][li] = acc[r];
    }
    __syncthreads();
    if (tid < kBwB * kBwC) {
      const int q = tid / kBwC, c = tid % kBwC;
      double sum = 0.0;
#pragma unroll
      for (int h = 0; h < kBwWaves / 4; ++h) sum += Wp[h][q][c];
      Ws[q][c] = sum;
    }
    __syncthreads();
    // ---- W2 = T W (upper triangular T), four waves
    if (wave < 4) {
      f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s4 = 0; s4 < 16; ++s4)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ts[16 * wave + li][4 * s4 + lk], Ws[4 * s4 + lk][li], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) W2[16 * wave + lk + 4 * r][li] = acc[r];
    }
    __syncthreads();
    // ---- X <- X - Y W2: row tiles of 16, dealt to the waves
    for (int i = i_lo + 16 * wave; i < n; i += 16 * kBwWaves) {
      f64x4 acc;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ii = i + lk + 4 * r;
        acc[r] = load_if(X + (int64_t)min(ii, n - 1) * n + min(c0 + li, k - 1), ii < n && col_ok);
      }
      const bool i_ok = i + li < n;
      double av[16];
#pragma unroll
      for (int s4 = 0; s4 < 16; ++s4) {
        const int q = 4 * s4 + lk;
        av[s4] = -load_if(Vh + (int64_t)(j0 + min(q, nq - 1)) * lda + min(i + li, n - 1), i_ok && q < nq);
      }
#pragma unroll
      for (int s4 = 0; s4 < 16; ++s4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s4], W2[4 * s4 + lk][li], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ii = i + lk + 4 * r;
        if (ii < n && col_ok) X[(int64_t)ii * n + c0 + li] = acc[r];
      }
    }
    __threadfence_block();
    __syncthreads();  // the slab is up to date for the next block; Ts / Ws / W2 are free
  }
  // ---- sign convention of the library: the largest-magnitude component of every column is positive
  {
    __shared__ double sb[kBwWaves][kBwC], sv[kBwWaves][kBwC];
    __shared__ int si[kBwWaves][kBwC];
    const int c = tid & 15, part = tid >> 4;  // 64 parts of the rows per column
    double best = -1.0, val = 0.0;
    int bi = 0x7fffffff;
    if (c0 + c < k)
      for (int i = part; i < n; i += NT / 16) {
        const double x = X[(int64_t)i * n + c0 + c];
        if (fabs(x) > best) {
          best = fabs(x);
          val = x;
          bi = i;
        }
      }
    // fold the parts of a column: lanes with equal (lane % 16) inside a wave, then the waves
#pragma unroll
    for (int off = 16; off < 64; off <<= 1) {
      const double ob = __shfl_xor(best, off, 64), ov = __shfl_xor(val, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (ob > best || (ob == best && oi < bi)) {
        best = ob;
        val = ov;
        bi = oi;
      }
    }
    if (lane < 16) {
      sb[wave][lane] = best;
      sv[wave][lane] = val;
      si[wave][lane] = bi;
    }
    __syncthreads();
    if (tid < 16) {
      double b2 = sb[0][tid], v2 = sv[0][tid];
      int i2 = si[0][tid];
      for (int ww = 1; ww < kBwWaves; ++ww)
        if (sb[ww][tid] > b2 || (sb[ww][tid] == b2 && si[ww][tid] < i2)) {
          b2 = sb[ww][tid];
          v2 = sv[ww][tid];
          i2 = si[ww][tid];
        }
      sgn[tid] = v2 < 0.0 ? -1.0 : 1.0;
    }
    __syncthreads();
    for (int e = tid; e < n * kBwC; e += NT) {
      const int i = e / kBwC, cc = e % kBwC;
      if (c0 + cc < k && sgn[cc] < 0.0) X[(int64_t)i * n + c0 + cc] = -X[(int64_t)i * n + c0 + cc];
    }
  }
}

// ---------------------------------------------------------------- back-transformation, rows dealt to the chip
// V = Q Z for at most 128 columns of ONE or two big matrices: a workgroup per 16 columns (back_wide_kernel) leaves all
// but 8 compute units idle, and one reflector at a time (trd_back_kernel) is 1.66 ms at order 2048.  Here the ROWS are
// dealt out: workgroup (chunk, tile) owns 128 rows x 32 columns of X, one launch per block of 64 reflectors (last
// block first), in which it
//     apply   W = sum over the chunks of the partial products of the block (fixed order: deterministic),
//             W2 = T W,  X_chunk <- X_chunk - Y_chunk W2
//     form    its partial product Y'_chunk^T X_chunk for the NEXT block (the one before), X still in registers:
//             the accumulator layout of a 16 x 16 tile of X is the B-operand layout of the four k-steps of its rows
// so the exchange between the chunks is the kernel boundary.  35 launches at order 2048.
constexpr int kBrR = 256;  // rows per workgroup
constexpr int kBrC = 16;   // columns per workgroup

// X <- Z for the kept columns, zeros up to k_fill.  k_fill is the batch's (min(k_cap, n_max)): a member of a smaller
// order has n columns only, and a column index past them would land in the next row of its V (ld n)
__global__ void __launch_bounds__(256) back_rows_init_kernel(const TrdDesc* __restrict__ desc, TrdWork w, int k_fill) {
  const TrdDesc& d = desc[blockIdx.y];
  const int n = d.n, k = d.k, kp = w.kp;
  const int cols = min(max(k, k_fill), n);
  const double* Z = w.Z + (int64_t)blockIdx.y * w.n_max * kp;
  double* X = d.V_out;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < (int64_t)n * cols; e += (int64_t)gridDim.x * 256) {
    const int i = (int)(e / cols), c = (int)(e % cols);
    X[(int64_t)i * n + c] = c < k ? Z[(int64_t)i * kp + c] : 0.0;
  }
}

// grid (chunks, column tiles, B).  g_apply / g_form: block whose update is applied / whose partial products are formed
// (-1: none).  part: [2][chunks][64][kp] per matrix, the buffer of block g is part[g & 1].
// A launch is a chain of memory round trips if its loads are issued where they are used (23 us per launch at order
// 2048): every operand whose address does not depend on the launch's own arithmetic -- the tiles of X, the rows of T,
// both blocks of reflectors, the partial products -- is requested before the first wait.
__global__ void __launch_bounds__(256) back_rows_step_kernel(const TrdDesc* __restrict__ desc, TrdWork w,
                                                            const double* __restrict__ Tw, int64_t tw_stride,
                                                            double* __restrict__ part, int64_t part_stride, int chunks,
                                                            int g_apply, int g_form) {
  const TrdDesc& d = desc[blockIdx.z];
  const int n = d.n, k = d.k, kp = w.kp, lda = w.lda;
  const int r0 = kBrR * (int)blockIdx.x, c0 = kBrC * (int)blockIdx.y;
  if (r0 >= n || c0 >= k) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int64_t b = blockIdx.z;
  const double* Vh = w.Vh + b * w.n_max * lda;
  double* X = d.V_out;  // ld n
  double* pb = part + b * part_stride;
  const int64_t buf = (int64_t)chunks * kBwB * kp;
  __shared__ double Ws[kBwB][kBrC + 1], W2[kBwB][kBrC + 1];
  const int nblocks = n >= 2 ? (n - 2) / kBwB + 1 : 0;
  if (g_apply >= nblocks) g_apply = -1;  // a smaller matrix of the batch
  if (g_form >= nblocks) g_form = -1;
  // does the chunk hold rows below the first reflector of block g?
  auto active = [&](int g) { return g >= 0 && r0 + kBrR - 1 >= kBwB * g + 1; };
  const bool do_apply = active(g_apply), do_form = active(g_form);
  if (!do_apply && !do_form) return;
  constexpr int RT = kBrR / 64;  // row tiles of 16 per wave: tiles wave, wave + 4, ...
#ifdef NDMPS_BR_STAMPS
  long long br_t[8];
  int br_n = 0;
#define BR_STAMP() { __builtin_amdgcn_s_waitcnt(0); br_t[br_n++] = wall_clock64(); }
#else
#define BR_STAMP()
#endif
  BR_STAMP()
  const bool col_ok = c0 + li < k;
  const int ja = kBwB * max(g_apply, 0), nqa = min(kBwB, n - 1 - ja);
  const int jf = kBwB * max(g_form, 0), nqf = min(kBwB, n - 1 - jf);
  // ---- every load of the launch
  f64x4 x[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ii = r0 + 16 * (wave + 4 * rt) + lk + 4 * r;
      x[rt][r] = load_if(X + (int64_t)min(ii, n - 1) * n + min(c0 + li, k - 1), ii < n && col_ok);
    }
  double tv[16], ya[RT][16], yf[RT][4][4];
  {
    const double* T = Tw + b * tw_stride + (int64_t)max(g_apply, 0) * kBwB * kBwB;
#pragma unroll
    for (int s4 = 0; s4 < 16; ++s4) tv[s4] = load_if(T + (16 * wave + li) * kBwB + 4 * s4 + lk, do_apply);
  }
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int i = r0 + 16 * (wave + 4 * rt);
    const bool live_a = do_apply && i + 15 >= ja + 1 && i + li < n;  // rows above a block's reflectors: Y is zero there
    const bool live_f = do_form && i + 15 >= jf + 1;
#pragma unroll
    for (int s4 = 0; s4 < 16; ++s4) {
      const int q = 4 * s4 + lk;
      ya[rt][s4] = -load_if(Vh + (int64_t)(ja + min(q, nqa - 1)) * lda + min(i + li, n - 1), live_a && q < nqa);
    }
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
      const int q = 16 * qt + li;
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        const int ii = i + 4 * s4 + lk;
        yf[rt][qt][s4] = load_if(Vh + (int64_t)(jf + min(q, nqf - 1)) * lda + min(ii, n - 1), live_f && q < nqf && ii < n);
      }
    }
  }
  BR_STAMP()
  if (do_apply) {
    const int first = (ja + 1) / kBrR;  // first chunk with rows below the block's first reflector
    const int live = min(chunks, (n + kBrR - 1) / kBrR);
    const double* src = pb + (g_apply & 1) * buf;
    {
      // W = the chunks' partial products in a fixed order, eight chunks' loads in flight
      constexpr int EPT = kBwB * kBrC / 256;
      double sum[EPT];
      int64_t at[EPT];
#pragma unroll
      for (int t = 0; t < EPT; ++t) {
        const int e = tid + 256 * t, q = e / kBrC, c = min(e % kBrC, k - 1 - c0);
        sum[t] = 0.0;
        at[t] = (int64_t)q * kp + c0 + c;
      }
      for (int ch = first; ch < live; ch += 8) {
        double v[8][EPT];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
          for (int t = 0; t < EPT; ++t) v[u][t] = load_if(src + (int64_t)min(ch + u, live - 1) * kBwB * kp + at[t], ch + u < live);
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
          for (int t = 0; t < EPT; ++t) sum[t] += v[u][t];
      }
#pragma unroll
      for (int t = 0; t < EPT; ++t) {
        const int e = tid + 256 * t;
        Ws[e / kBrC][e % kBrC] = c0 + e % kBrC < k ? sum[t] : 0.0;
      }
    }
    __syncthreads();
    BR_STAMP()
    // W2 = T W: wave w: rows 16 w .. of W2
    {
      f64x4 a0 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s4 = 0; s4 < 16; ++s4) a0 = __builtin_amdgcn_mfma_f64_16x16x4f64(tv[s4], Ws[4 * s4 + lk][li], a0, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) W2[16 * wave + lk + 4 * r][li] = a0[r];
    }
    __syncthreads();
    // X <- X - Y W2
    double w2[16];
#pragma unroll
    for (int s4 = 0; s4 < 16; ++s4) w2[s4] = W2[4 * s4 + lk][li];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int i = r0 + 16 * (wave + 4 * rt);
      if (i + 15 < ja + 1 || i >= n) continue;
#pragma unroll
      for (int s4 = 0; s4 < 16; ++s4) x[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(ya[rt][s4], w2[s4], x[rt], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ii = i + lk + 4 * r;
        if (ii < n && col_ok) X[(int64_t)ii * n + c0 + li] = x[rt][r];
      }
    }
  }
  BR_STAMP()
  if (do_form) {
    // partial W[q][c] = sum over the chunk's rows of Y[i][q] X[i][c]: per row tile four k-steps whose B operand is
    // the tile's accumulator element (row lk + 4 s of the tile = k index 4 s + lk)
    f64x4 acc[4];
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) acc[qt] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int qt = 0; qt < 4; ++qt)
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
          acc[qt] = __builtin_amdgcn_mfma_f64_16x16x4f64(yf[rt][qt][s4], x[rt][s4], acc[qt], 0, 0, 0);
    // the four waves' shares meet in Ws (free since W2 was formed), one wave after the other: a fixed order
    __syncthreads();
    for (int wv = 0; wv < 4; ++wv) {
      if (wave == wv) {
#pragma unroll
        for (int qt = 0; qt < 4; ++qt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double& cell = Ws[16 * qt + lk + 4 * r][li];
            cell = wv == 0 ? acc[qt][r] : cell + acc[qt][r];
          }
      }
      __syncthreads();
    }
    double* dst = pb + (g_form & 1) * buf + (int64_t)blockIdx.x * kBwB * kp;
    for (int e = tid; e < kBwB * kBrC; e += 256) {
      const int q = e / kBrC, c = e % kBrC;
      if (c0 + c < k) dst[(int64_t)q * kp + c0 + c] = Ws[q][c];
    }
  }
  BR_STAMP()
#ifdef NDMPS_BR_STAMPS
  if (tid == 0 && blockIdx.x == gridDim.x - 1 && blockIdx.y == 0 && g_apply >= 0 && g_form >= 0)
    for (int q = 0; q + 1 < br_n && q < 6; ++q) w.stamps[b * 16 + 9 + q] += br_t[q + 1] - br_t[q];
#endif
}

// sign convention of the library: the largest-magnitude component of every column is positive (first one on ties);
// grid (ceil(k_cap / 16), B), 1024 threads
__global__ void __launch_bounds__(1024) back_rows_sign_kernel(const TrdDesc* __restrict__ desc) {
  const TrdDesc& d = desc[blockIdx.y];
  const int n = d.n, k = d.k;
  const int c0 = 16 * (int)blockIdx.x;
  if (c0 >= k) return;
  double* X = d.V_out;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ double sb[16][16], sv[16][16], sgn[16];
  __shared__ int si[16][16];
  const int c = tid & 15, prt = tid >> 4;  // 64 parts of the rows per column
  double best = -1.0, val = 0.0;
  int bi = 0x7fffffff;
  if (c0 + c < k)
    for (int i = prt; i < n; i += 64) {
      const double x = X[(int64_t)i * n + c0 + c];
      if (fabs(x) > best) {
        best = fabs(x);
        val = x;
        bi = i;
      }
    }
#pragma unroll
  for (int off = 16; off < 64; off <<= 1) {
    const double ob = __shfl_xor(best, off, 64), ov = __shfl_xor(val, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (ob > best || (ob == best && oi < bi)) {
      best = ob;
      val = ov;
      bi = oi;
    }
  }
  if (lane < 16) {
    sb[wave][lane] = best;
    sv[wave][lane] = val;
    si[wave][lane] = bi;
  }
  __syncthreads();
  if (tid < 16) {
    double b2 = sb[0][tid], v2 = sv[0][tid];
    int i2 = si[0][tid];
    for (int ww = 1; ww < 16; ++ww)
      if (sb[ww][tid] > b2 || (sb[ww][tid] == b2 && si[ww][tid] < i2)) {
        b2 = sb[ww][tid];
        v2 = sv[ww][tid];
        i2 = si[ww][tid];
      }
    sgn[tid] = v2 < 0.0 ? -1.0 : 1.0;
  }
  __syncthreads();
  for (int e = tid; e < n * 16; e += 1024) {
    const int i = e / 16, cc = e % 16;
    if (c0 + cc < k && sgn[cc] < 0.0) X[(int64_t)i * n + c0 + cc] = -X[(int64_t)i * n + c0 + cc];
  }
}
