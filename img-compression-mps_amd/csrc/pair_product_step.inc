// One physical index i of the two-phase pair product (pair_product.h): the only definition of the two phases and their
// fencing.  Included inside the loop over i of a kernel of 256 threads; no include guard.  From the kernel it uses
//   Et, Z                         the two LDS images (__shared__ double[kPairLd * kPairLd]); Et holds E transposed
//   lr, lc, col                   lane >> 4, lane & 15, 16 wave + lc
//   tiles_re, tiles_co            16-row tiles of E and 16-column tiles of the result
//   steps1, steps2                k-steps of four of phase 1 (columns of E) and of phase 2 (rows of E)
//   own1, own2                    this wave's tile of Z / of the result exists
//   bq, aq (double[16])           this lane's operands of op(B_i) and op(A_i); bq is reloaded here for i + 1 < i1
//   kTrans, B, code_b, cb, d, cb2, i, i1      what that reload needs (pair_load_operands)
//   acc (f64x4[4])                the result, rows 16 wave + lr + 4 r, columns 16 nt + lc; accumulated over i
// Two barriers: after Z is written and after it is read.

      // ---- phase 1: Z_i[:, 16 wave ..] = E op(B_i)[:, 16 wave ..]
      ndmps::f64x4 z[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) z[mt] = (ndmps::f64x4){0.0, 0.0, 0.0, 0.0};
      if (own1) {
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
          if (ks < steps1) {
            const int k = 4 * ks + lr;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
              if (mt < tiles_re)
                z[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(Et[ndmps::pair_img(k, 16 * mt + lc)], bq[ks], z[mt], 0, 0, 0);
          }
          if (ks & 1) __builtin_amdgcn_sched_barrier(0);  // at most eight LDS operands in flight: no spill
        }
      }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) Z[ndmps::pair_img(16 * mt + lr + 4 * r, col)] = z[mt][r];
      __syncthreads();
      if (i + 1 < i1) ndmps::pair_load_operands<kTrans>(bq, B, code_b, cb, d, cb2, i + 1, lr, col, own1);
      // ---- phase 2: acc[16 wave .., :] += op(A_i)[16 wave .., :] Z_i
      if (own2) {
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
          if (ks < steps2) {
            const int k = 4 * ks + lr;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
              if (nt < tiles_co)
                acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(aq[ks], Z[ndmps::pair_img(k, 16 * nt + lc)], acc[nt], 0, 0, 0);
          }
          if (ks & 1) __builtin_amdgcn_sched_barrier(0);
        }
      }
      __syncthreads();  // Z, and Et where it is loaded per i, are rewritten by the next i
