// The two-phase fp64 pair product on v_mfma_f64_16x16x4_f64 and what its users share on the device.  The users are the
// Gram matrix of a series (series.hip), its weighted form (wgram.hip), the sandwich of the elementwise product
// (hadamard.hip) and the three forms of the sketch of a sum (sumsketch.hip).  What is shared lives in three places:
//   pair_product_step.inc  the two phases of one physical index with their fencing (text, included at kernel level);
//   this header            the only definition of the LDS image (pair_img), of the operand loader
//                          (pair_load_operands), of the loaders of the Et image (pair_load_et, pair_set_unit) and of
//                          the guarded store of a wave's strip of accumulators (pair_store_strip); the site kernel of
//                          wgram.hip alone spells pair_load_et and pair_store_strip out itself, for its time;
//   pair_host.h            the host front end: lists of chains and their checks, the fp64 copies of cores, the device
//                          tables, the pair table and the general route's forward sandwich (gram_pass.h: the layout
//                          of a sketch and its Gram pass).
// DESIGN.md 5.38 maps which file uses which piece.
//
// One workgroup of four waves forms, for the physical indices i of a site,
//     acc (+)= op(A_i) ( E op(B_i) ),      op(X_i) = X[:, i, :]   (kEnv == false: op(A_i) is used transposed)
//                                          op(X_i) = X[:, i, :]^T (kEnv == true)
// for cores A (ca, d, ca2), B (cb, d, cb2) and E (re x ce), every extent <= 64:
//     kEnv == false:  acc (ca2 x cb2) = A_i^T E B_i,     E is ca x cb
//     kEnv == true:   acc (ca x cb)   = A_i E B_i^T,     E is ca2 x cb2
//   LDS   Et  64 x 64 fp64  E transposed, Et[k][m] = E[m][k]      32 KiB
//         Z   64 x 64 fp64  Z_i = E op(B_i), row-major            32 KiB      64 KiB: two workgroups per CU
//   Both images have 512-byte rows with the 16-column block index XORed by the row's parity.  An operand read of
//   v_mfma_f64_16x16x4_f64 takes 16 consecutive doubles of four consecutive rows; ds_read_b64 resolves banks per half
//   wave (two rows), and the XOR puts the odd row on the other 128-byte half of the bank row: no conflict.
//   Per physical index i:  phase 1, wave w forms column tile w of Z_i (four row tiles, 16 registers) with E from LDS
//   as the A operand and the core of b from GLOBAL memory as the B operand; phase 2, wave w accumulates row tile w of
//   the result (four column tiles, kept in accumulators over all i) with the core of a from global memory as the A
//   operand and Z_i from LDS as the B operand.  The cores are not staged through LDS: with this split of the tiles
//   every core element is the operand of exactly one wave, so a copy in LDS would be written once and read once;
//   instead each lane loads its <= 16 operands of a phase into registers one phase ahead (the core of a during
//   phase 1, the core of b of i + 1 during phase 2), in the storage type (fp32, bf16, fp64: widening is exact).  LDS
//   operand reads are fenced in groups of eight so that they do not pile up in registers.  Bonds that are not
//   multiples of 16 are zero-padded in registers and LDS; tiles past the bonds are skipped.  Order of summation is
//   fixed (k ascending inside a product, i ascending), nothing is shared between workgroups, and nothing waits.
//
// What differs between the users stays in their kernels: where E comes from, which i a workgroup runs and where the
// result goes.  The step of one i (phase 1, Z, phase 2) is the text of pair_product_step.inc, included at kernel level:
// as a function, inlined, it is optimised once on its own and once more inside the kernel, and that second round
// costs the kernels registers (6 VGPRs in the environment form of the sandwich, spills in other spellings).
#pragma once
#include "common.h"

namespace ndmps {

constexpr int kPairResident = 64;  // largest bond of the resident pair product
constexpr int kPairLd = 64;        // row length of the LDS images (doubles)

// element (row, col) of a 64 x 64 LDS image: odd rows hold their 16-column blocks pairwise swapped
__device__ __forceinline__ int pair_img(int row, int col) { return row * kPairLd + (col ^ ((row & 1) << 4)); }

// This lane's operands of one phase, q[ks] = op(core_i)[4 ks + lr][c], zero outside.
//   kTrans == false:  op(core_i)[k][c] = core[k, i, c]   (k < chi, c < chi2)
//   kTrans == true:   op(core_i)[k][c] = core[c, i, k]   (k < chi2, c < chi)
// Branch-free per element (a lane outside reads element 0 and discards it); the storage type is switched once per call.
template <typename T, bool kTrans>
__device__ __forceinline__ void pair_load_operands_as(double (&q)[16], const T* __restrict__ core, int chi, int d, int chi2,
                                                      int i, int lr, int c, bool active) {
  const int klim = kTrans ? chi2 : chi;
  const bool c_ok = active && c < (kTrans ? chi : chi2);
  const int64_t base = kTrans ? ((int64_t)c * d + i) * chi2 + lr : ((int64_t)lr * d + i) * chi2 + c;
  const int64_t step = kTrans ? (int64_t)4 : (int64_t)4 * d * chi2;
  T raw[16];
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) raw[ks] = core[(c_ok && 4 * ks + lr < klim) ? base + ks * step : 0];
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) q[ks] = (c_ok && 4 * ks + lr < klim) ? to_f64(raw[ks]) : 0.0;
}
template <bool kTrans>
__device__ __forceinline__ void pair_load_operands(double (&q)[16], const void* core, int code, int chi, int d, int chi2, int i,
                                                   int lr, int c, bool active) {
  if (code == 2) pair_load_operands_as<double, kTrans>(q, (const double*)core, chi, d, chi2, i, lr, c, active);
  else if (code == 1) pair_load_operands_as<__bf16, kTrans>(q, (const __bf16*)core, chi, d, chi2, i, lr, c, active);
  else pair_load_operands_as<float, kTrans>(q, (const float*)core, chi, d, chi2, i, lr, c, active);
}

// src (rows x cols, leading dimension ld) transposed into an LDS image, img[k][m] = src[m][k], zero outside.  A wave's
// pass reads 16 consecutive k of four rows m and writes four consecutive m of 16 image rows.
__device__ __forceinline__ void pair_load_et(double* img, const double* __restrict__ src, int rows, int cols, int64_t ld, int tid) {
  asm volatile("" : "+v"(tid));  // the addresses are formed here, per call: hoisted out of a kernel's loop they spill
  const int kk = tid & 15, mm = tid >> 4;
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
      const int k = 16 * kb + kk, m = 16 * mb + mm;
      const bool ok = k < cols && m < rows;
      const double v = src[ok ? (int64_t)m * ld + k : 0];
      img[pair_img(k, m)] = ok ? v : 0.0;
    }
}

// E_0 = [1] as an image: element (0, 0) one, zero elsewhere
__device__ __forceinline__ void pair_set_unit(double* img, int tid) {
  for (int e = tid; e < kPairLd * kPairLd; e += 256) img[e] = e == 0 ? 1.0 : 0.0;
}

// A wave's 16 x 64 strip of accumulators, rows 16 wave + lr + 4 r and columns 16 nt + lc, stored into out (row-major,
// leading dimension ld) where it lies inside rows x cols.  The caller folds a row or column offset into `out`.
__device__ __forceinline__ void pair_store_strip(double* out, int64_t ld, const f64x4 (&acc)[4], int rows, int cols, int wave,
                                                 int lr, int lc) {
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * wave + lr + 4 * r, c = 16 * nt + lc;
      if (row < rows && c < cols) out[(int64_t)row * ld + c] = acc[nt][r];
    }
}

}  // namespace ndmps
