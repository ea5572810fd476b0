// Bond truncation from two Gram matrices, shared by compress_bond (tt.hip) and the rounding of a linear
// combination (lincomb.hip).
//
// A bond joins a "metric" factor F and a "data" factor D; the tensor through the bond is F D.  Given only
//   Gf = F^T F  (chi x chi, the factor that is square-rooted: Lt Lt^T = Gf)  and
//   Gd = D D^T  (chi x chi),
// H = Lt^T Gd Lt = V diag(s^2) V^T carries the singular values s of F D.  compress_bond passes Gf = T2 T2^T and
// Gd = T1^T T1 (the roles mirrored); the linear-combination sweep passes Gf = the left Gram GL_k and Gd = C_k C_k^T.
#pragma once
#include "common.h"

namespace ndmps {

// Device buffers of one truncation (chi = order of both Gram matrices).  tmp and H must be carved one after the
// other: the Cholesky factorisation uses the 2 chi^2 doubles from tmp on as its scratch.
struct GramTrunc {
  int64_t chi;
  double* Lt;    // chi x chi: Lt Lt^T = Gf (Cholesky factor, or W D^(1/2))
  double* tmp;   // chi x chi: Gd Lt
  double* H;     // chi x chi: Lt^T Gd Lt (destroyed)
  double* V;     // chi x chi: eigenvectors of H, descending; the first k are valid on return
  double* P1;    // chi x chi: scratch
  double* w2;    // chi: eigenvalues of Gf
  double* wh;    // chi: eigenvalues of H (s^2, measured where in doubt)
  double* sig;   // chi: s = sqrt(max(wh, 0))
  char* ev_ws;
  int64_t ev_bytes;
};
// eigen-solver workspace of one truncation of order chi
int64_t gram_trunc_eig_bytes(int64_t chi);

// Decides the rank k and leaves Lt, tmp, V[:, :k] and sig on the device.  Gf is destroyed.
// Kept: s_j > c s_0 with c = max(cutoff, floor, abs_thr / s_0), at most max_bond (<= 0: no cap), at least one.
// abs_thr < 0: no absolute threshold.  abs_thr >= 0: k = 0 when s_0 <= abs_thr (nothing survives; with abs_thr = 0
// that is a zero tensor, whose s_0 = 0 would otherwise be kept and divided by).  f64_tails: the singular values in doubt below the
// cap are measured as |rows of `data` . Lt v_j| (fp64 storage, where the squared values cannot resolve the floor);
// data(r, c) = data[r rs + c cs], r < rows, c < chi, is a factor with data^T data = Gd.  h_s: chi host doubles (s).
// cap_decides: when the max_bond largest eigenvalues of H are clearly above the threshold, the direct solver's noise
// near the threshold cannot move the rank and H stays on the direct solver (compress_bond passes false: its
// historical choice of solver, so its cores do not change).
template <typename T>
int gram_truncate(const GramTrunc& g, double* Gf, const double* Gd, const T* data, int64_t rows, int64_t rs, int64_t cs,
                  double cutoff, double floor, double abs_thr, int64_t max_bond, bool f64_tails, bool cap_decides,
                  int64_t* k_out, double* h_s, hipStream_t s);

}  // namespace ndmps
