// dompc_lanes_la.h - small dense linear algebra on the lane-row layer of dompc_lanes.h, for kernels that keep row r of a matrix in lane r
// of the group (the design of dompc_lqr.hip, the reduction of a model with algebraic states in dompc_ekf.hip): rows in and out of
// memory, the product with the rows of another matrix taken from their owners, and Gauss-Jordan elimination with partial pivoting over
// the lanes.  Templated on the group type (the `j` of the device flavour is all it reads); the two rules of dompc_lanes.h hold for
// every routine here: they read across lanes, so they are called from wavefront-uniform control flow only.
#pragma once
#include "dompc_lanes.h"

namespace dompc_lanes {

// column `c` of a row-major matrix with `nrows` rows: entry [lane][c]; 0 in the other lanes
#ifndef DOMPC_HOST_EMU
template <class G_> __device__ inline lv rows_load(const G_& G, const double* p, int stride, int c, int nrows) { return G.j < nrows ? p[G.j * stride + c] : 0.0; }
template <class G_> __device__ inline void rows_store(const G_& G, double* p, int stride, int c, lv v, int nrows, bool act) { if (act && G.j < nrows) p[G.j * stride + c] = v; }
#else
template <class G_> inline lv rows_load(const G_&, const double* p, int stride, int c, int nrows) { lv r; for (int l = 0; l < 16; ++l) r.e[l] = l < nrows ? p[l * stride + c] : 0.0; return r; }
template <class G_> inline void rows_store(const G_&, double* p, int stride, int c, const lv& v, int nrows, bool act) { if (act) for (int l = 0; l < nrows; ++l) p[l * stride + c] = v.e[l]; }
#endif

// out += M X: M with KN columns in the lanes that own its rows, X with KN rows (in lanes 0 .. KN-1) and NC columns
template <int KN, int NC>
DOMPC_LANES_FN void mm(lv (&out)[NC], lv (&M)[KN], lv (&X)[NC]) {
  dpp_ready(X);
  sfor<KN>([&](auto K_) {
    constexpr int k = K_;
    sfor<NC>([&](auto C_) { constexpr int c = C_; fmac_bc<k>(out[c], X[c], M[k]); });
  });
}
// Solves M Z = [X1 X2] in place of X1, X2 (M: NR x NR with its rows in lanes 0 .. NR-1, destroyed) by Gauss-Jordan elimination with
// partial pivoting over the lanes.  Rows are not swapped: column k takes as pivot the largest entry among the rows that have not been
// pivot yet, that row reaches the other lanes by lane_bcast, and row k of the solution is gathered from its lane at the end.
// Returns true when a pivot is zero or not finite (the results are then meaningless but every operation has been carried out).
// X2 = nullptr with NC2 = 0: one block of right-hand sides.
template <int NR, int NC1, int NC2, class G_>
DOMPC_LANES_FN bool gj_(const G_& G, lv (&M)[NR], lv (&X1)[NC1], lv* X2) {
  bool sing = false;
  const lv rows = lane_lt(G, NR);
  lv used = splat(1.0) - rows;                   // lanes without a row are never pivot
  lv where = splat(0.0);                         // lane k: the lane that holds row k of the solution
  sfor<NR>([&](auto K_) {
    constexpr int k = K_;
    const lv cand = lsel(used, splat(-1.0), lfabs(M[k]));
    double best = -1.0;
    int piv = 0;
    sfor<NR>([&](auto L_) {
      constexpr int l = L_;
      const double v = bc<l>(cand);
      const bool gt = v > best;                  // (false for NaN)
      best = gt ? v : best;
      piv = gt ? l : piv;
    });
    const bool ok = best > 0.0 && best < INFINITY;
    sing = sing || !ok;
    const lv isp = unit(G, piv);
    const double pv = lane_bcast(M[k], piv);
    const double inv = 1.0 / (ok ? pv : 1.0);
    const lv m = lsel(isp, splat(0.0), M[k] * inv);
    sfor<NR>([&](auto C_) {
      constexpr int c = C_;
      if constexpr (c > k) { const double pr = lane_bcast(M[c], piv); M[c] = lsel(isp, M[c] * inv, M[c] - m * pr); }
    });
    sfor<NC1>([&](auto C_) { constexpr int c = C_; const double pr = lane_bcast(X1[c], piv); X1[c] = lsel(isp, X1[c] * inv, X1[c] - m * pr); });
    sfor<NC2>([&](auto C_) { constexpr int c = C_; const double pr = lane_bcast(X2[c], piv); X2[c] = lsel(isp, X2[c] * inv, X2[c] - m * pr); });
    used = lsel(isp, splat(1.0), used);
    where = where + unit(G, k) * (double)piv;
  });
  sfor<NC1>([&](auto C_) { constexpr int c = C_; X1[c] = lsel(rows, lane_gather(X1[c], where), splat(0.0)); });
  sfor<NC2>([&](auto C_) { constexpr int c = C_; X2[c] = lsel(rows, lane_gather(X2[c], where), splat(0.0)); });
  return sing;
}
template <int NR, int NC1, int NC2, class G_>
DOMPC_LANES_FN bool gj(const G_& G, lv (&M)[NR], lv (&X1)[NC1], lv (&X2)[NC2]) { return gj_<NR, NC1, NC2>(G, M, X1, X2); }
template <int NR, int NC1, class G_>
DOMPC_LANES_FN bool gj(const G_& G, lv (&M)[NR], lv (&X1)[NC1]) { return gj_<NR, NC1, 0>(G, M, X1, nullptr); }


}  // namespace dompc_lanes
