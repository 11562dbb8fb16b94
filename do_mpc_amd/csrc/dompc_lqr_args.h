// dompc_lqr_args.h - kernel argument block of the batched LQR design, shared by the generic host runtime (dompc_lqr_runtime.cpp)
// and the per-design device code (dompc_lqr.hip).  Plain data, no size that depends on the design.
#pragma once
#include <stdint.h>

namespace dompc_lqrk {
struct Args {
  double *A, *B;                             // [B][nx][nx], [B][nx][nu] row-major, the DISCRETE pair: read by a code object without a
                                             // model, written (when not null) by one with a model
  const double *x, *u, *tvp, *p;             // with a model: operating points [B][nx], [B][nu]; tvp / p per design or shared (stride 0)
  const double *Q, *R, *Pf;                  // design-size weights [n][n], [nu][nu] and terminal weight [n][n] (finite horizon only);
                                             // per design or shared (stride 0)
  double *K, *P;                             // out: gain [B][nu][n], Riccati solution / cost-to-go [B][n][n]
  int32_t* status;                           // [B] (may be null): bit 0 = the doubling iteration did not converge, bit 1 = singular or
                                             // non-finite block (K = 0, P = Q are returned), bit 2 (models with algebraic states) =
                                             // Newton on g = 0 did not converge, or g_z singular or not finite at the last iterate
                                             // (K = 0, P = Q, A = B = 0); iterations in bits 8 .. 23, Newton passes in bits 24 .. 30
  int32_t batch, stride_q, stride_r, stride_pf, stride_tvp, stride_p;
  int32_t n_horizon;                         // 0: infinite horizon (doubling); > 0: passes of the backward recursion
  int32_t max_iter;
  double t_step, tol;
  // models with algebraic states (LQR_NZ > 0): the index-1 reduction inside the design
  const double* z;                           // [B][nz] guess of the algebraic states at the operating points
  double* z_out;                             // [B][nz] (may be null): the consistent algebraic states (the last Newton iterate)
  double z_tol;                              // Newton stops at max |g| <= z_tol ...
  int32_t z_max_iter;                        // ... or after z_max_iter updates z <- z - g_z^-1 g (at most 127)
};
// dompc_lqr_pairs_kernel: the discrete pairs of a model at the B x K knots of B trajectories, one item (k, b) per row of 16 lanes
struct PairsArgs {
  const double *x, *u;                       // knots, step-major: [K][B][nx], [K][B][nu]
  const double *tvp, *p;                     // tvp of item (k, b) at k * stride_tvp_step + b * stride_tvp_loop ([K][ntvp] shared by the
                                             // batch: (ntvp, 0); [K][B][ntvp]: (B ntvp, ntvp)); p of loop b at b * stride_p
  const double* z;                           // [K][B][nz] Newton start of the algebraic states (LQR_NZ > 0)
  double *A, *B;                             // out: [K][B][nx][nx], [K][B][nx][nu]; zeros at a knot that failed
  double* z_out;                             // [K][B][nz] (may be null): the consistent algebraic states
  int32_t* status;                           // [K][B] (may be null): bit 1 = the exponential failed, bit 2 = Newton or the reduction
                                             // failed; Newton updates in bits 24 .. 30
  int32_t batch, steps;
  int64_t stride_tvp_step, stride_tvp_loop, stride_p;
  double t_step, z_tol;
  int32_t z_max_iter;
};

// dompc_lqr_tv_kernel: the time-varying backward recursion over K pairs for B trajectories, one trajectory per row of 16 lanes
struct TvArgs {
  const double *A, *B;                       // [K][B][nx][nx], [K][B][nx][nu]: the discrete pairs (model size)
  const int32_t* pair_status;                // [K][B] (may be null), the status words of the pairs launch: a non-zero low byte is a failed pair
  const double *Q, *R, *Pf;                  // design-size weights, per trajectory or shared (stride 0)
  double* K;                                 // out (may be null): gains [K][B][nu][n]
  double* M;                                 // out (may be null, standard mode only): law layout [K][nu][nx][ld], loop index fastest
  double* P;                                 // out (may be null): cost-to-go [K+1][B][n][n]
  double* P0;                                // out: [B][n][n]
  int32_t* status;                           // [B] (may be null): bit 1 = singular or non-finite block, bit 2 = failed or non-finite
                                             // pair, at the step in bits 8 .. 23: K_j = 0 for j <= step, P_0 = Q
  int32_t batch, steps, ld, stride_q, stride_r, stride_pf;
};
}  // namespace dompc_lqrk
