// dompc_ekf_args.h - kernel argument block of the batched extended Kalman filter, shared by the generic host runtime
// (dompc_ekf_runtime.cpp) and the per-model device code (dompc_ekf.hip).  Plain data, no model-dependent sizes.
#pragma once
#include <stdint.h>

namespace dompc_ekfk {
struct Args {
  double *x, *P;                             // [B][nx], [B][nx][nx] row-major: prior estimate in, posterior out (in place)
  const double *y, *u, *tvp, *p, *Q, *R;     // [B][ny]; per-filter or shared (stride 0) rows of u, tvp, p, Q (nx*nx), R (ny*ny)
  int32_t* status;                           // [B] (may be null): bit 0 = step limit reached / NaN right-hand side, bit 1 = S singular
                                             // or not finite (the a-priori x, P are returned), bit 2 = Newton on the algebraic equations
                                             // did not converge or g_z singular / not finite (x, P, z are not written: the prior
                                             // stays); integration steps in status >> 8
  int32_t batch, stride_u, stride_tvp, stride_p, stride_q, stride_r;
  int32_t max_steps;
  double t_step, rtol, atol;
  // models with algebraic states (EKF_NZ > 0; null / unused otherwise)
  double* z;                                 // [B][nz] (may be null: guess 0, nothing handed back): guess in, the algebraic states
                                             // consistent with the a-priori state out (in place); untouched on status bit 2
  int32_t* newton;                           // [B] (may be null): Newton updates of the filter in this call
  double z_tol;                              // Newton on g = 0 stops at max |g| <= z_tol ...
  int32_t z_max_iter;                        // ... or after z_max_iter updates of one solve (status bit 2)
};
}  // namespace dompc_ekfk
