// dompc_plant_args.h - kernel argument block of the batched plant integrator, shared by the generic host runtime
// (dompc_runtime.cpp) and the per-model device code (dompc_plant.hip).  Plain data, no model-dependent sizes.
#pragma once
#include <stdint.h>

#include "dompc_affine.h"

namespace dompc_plantk {
struct Args {
  const double *x, *u, *tvp, *p, *w, *v;     // [B][nx], then per-sample or shared (stride 0) rows of u, tvp, p, w, v
  double *x_next, *y;                        // [B][nx], [B][ny] (y may be null)
  int32_t* status;                           // [B] (may be null): bit 0 = step limit reached / NaN; steps taken in status >> 8
  int32_t batch, stride_u, stride_tvp, stride_p, stride_w, stride_v;
  int32_t max_steps;
  int32_t method;                            // 0: explicit pair, samples that turn out stiff repeat their interval with the implicit method;
                                             // 1: explicit Dormand-Prince 5(4) only; 2: implicit SDIRK 4(3) only
  double t_step, rtol, atol;
  double* z_guess;                           // [B][nz] or null: Newton start of the algebraic states per sample (in), their values at x_next (out)
  int32_t explicit_limit, pad;               // method 0: steps of the explicit pair after which a sample counts as stiff
};
// K control steps affine law -> plant step in one launch (dompc_plant_rollout_kernel): per sample and step k the law of
// dompc_affine.h at X_traj[k] gives U_traj[k], the plant step of `plant` takes X_traj[k], U_traj[k] to X_traj[k + 1]
struct RolloutArgs {
  Args plant;                                // batch, method, tolerances, limits; its x, u, tvp, p, x_next, status are set per step, w = v = y = null
  dompc_affine::Law law;
  double *X_traj, *U_traj;                   // [K + 1][B][nx] (row 0: the start, in), [K][B][nu]
  const double *tvp_rows, *p_rows;           // [K][ntvp], [K][np]: the plant's parameters of step k, shared by the batch
  int32_t *plant_status, *law_status;        // [K][B] each (may be null)
  int32_t K, pad;
};
}  // namespace dompc_plantk
