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
// The general rollout (dompc_plant_loop_kernel), for every plant: K control steps of one loop per thread, with the inputs from a law
// (has_law; optionally with a previous-input term G) or given in U_traj, noise, measurements, parameters per loop and algebraic
// states.  Per step k: u = law(X_traj[k], u_prev) -> U_traj[k] (or U_traj[k] is read), then the plant step of `plant` from X_traj[k]
// with U_traj[k], W_traj[k], V_traj[k] to X_traj[k + 1], Y_traj[k] and - from plant.z_guess - Z_traj[k].
struct LoopArgs {
  Args plant;                                // batch, method, tolerances, limits, z_guess; the per-step fields are set per step
  dompc_affine::Law law;                     // read only with has_law
  const double *G, *up_ref, *U_prev0;        // [nu][nu][ld], [nu][ld], [B][nu]: the previous-input term of the law (G null: none)
  double *X_traj, *U_traj;                   // [K + 1][B][nx] (row 0: the start, in), [K][B][nu] (out with a law, in without)
  const double *W_traj, *V_traj;             // [K][B][nw], [K][B][nv] (either may be null: zeros)
  double *Y_traj, *Z_traj;                   // [K][B][ny], [K][B][nz] (either may be null): measurement and algebraic states at X_traj[k + 1]
  const double *tvp_rows, *p_rows, *p_loops; // [K][ntvp], and either [K][np] shared by the batch or [B][np] per loop, constant over the steps
  int32_t *plant_status, *law_status;        // [K][B] each (may be null)
  int32_t K, has_law;
};
// The general rollout with a law record per step (dompc_plant_tvloop_kernel): the record of step k is `loop.law` with x_ref, u_ref, M
// and flags advanced by k nx law_step, k nu law_step, k nu nx law_step and k law_step elements - arrays [K][nx][ld], [K][nu][ld],
// [K][nu][nx][ld], [K][ld] with law_step = ld; lb, ub, x_scale, clip and max_dx are shared by the steps.  has_law = 1, G = null.
struct TvLoopArgs {
  LoopArgs loop;
  int64_t law_step;
};
}  // namespace dompc_plantk
