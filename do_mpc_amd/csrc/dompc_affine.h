// dompc_affine.h - the affine state feedback  u = sat(u_ref + M (x - x_ref))  of one loop, the law record it reads, and nothing else.
// Two kernel sources include it: the law step of dompc_asmpc.hip (one launch per control step) and the plant rollouts of dompc_plant.hip
// (K control steps in one launch; the general one through step_prev below).  All have to give the same bits, on the device and on the host, so the arithmetic is spelled
// out: one subtraction per state, then u_i = fma(M[i][k], x_k - x_ref_k, u_i) for k ASCENDING from u_i = u_ref_i, then the clip as
// two comparisons (not fmin / fmax: a NaN stays a NaN in its own row).  Nothing here may be rewritten as a sum the compiler is free
// to reassociate or contract differently in the two kernels.
//
// The law record.  Plain data, no model-dependent sizes; include/dompc_ipm.h declares the same layout as
// dompc_affine_law.  Arrays are laid out so that consecutive loops are consecutive in memory - one thread per loop reads them
// coalesced over the batch:
//   x_ref [nx][ld], u_ref [nu][ld], M [nu][nx][ld]  (entry of loop b at index ... * ld + b), flags [ld] (may be null: all zero),
//   lb / ub [nu] in physical units (may be +-inf; read only with clip != 0), x_scale [nx] (read only for max_dx).
// Status bits of a step: 0 and 1 copied from flags (the law of this loop is a fallback: M = 0), 2 = an input was clipped,
// 3 = max_k |x_k - x_ref_k| / x_scale_k > max_dx.  Bit 4 (value 16) is never written here: the event-triggered loop
// (closed_loop.BatchClosedLoopASMPC) sets it in the status it records for a loop that it re-solved at that step.
#pragma once
#include <math.h>
#include <stdint.h>

namespace dompc_affine {

struct Law {
  const double *x_ref, *u_ref, *M;
  const int32_t* flags;
  const double *lb, *ub, *x_scale;
  int64_t ld;
  double max_dx;
  int32_t clip, pad;
};

#ifdef DOMPC_AFFINE_FN               // (defined by a kernel source before the include: `__device__ inline` or `inline`)
#ifdef __clang__                     // (the loops over the sizes are unrolled: x, dx and u stay in registers)
#define DOMPC_AFFINE_UNROLL _Pragma("unroll")
#else
#define DOMPC_AFFINE_UNROLL
#endif
// x [NX] -> u [NU] for loop b; returns the status bits
template <int NX, int NU>
DOMPC_AFFINE_FN int step(const Law& L, int64_t b, const double* x, double* u) {
  int st = L.flags ? (L.flags[b] & 3) : 0;
  double dx[NX];
  bool far = false;
  DOMPC_AFFINE_UNROLL
  for (int k = 0; k < NX; ++k) {
    dx[k] = x[k] - L.x_ref[k * L.ld + b];
    far = far || fabs(dx[k] / L.x_scale[k]) > L.max_dx;
  }
  if (far) st |= 8;
  DOMPC_AFFINE_UNROLL
  for (int i = 0; i < NU; ++i) {
    double ui = L.u_ref[i * L.ld + b];
    DOMPC_AFFINE_UNROLL
    for (int k = 0; k < NX; ++k) ui = fma(L.M[((int64_t)i * NX + k) * L.ld + b], dx[k], ui);
    if (L.clip) {
      if (ui < L.lb[i]) { ui = L.lb[i]; st |= 4; }
      if (ui > L.ub[i]) { ui = L.ub[i]; st |= 4; }
    }
    u[i] = ui;
  }
  return st;
}

// The law with a previous-input term (the general plant rollout of dompc_plant.hip):
//   u = sat(u_ref + M (x - x_ref) + G (u_prev - up_ref)),   G [nu][nu][ld], up_ref [nu][ld] (it may alias u_ref), u_prev [NU].
// dx, `far` and the M chain are those of step(); with G non-null the SAME chain goes on, u_i = fma(G[i][j], u_prev_j - up_ref_j, u_i)
// for j ASCENDING, then the clip.  With G == nullptr this gives the bits of step() (nothing of u_prev or up_ref is read).
// u may not alias u_prev.
template <int NX, int NU>
DOMPC_AFFINE_FN int step_prev(const Law& L, const double* G, const double* up_ref, int64_t b, const double* x, const double* u_prev,
                              double* u) {
  int st = L.flags ? (L.flags[b] & 3) : 0;
  double dx[NX];
  bool far = false;
  DOMPC_AFFINE_UNROLL
  for (int k = 0; k < NX; ++k) {
    dx[k] = x[k] - L.x_ref[k * L.ld + b];
    far = far || fabs(dx[k] / L.x_scale[k]) > L.max_dx;
  }
  if (far) st |= 8;
  DOMPC_AFFINE_UNROLL
  for (int i = 0; i < NU; ++i) {
    double ui = L.u_ref[i * L.ld + b];
    DOMPC_AFFINE_UNROLL
    for (int k = 0; k < NX; ++k) ui = fma(L.M[((int64_t)i * NX + k) * L.ld + b], dx[k], ui);
    if (G) {
      DOMPC_AFFINE_UNROLL
      for (int j = 0; j < NU; ++j) ui = fma(G[((int64_t)i * NU + j) * L.ld + b], u_prev[j] - up_ref[j * L.ld + b], ui);
    }
    if (L.clip) {
      if (ui < L.lb[i]) { ui = L.lb[i]; st |= 4; }
      if (ui > L.ub[i]) { ui = L.ub[i]; st |= 4; }
    }
    u[i] = ui;
  }
  return st;
}
#endif

}  // namespace dompc_affine
