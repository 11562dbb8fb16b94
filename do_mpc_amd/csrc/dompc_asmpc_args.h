// dompc_asmpc_args.h - kernel argument blocks of the sensitivity-based MPC law (dompc_asmpc.hip), shared with the generic host
// runtime (dompc_asmpc_runtime.cpp).  Plain data, no model-dependent sizes.
#pragma once
#include <stdint.h>

#include "dompc_affine.h"

namespace dompc_asmpck {
// law preparation: M = (I - G)^-1 J per loop, written into the law record `law` (its arrays are written here: the const is cast away)
struct PrepArgs {
  const double *x_prev, *u0;                 // [B][nx], [B][nu]: the states the batch was solved at and its inputs
  const double *J, *G;                       // du0/dx0 [nu][nx] and du0/du_prev [nu][nu] of loop b at J + b * batch_J + r * row_J + c
  const int32_t* ok;                         // [B]: 0 = the solve or its sensitivities failed
  int64_t row_J, batch_J, row_G, batch_G;
  dompc_affine::Law law;
  int32_t batch, pad;
};
// law step: U = sat(u_ref + M (X - x_ref)), one thread per loop
struct StepArgs {
  const double* x;                           // [B][nx]
  double* u;                                 // [B][nu]
  int32_t* status;                           // [B] (may be null): the bits of dompc_affine.h
  dompc_affine::Law law;
  int32_t batch, pad;
};
}  // namespace dompc_asmpck
