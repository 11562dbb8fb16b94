// dompc_ampc_args.h - kernel argument blocks of the batched approximate-MPC network step and of its Jacobian, shared by the generic host runtime
// (dompc_ampc_runtime.cpp) and the per-network device code (dompc_ampc.hip).  Plain data, no size that depends on the network.
#pragma once
#include <stdint.h>

namespace dompc_ampck {
struct Args {
  const double *x, *u_prev;                  // [B][nx], [B][n_in - nx] (null when the network input is x alone)
  double* u;                                 // out: [B][n_out]
  const float* w;                            // packed weights and biases of all layers (layout: dompc_ampc.hip, ampc.py:pack_weights)
  const double* par;                         // shift [n_in], range [n_in], lbu [n_out], ubu [n_out], ubu - lbu [n_out]
  int32_t batch, nx;
  int32_t clip;                              // != 0: max(., lbu) then min(., ubu)
  int32_t pad_;
};
// the Jacobian kernel: the step and, beside u, the network's Jacobian (a clipped output's row is zero)
struct JacArgs {
  Args step;
  double *du_dx, *du_du_prev;                // out: [B][n_out][nx], [B][n_out][n_in - nx] (null when the network input is x alone)
};
}  // namespace dompc_ampck
