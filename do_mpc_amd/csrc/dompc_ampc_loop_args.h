// dompc_ampc_loop_args.h - kernel argument block of the fused approximate-MPC loop (dompc_ampc_loop.hip), shared by the plant runtime
// (dompc_plant_runtime.cpp), which launches it, and the device code of a (plant, network shape) pair.  Plain data, no size that
// depends on the plant or on the network.
#pragma once
#include <stdint.h>

#include "dompc_plant_args.h"

namespace dompc_ampc_loopk {
// K control steps network -> plant of B loops in one launch.  `loop` is the block of the general rollout with has_law = 0: the
// trajectories, the noise, the records, the parameter rows and the plant's settings mean what they mean there; U_traj is written by
// the network step, and loop.U_prev0 [B][nu] is the network's previous input at k = 0 (null when the network input is x alone).
struct AmpcLoopArgs {
  dompc_plantk::LoopArgs loop;
  const float* w;                            // packed weights and biases (dompc_ampck::Args::w)
  const double* par;                         // shift, range, lbu, ubu, ubu - lbu (dompc_ampck::Args::par)
  int32_t nx;                                // leading entries of the network input that come from x
  int32_t clip;                              // != 0: max(., lbu) then min(., ubu)
};
}  // namespace dompc_ampc_loopk
