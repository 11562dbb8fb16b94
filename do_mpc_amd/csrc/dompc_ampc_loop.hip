// dompc_ampc_loop.hip - K control steps approximate MPC -> plant of B closed loops in ONE launch (BatchClosedLoopAMPC.run(fused=True),
// Simulator.rollout_ampc_device, C ABI: dompc_plant_ampc_loop_device).  The reference closes this loop one sample and one step at a
// time on the host: `u0 = approx_mpc.make_step(x0)`, `x0 = simulator.make_step(u0)`.
//
// The code object belongs to a PAIR: one lowered plant model (DOMPC_PLANT_HEADER) and one network shape (DOMPC_AMPC_HEADER); the
// weights stay runtime data.  It is a superset of the plant's own object - this file includes dompc_plant.hip whole, entry points and
// info kernel included, so that a plant handle opens it like any plant object - plus dompc_ampc_loop_kernel and its info kernel.
//
// One workgroup = one wavefront = 64 loops, and the wavefront alternates between two layouts per control step k:
//   network  dompc_ampck::step32 (dompc_ampc.hip, unchanged) for the wavefront's two groups of 32 samples, on the matrix cores: it
//            reads X_traj[k] (and, with an rterm, the inputs applied before: U_prev0 at k = 0, U_traj[k - 1] afterwards - the
//            clipped ones) in the tile layout and writes U_traj[k] in the accumulator layout, lane l holding sample l & 31 and the
//            output rows of its lane half.  ALL 64 lanes are live here whatever the batch is: the matrix step needs them, and step32
//            masks its loads and stores on `s < batch` itself;
//   plant    dompc_plantk::step_sample (dompc_plant.hip, unchanged) per thread, loop b = 64 * block + lane, from X_traj[k], U_traj[k],
//            W_traj[k], V_traj[k] to X_traj[k + 1], Y_traj[k], Z_traj[k] - the per-step block of loop_sample.  Lanes with b >= batch
//            skip it (and with it every store); the lanes reconverge behind the branch before the next network step.
// Hand-over: U_traj[k] is written by one lane and read by another, X_traj[k + 1] likewise - writer and reader are lanes of the SAME
// wavefront, so a workgroup-scope release / acquire with the stores drained (hand_over) between writer and reader is enough; no
// agent scope, no __threadfence().  The trajectories reach memory in any case: they are the records.
//
// step_sample is instantiated with SITE = 2: an instance of its own, so that the plant kernels of this object keep the call sites -
// and the inliner's decisions - they have in the plant's own object (see step_sample).
//
// Build flavours as dompc_plant.hip: hipcc --genco (product) or g++ -DDOMPC_HOST_EMU (tests).
#include "dompc_plant.hip"
#define DOMPC_AMPC_NO_ENTRY 1
#include "dompc_ampc.hip"
#include "dompc_ampc_loop_args.h"

namespace dompc_ampc_loopk {

using dompc_plantk::NX;
using dompc_plantk::NU;
static_assert(dompc_ampck::NO == NU, "the network's outputs are the plant's inputs");
static_assert(dompc_ampck::NI == NX || dompc_ampck::NI == NX + NU, "the network's input is x or [x; u_prev]");
constexpr bool RTERM = dompc_ampck::NI > NX;

#ifndef DOMPC_HOST_EMU
// what one lane of the wavefront stored is read by another: stores drained, workgroup-scope release, then acquire
__device__ __forceinline__ void hand_over() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
#else
inline void hand_over() {}
#endif

// the network step of control step k for the 64 loops from `first` on
AMPC_DEV void network_step(const AmpcLoopArgs& R, int k, int64_t first) {
  const dompc_plantk::LoopArgs& L = R.loop;
  const int64_t B = L.plant.batch;
  dompc_ampck::Args N;
  N.x = L.X_traj + (int64_t)k * B * NX;
  // (without an rterm U_prev0 is null and never read; the host's null, not a constant here: a null the compiler can see makes the
  //  branch of scaled_input that would read it undefined, and this ROCm's clang crashes while folding that away)
  N.u_prev = (RTERM && k > 0) ? L.U_traj + (int64_t)(k - 1) * B * NU : L.U_prev0;
  N.u = L.U_traj + (int64_t)k * B * NU;
  N.batch = L.plant.batch; N.nx = R.nx; N.clip = R.clip; N.pad_ = 0;
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    // weights and bounds are the same for both groups and for every step: read again per group they cost a cache hit, hoisted out of
    // the loops they would sit in hundreds of registers beside the integrator's (as in jac32)
    N.w = dompc_ampck::reloaded(R.w);
    N.par = dompc_ampck::reloaded(R.par);
    dompc_ampck::step32(N, first + 32 * (int64_t)half);
  }
}

// the plant step of control step k for loop b: the per-step block of dompc_plantk::loop_sample without a law
PLANT_DEV inline void plant_step(const dompc_plantk::LoopArgs& L, int k, int b) {
  using namespace dompc_plantk;
  const int64_t B = L.plant.batch;
  double* xk = L.X_traj + (int64_t)k * B * NX;
  Args A = L.plant;
  A.x = xk; A.u = L.U_traj + (int64_t)k * B * NU; A.stride_u = NU;
  A.tvp = L.tvp_rows + (int64_t)k * NTVP; A.stride_tvp = 0;
  if (L.p_loops) { A.p = L.p_loops; A.stride_p = NP; }
  else { A.p = L.p_rows + (int64_t)k * NP; A.stride_p = 0; }
  A.w = L.W_traj ? L.W_traj + (int64_t)k * B * NW : nullptr; A.stride_w = NW;
  A.v = L.V_traj ? L.V_traj + (int64_t)k * B * NV : nullptr; A.stride_v = NV;
  A.y = L.Y_traj ? L.Y_traj + (int64_t)k * B * NY : nullptr;
  A.x_next = xk + B * NX;
  A.status = L.plant_status ? L.plant_status + (int64_t)k * B : nullptr;
  step_sample<2>(A, b);
#if PLANT_NZ > 0
  if (L.Z_traj && A.z_guess)
    for (int i = 0; i < NZ; ++i) L.Z_traj[((int64_t)k * B + b) * NZ + i] = A.z_guess[(int64_t)b * NZ + i];
#endif
}

}  // namespace dompc_ampc_loopk

// what the pair object was built for: the argument block, the network's shape and the hash of its header
#define AMPC_LOOP_INFO(out, hash)                                                                                             \
  do {                                                                                                                        \
    using namespace dompc_ampck;                                                                                              \
    out[0] = (int64_t)sizeof(dompc_ampc_loopk::AmpcLoopArgs);                                                                 \
    out[1] = NI; out[2] = NO; out[3] = NH; out[4] = NN; out[5] = AMPC_ACT; out[6] = AMPC_OUT_ACT; out[7] = AMPC_SCALING;      \
    out[8] = PACKED;                                                                                                          \
    const char h_[] = AMPC_MODEL_HASH;                                                                                        \
    for (int i = 0; i < (int)sizeof(h_); ++i) hash[i] = h_[i];                                                                \
  } while (0)

#ifndef DOMPC_HOST_EMU
extern "C" __global__ void __launch_bounds__(64) dompc_ampc_loop_kernel(dompc_ampc_loopk::AmpcLoopArgs R) {
  using namespace dompc_ampc_loopk;
  const int64_t first = (int64_t)blockIdx.x * 64;
  const int64_t b = first + threadIdx.x;
  const bool live = b < R.loop.plant.batch;                // (no early return: the matrix steps need every lane)
#pragma unroll 1
  for (int k = 0; k < R.loop.K; ++k) {
    network_step(R, k, first);
    hand_over();                                           // U_traj[k]: accumulator layout -> thread per loop
    if (live) plant_step(R.loop, k, (int)b);
    hand_over();                                           // X_traj[k + 1]: thread per loop -> tile layout
  }
}
extern "C" __global__ void dompc_ampc_loop_info_kernel(int64_t* out, char* hash) {
  if (threadIdx.x == 0 && blockIdx.x == 0) AMPC_LOOP_INFO(out, hash);
}
#else
extern "C" void dompc_ampc_loop_hostemu_info(const void* args) { void* const* a = (void* const*)args; AMPC_LOOP_INFO(((int64_t*)a[0]), ((char*)a[1])); }
// per block of 64 loops and per step: the two step32 calls, then the plant step of each of its loops
extern "C" void dompc_ampc_loop_hostemu_run(const void* args) {
  using namespace dompc_ampc_loopk;
  const AmpcLoopArgs* R = (const AmpcLoopArgs*)args;
  const int64_t B = R->loop.plant.batch;
  for (int64_t first = 0; first < B; first += 64)
    for (int k = 0; k < R->loop.K; ++k) {
      network_step(*R, k, first);
      for (int64_t b = first; b < first + 64 && b < B; ++b) plant_step(R->loop, k, (int)b);
    }
}
#endif
