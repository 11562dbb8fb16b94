// dompc_asmpc_args.h - kernel argument blocks of the sensitivity-based MPC law (dompc_asmpc.hip), shared with the generic host
// runtime (dompc_asmpc_runtime.cpp).  Plain data, no model-dependent sizes.
#pragma once
#include <stdint.h>

#include "dompc_affine.h"

namespace dompc_asmpck {
// law preparation: M = (I - G)^-1 J per loop, written into the law record `law` (its arrays are written here: the const is cast away).
// slot (may be null: entry j goes to column j): entry j of the compact inputs goes to column slot[j] of the record, the other columns
// are not touched; a slot outside [0, law.ld) stores nothing.
struct PrepArgs {
  const double *x_prev, *u0;                 // [B][nx], [B][nu]: the states the batch was solved at and its inputs
  const double *J, *G;                       // du0/dx0 [nu][nx] and du0/du_prev [nu][nu] of loop b at J + b * batch_J + r * row_J + c
  const int32_t* ok;                         // [B]: 0 = the solve or its sensitivities failed
  const int32_t* slot;                       // [B] (may be null)
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
// ordered selection: idx[0 .. count) = the loops b with status[b] & mask != 0, ascending in b.  Two launches over workgroups that
// each own SELECT_SPAN consecutive loops: the first writes group_count[g], the second adds the counts of the workgroups before g
// and writes the indices; the last workgroup writes count.
constexpr int SELECT_THREADS = 256, SELECT_ROUNDS = 4, SELECT_SPAN = SELECT_THREADS * SELECT_ROUNDS;
struct SelectArgs {
  const int32_t* status;                     // [B]: what the law step wrote
  int32_t *idx, *count;                      // [B], [1]; entries of idx beyond count are not written
  int32_t* group_count;                      // [ceil(B / SELECT_SPAN)]: scratch of the runtime
  int32_t batch, mask;
};
}  // namespace dompc_asmpck
