// Stand-alone sanitizer run of the general plant rollout (csrc/dompc_plant.hip: loop_sample; csrc/dompc_plant_runtime.cpp:
// dompc_plant_rollout_device) on the host emulation: the DAE member of the probe family of tests/plant_family_common.py, B = 67 loops
// and K = 3 steps, every array an exact-size heap block - once with a law with a previous-input term, noise, measurements, algebraic
// states and parameters per loop, once open loop with shared parameter rows and nothing optional, and the refusals.
// Built and run by tools/rollout_sanitize.sh (g++ -fsanitize=address,undefined; no Python in the process).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../include/dompc_ipm.h"

static unsigned s_ = 12345;
static double rnd() { s_ = s_ * 1664525u + 1013904223u; return (double)(s_ >> 8) / (double)(1u << 24); }
static double* block(size_t n, double lo, double hi) {
  double* p = (double*)malloc(sizeof(double) * (n ? n : 1));
  for (size_t i = 0; i < n; ++i) p[i] = lo + (hi - lo) * rnd();
  return p;
}

int main() {
  const int nx = 3, nu = 1, np = 3, ntvp = 1, nw = 3, nv = 2, ny = 2, nz = 2, B = 67, K = 3;
  dompc_plant_desc d;
  memset(&d, 0, sizeof(d));
  d.nx = nx; d.nu = nu; d.np = np; d.ntvp = ntvp; d.nw = nw; d.nv = nv; d.ny = ny; d.discrete = 0;
  d.code_object_path = ""; d.model_hash = nullptr; d.t_step = 0.1; d.reltol = 1e-8; d.abstol = 1e-8;
  dompc_plant* h = nullptr;
  if (dompc_plant_create(&d, &h)) { printf("create: %s\n", dompc_plant_last_error(nullptr)); return 2; }
  if (dompc_plant_num_alg_states(h) != nz) return 3;
  double* X = block((size_t)(K + 1) * B * nx, -1.0, 1.0);
  double* U = block((size_t)K * B * nu, -1.0, 1.0);
  double* W = block((size_t)K * B * nw, -0.3, 0.3);
  double* V = block((size_t)K * B * nv, -0.1, 0.1);
  double* Y = block((size_t)K * B * ny, 0.0, 0.0);
  double* Z = block((size_t)K * B * nz, 0.0, 0.0);
  double* tvp = block((size_t)K * ntvp, -1.0, 1.0);
  double* P = block((size_t)B * np, 0.5, 2.0);              // lam, om, q per loop
  double* Prow = block((size_t)K * np, 0.5, 2.0);
  double* x_ref = block((size_t)nx * B, -1.0, 1.0);
  double* u_ref = block((size_t)nu * B, -1.0, 1.0);
  double* M = block((size_t)nu * nx * B, -1.0, 1.0);
  double* G = block((size_t)nu * nu * B, -0.5, 0.5);
  double* Up0 = block((size_t)B * nu, -1.0, 1.0);
  double* lb = block(nu, -0.8, -0.8);
  double* ub = block(nu, 0.8, 0.8);
  double* xs = block(nx, 1.0, 1.0);
  int32_t* pst = (int32_t*)malloc(sizeof(int32_t) * K * B);
  int32_t* lst = (int32_t*)malloc(sizeof(int32_t) * K * B);
  dompc_affine_law law;
  memset(&law, 0, sizeof(law));
  law.x_ref = x_ref; law.u_ref = u_ref; law.M = M; law.lb = lb; law.ub = ub; law.x_scale = xs; law.ld = B; law.max_dx = 0.5; law.clip = 1;
  dompc_plant_rollout_desc r;
  memset(&r, 0, sizeof(r));
  r.law = &law; r.G = G; r.up_ref = u_ref; r.U_prev0 = Up0; r.X_traj = X; r.U_traj = U; r.W_traj = W; r.V_traj = V; r.Y_traj = Y; r.Z_traj = Z;
  r.tvp_rows = tvp; r.p_loops = P; r.plant_status = pst; r.law_status = lst; r.reseed_z = 1;
  if (dompc_plant_rollout_device(h, B, K, &r, nullptr)) { printf("rollout: %s\n", dompc_plant_last_error(h)); return 4; }
  int failed = 0, clipped = 0;
  for (int i = 0; i < K * B; ++i) { failed += pst[i] & 1; clipped += (lst[i] >> 2) & 1; }
  printf("law + G + noise + y + z, B %d K %d: failed plant steps %d, clipped inputs %d, x[K][B-1] = %.6e %.6e %.6e, z = %.6e %.6e\n", B, K, failed,
         clipped, X[((size_t)K * B + B - 1) * nx], X[((size_t)K * B + B - 1) * nx + 1], X[((size_t)K * B + B - 1) * nx + 2],
         Z[((size_t)(K - 1) * B + B - 1) * nz], Z[((size_t)(K - 1) * B + B - 1) * nz + 1]);
  // open loop, shared parameter rows, nothing optional, the Newton starts carried
  dompc_plant_rollout_desc o;
  memset(&o, 0, sizeof(o));
  o.X_traj = X; o.U_traj = U; o.tvp_rows = tvp; o.p_rows = Prow;
  if (dompc_plant_rollout_device(h, B, K, &o, nullptr)) { printf("open loop: %s\n", dompc_plant_last_error(h)); return 5; }
  printf("open loop: x[K][0] = %.6e %.6e %.6e\n", X[(size_t)K * B * nx], X[(size_t)K * B * nx + 1], X[(size_t)K * B * nx + 2]);
  // refusals leave everything alone
  o.p_loops = P;
  if (dompc_plant_rollout_device(h, B, K, &o, nullptr) != 1) return 6;
  printf("refused: %s\n", dompc_plant_last_error(h));
  o.p_loops = nullptr; o.G = G;
  if (dompc_plant_rollout_device(h, B, K, &o, nullptr) != 1) return 7;
  printf("refused: %s\n", dompc_plant_last_error(h));
  if (dompc_plant_rollout_device(h, 0, K, &o, nullptr) != 0 || dompc_plant_rollout_device(h, B, 0, nullptr, nullptr) != 0) return 8;
  dompc_plant_destroy(h);
  free(X); free(U); free(W); free(V); free(Y); free(Z); free(tvp); free(P); free(Prow); free(x_ref); free(u_ref); free(M); free(G);
  free(Up0); free(lb); free(ub); free(xs); free(pst); free(lst);
  return failed ? 9 : 0;
}
