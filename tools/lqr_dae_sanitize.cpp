// Stand-alone sanitizer run of the index-1 reduction of csrc/dompc_lqr.hip: the model of case (c) of tests/lqr_dae_common.py (cubic g, seven
// designs whose Newton iterations end after different numbers of passes) through dompc_lqr_hostemu_run, with and without z_out, on
// exact-size heap blocks.  Built and run by tools/lqr_dae_sanitize.sh (g++ -fsanitize=address,undefined; no Python in the process).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <stdint.h>
#include "dompc_lqr_args.h"
extern "C" void dompc_lqr_hostemu_info(const void* args);      // {int64_t* info, char* hash}
extern "C" void dompc_lqr_hostemu_run(const void* args);       // dompc_lqrk::Args
int main() {
  int64_t info[16] = {0}; char hash[64] = {0};
  void* const info_args[2] = {info, hash};
  dompc_lqr_hostemu_info(info_args);
  const int nx = info[0], nu = info[1], n = info[2], nz = info[9], B = 7;
  printf("nx %d nu %d n %d nz %d args %lld (sizeof %zu)\n", nx, nu, n, nz, (long long)info[8], sizeof(dompc_lqrk::Args));
  if (info[8] != (int64_t)sizeof(dompc_lqrk::Args)) return 2;
  // exact-size heap blocks: an access outside any of them is reported
  double* x = (double*)malloc(sizeof(double) * B * nx); double* u = (double*)malloc(sizeof(double) * B * nu);
  double* z = (double*)calloc(B * nz, sizeof(double)); double* zo = (double*)malloc(sizeof(double) * B * nz);
  double* Q = (double*)calloc(n * n, sizeof(double)); double* R = (double*)calloc(nu * nu, sizeof(double));
  double* K = (double*)malloc(sizeof(double) * B * nu * n); double* P = (double*)malloc(sizeof(double) * B * n * n);
  double* Ao = (double*)malloc(sizeof(double) * B * nx * nx); double* Bo = (double*)malloc(sizeof(double) * B * nx * nu);
  int32_t* st = (int32_t*)malloc(sizeof(int32_t) * B);
  const double scale[7] = {1e-3, 1e2, 1.0, 10.0, 0.1, 30.0, 3.0};
  unsigned s = 12345;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (double)(1u << 24); };
  for (int b = 0; b < B; ++b) { for (int i = 0; i < nx; ++i) x[b * nx + i] = scale[b] * (0.5 + 0.5 * rnd()) * (rnd() < 0.5 ? -1 : 1); for (int i = 0; i < nu; ++i) u[b * nu + i] = 2 * rnd() - 1; }
  for (int i = 0; i < n; ++i) Q[i * n + i] = 1.0;
  for (int i = 0; i < nu; ++i) R[i * nu + i] = 1.0;
  for (int with_zout = 0; with_zout < 2; ++with_zout) {
    dompc_lqrk::Args A; memset(&A, 0, sizeof(A));
    A.A = Ao; A.B = Bo; A.x = x; A.u = u; A.Q = Q; A.R = R; A.K = K; A.P = P; A.status = st; A.batch = B;
    A.max_iter = 50; A.t_step = 0.5; A.tol = 1e-13; A.z = z; A.z_out = with_zout ? zo : nullptr; A.z_tol = 1e-10; A.z_max_iter = 40;
    dompc_lqr_hostemu_run(&A);
    for (int b = 0; b < B; ++b) printf("design %d: status %d steps %d Newton %d K[0] %.6e\n", b, st[b] & 0xFF, (st[b] >> 8) & 0xFFFF, st[b] >> 24, K[b * nu * n]);
  }
  free(x); free(u); free(z); free(zo); free(Q); free(R); free(K); free(P); free(Ao); free(Bo); free(st);
  return 0;
}
