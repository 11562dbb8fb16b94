// Stand-alone sanitizer run of the host device layer (csrc/dompc_host.h) under one of its runtimes: dompc_ampc_runtime.cpp + the kernel
// text of csrc/dompc_ampc.hip compiled by g++ with -DDOMPC_HOST_EMU for the network of lowering.lower_ampc(6, 2, 1, 50, "tanh", "linear",
// True), driven through the C ABI on exact-size heap blocks: creates that fail (nothing may leak), a refused set_weights, staging that
// grows and is reused, the Jacobian entry.  Built and run by tools/host_layer_sanitize.sh (g++ -fsanitize=address,undefined with leak
// detection on; no Python in the process).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../include/dompc_ipm.h"

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } \
  } while (0)

int main(int argc, char** argv) {
  CHECK(argc == 2);                      // the model hash of the generated header
  const int n_in = 6, n_out = 2, nx = 4, nup = n_in - nx;
  dompc_ampc_desc d;
  memset(&d, 0, sizeof(d));
  d.n_in = n_in; d.n_out = n_out; d.n_hidden_layers = 1; d.n_neurons = 50; d.act = 1; d.out_act = 4; d.scaling = 1; d.nx = nx;      // (activations: 1 tanh, 4 linear)
  d.code_object_path = ""; d.model_hash = argv[1];
  dompc_ampc* h = nullptr;

  // creates that fail: the reason is named, nothing is left behind
  dompc_ampc_desc bad = d;
  bad.model_hash = "not-the-hash";
  CHECK(dompc_ampc_create(&bad, &h) != 0 && h == nullptr);
  printf("wrong hash: %s\n", dompc_ampc_last_error(nullptr));
  CHECK(strstr(dompc_ampc_last_error(nullptr), "model hash mismatch"));
  bad = d;
  bad.n_in = n_in + 1;
  CHECK(dompc_ampc_create(&bad, &h) != 0 && h == nullptr);
  printf("wrong n_in: %s\n", dompc_ampc_last_error(nullptr));
  CHECK(strstr(dompc_ampc_last_error(nullptr), "different model dimensions"));

  CHECK(dompc_ampc_create(&d, &h) == 0 && h != nullptr);
  const int64_t n = dompc_ampc_packed_size(h);
  printf("packed weights: %lld floats\n", (long long)n);
  CHECK(n > 0);
  float* w = (float*)malloc(sizeof(float) * (size_t)n);
  unsigned s = 12345;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (double)(1u << 24) - 0.5; };
  for (int64_t i = 0; i < n; ++i) w[i] = (float)rnd();
  double* lb_in = (double*)malloc(sizeof(double) * n_in); double* ub_in = (double*)malloc(sizeof(double) * n_in);
  double* lbu = (double*)malloc(sizeof(double) * n_out); double* ubu = (double*)malloc(sizeof(double) * n_out);
  for (int i = 0; i < n_in; ++i) { lb_in[i] = -1.0 - i; ub_in[i] = 2.0 + i; }
  for (int i = 0; i < n_out; ++i) { lbu[i] = -2.0; ubu[i] = 5.0; }

  // a step before there are weights, and weights of the wrong length, are refused
  double x1[nx] = {0}, up1[nup] = {0}, u1[n_out];
  CHECK(dompc_ampc_step_batch(h, 1, x1, up1, u1, 1) != 0);
  CHECK(dompc_ampc_set_weights(h, w, n - 1, lb_in, ub_in, lbu, ubu) != 0);
  printf("wrong length: %s\n", dompc_ampc_last_error(h));
  CHECK(strstr(dompc_ampc_last_error(h), "packed weights have"));
  CHECK(dompc_ampc_set_weights(h, w, n, lb_in, ub_in, lbu, ubu) == 0);

  // the staging grows (3 -> 70) and is reused (5); every array has exactly the size of its call
  const int batches[3] = {3, 70, 5};
  for (int B : batches) {
    double* x = (double*)malloc(sizeof(double) * B * nx); double* up = (double*)malloc(sizeof(double) * B * nup);
    double* u = (double*)malloc(sizeof(double) * B * n_out);
    for (int i = 0; i < B * nx; ++i) x[i] = rnd();
    for (int i = 0; i < B * nup; ++i) up[i] = rnd();
    CHECK(dompc_ampc_step_batch(h, B, x, up, u, 1) == 0);
    for (int i = 0; i < B * n_out; ++i) CHECK(u[i] >= lbu[i % n_out] && u[i] <= ubu[i % n_out]);
    printf("step B = %d: u[0] = %.6e, u[last] = %.6e\n", B, u[0], u[B * n_out - 1]);
    free(x); free(up); free(u);
  }
  {
    const int B = 40;
    double* x = (double*)malloc(sizeof(double) * B * nx); double* up = (double*)malloc(sizeof(double) * B * nup);
    double* u = (double*)malloc(sizeof(double) * B * n_out); double* dx = (double*)malloc(sizeof(double) * B * n_out * nx);
    double* dup = (double*)malloc(sizeof(double) * B * n_out * nup);
    for (int i = 0; i < B * nx; ++i) x[i] = rnd();
    for (int i = 0; i < B * nup; ++i) up[i] = rnd();
    CHECK(dompc_ampc_jacobian_batch(h, B, x, up, u, dx, dup, 0) == 0);
    printf("jacobian B = %d: u[0] = %.6e, du_dx[0] = %.6e, du_du_prev[last] = %.6e\n", B, u[0], dx[0], dup[B * n_out * nup - 1]);
    free(x); free(up); free(u); free(dx); free(dup);
  }
  dompc_ampc_destroy(h);
  free(w); free(lb_in); free(ub_in); free(lbu); free(ubu);
  printf("host layer: clean\n");
  return 0;
}
