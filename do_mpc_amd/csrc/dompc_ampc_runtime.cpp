// dompc_ampc_runtime.cpp - host side of the batched approximate-MPC step behind the C ABI of include/dompc_ipm.h (dompc_ampc_*).
// Generic: sizes come from the per-network code object (dompc_ampc_info_kernel); weights and bounds are data of the handle.
// Build flavours as dompc_lqr_runtime.cpp: product = part of libdompc_ipm.so (HIP only); test = g++ -DDOMPC_HOST_EMU together with
// dompc_ampc.hip compiled as C++ (tests/_hostemu; never shipped).  dompc_host.h knows which one this is; this file does not.
#include "../../include/dompc_ipm.h"
#include "dompc_host.h"
#include "dompc_ampc_args.h"

// the host twins of the kernels (dompc_ampc.hip)
extern "C" void dompc_ampc_hostemu_info(const void* args);
extern "C" void dompc_ampc_hostemu_run(const void* args);
extern "C" void dompc_ampc_hostemu_jac(const void* args);

static thread_local std::string g_ampc_create_error;

struct dompc_ampc : dompc_host::Context {
  dompc_ampc_desc d;
  int64_t packed = 0;                    // floats of the packed weights the code object reads
  bool have_weights = false;
  float* w = nullptr;
  double* par = nullptr;
  int32_t cap = 0;
  double *s_x = nullptr, *s_up = nullptr, *s_u = nullptr;
  int32_t cap_jac = 0;                   // staging of the Jacobian's two outputs (its x, u_prev and u are the step's)
  double *s_dx = nullptr, *s_dup = nullptr;
  dompc_host::Kernel fn, fn_jac;
};

extern "C" const char* dompc_ampc_last_error(const dompc_ampc* h) { return h ? h->error.c_str() : g_ampc_create_error.c_str(); }

extern "C" void dompc_ampc_destroy(dompc_ampc* h) {
  if (!h) return;
  h->close();
  delete h;
}

extern "C" int dompc_ampc_create(const dompc_ampc_desc* desc, dompc_ampc** out) {
  if (!desc || !out) { g_ampc_create_error = "null argument"; return 1; }
  dompc_ampc* h = new dompc_ampc();
  h->d = *desc;
  h->device = desc->device;
  auto fail = [&]() { g_ampc_create_error = h->error; dompc_ampc_destroy(h); *out = nullptr; return 1; };
  if (desc->n_in <= 0 || desc->n_out <= 0) { h->error = "network without inputs or without outputs"; return fail(); }
  if (desc->nx <= 0 || desc->nx > desc->n_in) { h->error = "nx must be between 1 and n_in"; return fail(); }
  int64_t info[16] = {0};
  char hash[64] = {0};
  if (h->open("approximate MPC", desc->code_object_path, nullptr,
              {{"dompc_ampc_kernel", &h->fn, DOMPC_TWIN(dompc_ampc_hostemu_run)}, {"dompc_ampc_jac_kernel", &h->fn_jac, DOMPC_TWIN(dompc_ampc_hostemu_jac)}},
              "code object lacks the network kernels", "dompc_ampc_info_kernel", DOMPC_TWIN(dompc_ampc_hostemu_info), info, hash))
    return fail();
  const int64_t want[7] = {desc->n_in, desc->n_out, desc->n_hidden_layers, desc->n_neurons, desc->act, desc->out_act, desc->scaling ? 1 : 0};
  if (h->check_info("network ", info, want, 7, 7, sizeof(dompc_ampck::Args), hash, desc->model_hash)) return fail();
  if (info[9] != (int64_t)sizeof(dompc_ampck::JacArgs)) { h->error = "network argument layout mismatch between runtime and code object (Jacobian kernel)"; return fail(); }
  h->packed = info[8];
  if (h->packed <= 0) { h->error = "network code object reports no weights"; return fail(); }
  if (h->alloc((void**)&h->w, sizeof(float) * (size_t)h->packed) ||
      h->alloc((void**)&h->par, sizeof(double) * (size_t)(2 * desc->n_in + 3 * desc->n_out)))
    return fail();
  h->d.code_object_path = nullptr; h->d.model_hash = nullptr;
  *out = h;
  return 0;
}

extern "C" int64_t dompc_ampc_packed_size(const dompc_ampc* h) { return h ? h->packed : 0; }

extern "C" int dompc_ampc_set_weights(dompc_ampc* h, const float* packed, int64_t n, const double* lb_in, const double* ub_in,
                                      const double* lbu, const double* ubu) {
  if (!h) return 1;
  if (!packed || !lb_in || !ub_in || !lbu || !ubu) { h->error = "null pointer"; return 1; }
  if (n != h->packed) {
    char buf[160];
    snprintf(buf, sizeof(buf), "packed weights have %lld floats, the code object reads %lld", (long long)n, (long long)h->packed);
    h->error = buf;
    return 1;
  }
  const int ni = h->d.n_in, no = h->d.n_out;
  std::vector<double> par((size_t)(2 * ni + 3 * no));
  for (int i = 0; i < ni; ++i) { par[i] = lb_in[i]; par[ni + i] = ub_in[i] - lb_in[i]; }
  for (int i = 0; i < no; ++i) { par[2 * ni + i] = lbu[i]; par[2 * ni + no + i] = ubu[i]; par[2 * ni + 2 * no + i] = ubu[i] - lbu[i]; }
  if (h->set_device() || h->drain()) return 1;     // no step that still reads the old weights is in flight on any stream
  if (h->h2d(h->w, packed, sizeof(float) * (size_t)n) || h->h2d(h->par, par.data(), sizeof(double) * par.size()) || h->sync()) return 1;
  h->have_weights = true;
  return 0;
}

extern "C" int dompc_ampc_device_weights(dompc_ampc* h, const float** w, const double** par) {
  if (!h) return 1;
  if (!w || !par) { h->error = "null pointer"; return 1; }
  if (!h->have_weights) { h->error = "no weights: call dompc_ampc_set_weights first"; return 1; }
  *w = h->w; *par = h->par;
  return 0;
}

extern "C" int dompc_ampc_step_batch_device(dompc_ampc* h, int32_t B, const double* x, const double* u_prev, double* u, int32_t clip,
                                            void* stream) {
  if (!h) return 1;
  if (B <= 0) return 0;
  const dompc_ampc_desc& d = h->d;
  if (!h->have_weights) { h->error = "no weights: call dompc_ampc_set_weights first"; return 1; }
  if (!x || !u || (d.n_in > d.nx && !u_prev)) { h->error = "null pointer"; return 1; }
  dompc_ampck::Args G;
  memset(&G, 0, sizeof(G));
  G.x = x; G.u_prev = u_prev; G.u = u; G.w = h->w; G.par = h->par;
  G.batch = B; G.nx = d.nx; G.clip = clip ? 1 : 0;
  if (h->set_device()) return 1;
  // one wavefront per workgroup, 32 samples per wavefront
  return h->run(h->fn, (unsigned)(((int64_t)B + 31) / 32), 64, 0, stream, &G, sizeof(G));
}

extern "C" int dompc_ampc_step_batch(dompc_ampc* h, int32_t B, const double* x, const double* u_prev, double* u_out, int32_t clip) {
  if (!h) return 1;
  if (B <= 0) return 0;
  const dompc_ampc_desc& d = h->d;
  const int nup = d.n_in - d.nx;
  if (!x || !u_out || (nup > 0 && !u_prev)) { h->error = "null pointer"; return 1; }
  if (h->set_device()) return 1;
  const size_t D = sizeof(double);
  if (h->grow_staging(&h->cap, B, {{(void**)&h->s_x, D * d.nx}, {(void**)&h->s_up, D * nup}, {(void**)&h->s_u, D * d.n_out}})) return 1;
  if (h->h2d(h->s_x, x, D * B * d.nx) || (nup > 0 && h->h2d(h->s_up, u_prev, D * B * nup))) return 1;
  if (dompc_ampc_step_batch_device(h, B, h->s_x, nup > 0 ? h->s_up : nullptr, h->s_u, clip, h->stream_ptr())) return 1;
  if (h->d2h(u_out, h->s_u, D * B * d.n_out)) return 1;
  return h->sync();
}

extern "C" int dompc_ampc_jacobian_batch_device(dompc_ampc* h, int32_t B, const double* x, const double* u_prev, double* u, double* du_dx,
                                                double* du_du_prev, int32_t clip, void* stream) {
  if (!h) return 1;
  if (B <= 0) return 0;
  const dompc_ampc_desc& d = h->d;
  if (!h->have_weights) { h->error = "no weights: call dompc_ampc_set_weights first"; return 1; }
  if (!x || !u || !du_dx || (d.n_in > d.nx && (!u_prev || !du_du_prev))) { h->error = "null pointer"; return 1; }
  dompc_ampck::JacArgs G;
  memset(&G, 0, sizeof(G));
  G.step.x = x; G.step.u_prev = u_prev; G.step.u = u; G.step.w = h->w; G.step.par = h->par;
  G.step.batch = B; G.step.nx = d.nx; G.step.clip = clip ? 1 : 0;
  G.du_dx = du_dx; G.du_du_prev = d.n_in > d.nx ? du_du_prev : nullptr;
  if (h->set_device()) return 1;
  return h->run(h->fn_jac, (unsigned)(((int64_t)B + 31) / 32), 64, 0, stream, &G, sizeof(G));
}

extern "C" int dompc_ampc_jacobian_batch(dompc_ampc* h, int32_t B, const double* x, const double* u_prev, double* u_out, double* du_dx,
                                         double* du_du_prev, int32_t clip) {
  if (!h) return 1;
  if (B <= 0) return 0;
  const dompc_ampc_desc& d = h->d;
  const int nup = d.n_in - d.nx;
  if (!x || !u_out || !du_dx || (nup > 0 && (!u_prev || !du_du_prev))) { h->error = "null pointer"; return 1; }
  if (h->set_device()) return 1;
  const size_t D = sizeof(double);
  if (h->grow_staging(&h->cap, B, {{(void**)&h->s_x, D * d.nx}, {(void**)&h->s_up, D * nup}, {(void**)&h->s_u, D * d.n_out}}) ||
      h->grow_staging(&h->cap_jac, B, {{(void**)&h->s_dx, D * d.n_out * d.nx}, {(void**)&h->s_dup, D * d.n_out * nup}}))
    return 1;
  if (h->h2d(h->s_x, x, D * B * d.nx) || (nup > 0 && h->h2d(h->s_up, u_prev, D * B * nup))) return 1;
  if (dompc_ampc_jacobian_batch_device(h, B, h->s_x, nup > 0 ? h->s_up : nullptr, h->s_u, h->s_dx, nup > 0 ? h->s_dup : nullptr, clip,
                                       h->stream_ptr()))
    return 1;
  if (h->d2h(u_out, h->s_u, D * B * d.n_out) || h->d2h(du_dx, h->s_dx, D * B * d.n_out * d.nx) ||
      (nup > 0 && h->d2h(du_du_prev, h->s_dup, D * B * d.n_out * nup)))
    return 1;
  return h->sync();
}
