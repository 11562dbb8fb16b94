// dompc_ekf_runtime.cpp - host side of the batched extended Kalman filter behind the C ABI of include/dompc_ipm.h (dompc_ekf_*).
// Generic: sizes come from the per-model code object (dompc_ekf_info_kernel).
// Build flavours as dompc_plant_runtime.cpp: product = part of libdompc_ipm.so (HIP only); test = g++ -DDOMPC_HOST_EMU together with
// dompc_ekf.hip compiled as C++ (tests/_hostemu; never shipped).  dompc_host.h knows which one this is; this file does not.
#include "../../include/dompc_ipm.h"
#include "dompc_host.h"
#include "dompc_ekf_args.h"

// the host twins of the kernels (dompc_ekf.hip)
extern "C" void dompc_ekf_hostemu_info(const void* args);
extern "C" void dompc_ekf_hostemu_run(const void* args);

static thread_local std::string g_ekf_create_error;

struct dompc_ekf : dompc_host::Context {
  dompc_ekf_desc d;
  int32_t cap = 0;
  double *s_x = nullptr, *s_P = nullptr, *s_y = nullptr, *s_u = nullptr, *s_tvp = nullptr, *s_p = nullptr, *s_Q = nullptr, *s_R = nullptr;
  double* s_z = nullptr;
  int32_t *s_st = nullptr, *s_nw = nullptr;
  dompc_host::Kernel fn;
};

extern "C" const char* dompc_ekf_last_error(const dompc_ekf* h) { return h ? h->error.c_str() : g_ekf_create_error.c_str(); }

extern "C" void dompc_ekf_destroy(dompc_ekf* h) {
  if (!h) return;
  h->close();
  delete h;
}

extern "C" int dompc_ekf_create(const dompc_ekf_desc* desc, dompc_ekf** out) {
  if (!desc || !out) { g_ekf_create_error = "null argument"; return 1; }
  dompc_ekf* h = new dompc_ekf();
  h->d = *desc;
  h->device = desc->device;
  auto fail = [&]() { g_ekf_create_error = h->error; dompc_ekf_destroy(h); *out = nullptr; return 1; };
  if (desc->nx <= 0) { h->error = "filter without states"; return fail(); }
  if (!(desc->t_step > 0.0) && !desc->discrete) { h->error = "t_step must be positive"; return fail(); }
  if (desc->nz < 0 || desc->nz > 16) { h->error = "algebraic states: 0 <= nz <= 16"; return fail(); }
  int64_t info[16] = {0};
  char hash[64] = {0};
  if (h->open("extended Kalman filter", desc->code_object_path, nullptr, {{"dompc_ekf_kernel", &h->fn, DOMPC_TWIN(dompc_ekf_hostemu_run)}},
              "code object lacks the filter kernels", "dompc_ekf_info_kernel", DOMPC_TWIN(dompc_ekf_hostemu_info), info, hash))
    return fail();
  const int64_t want[6] = {desc->nx, desc->nu, desc->np, desc->ntvp, desc->ny, desc->discrete ? 1 : 0};
  if (h->check_info("filter ", info, want, 6, 6, sizeof(dompc_ekfk::Args), hash, desc->model_hash)) return fail();
  if (info[7] != desc->nz) { h->error = "filter code object was built for another number of algebraic states"; return fail(); }
  h->d.code_object_path = nullptr; h->d.model_hash = nullptr;
  *out = h;
  return 0;
}

static int step_device(dompc_ekf* h, int32_t B, double* x, double* P, const double* y, const double* u, double* z, const double* tvp,
                       const double* p, const double* Q, const double* R, int32_t shared_mask, int32_t* newton, int32_t* status,
                       void* stream) {
  if (!h) return 1;
  if (B <= 0) return 0;
  const dompc_ekf_desc& d = h->d;
  if (!x || !P || !Q || (d.ny && (!y || !R)) || (d.nu && !u) || (d.ntvp && !tvp) || (d.np && !p)) { h->error = "null pointer"; return 1; }
  dompc_ekfk::Args A;
  memset(&A, 0, sizeof(A));
  A.x = x; A.P = P; A.y = y; A.u = u; A.tvp = tvp; A.p = p; A.Q = Q; A.R = R; A.status = status;
  A.batch = B;
  A.stride_u = (shared_mask & 1) ? 0 : d.nu; A.stride_tvp = (shared_mask & 2) ? 0 : d.ntvp; A.stride_p = (shared_mask & 4) ? 0 : d.np;
  A.stride_q = (shared_mask & 8) ? 0 : d.nx * d.nx; A.stride_r = (shared_mask & 16) ? 0 : d.ny * d.ny;
  A.max_steps = d.max_steps > 0 ? d.max_steps : 200000;
  A.t_step = d.t_step; A.rtol = d.reltol > 0 ? d.reltol : 1e-10; A.atol = d.abstol > 0 ? d.abstol : 1e-10;
  A.z = d.nz ? z : nullptr; A.newton = d.nz ? newton : nullptr;
  A.z_tol = d.z_tol > 0 ? d.z_tol : 1e-10;
  A.z_max_iter = d.z_max_iter > 0 ? d.z_max_iter : 20;
  if (h->set_device()) return 1;
  // one wavefront per workgroup, four filters per wavefront
  return h->run(h->fn, (unsigned)((B + 3) / 4), 64, 0, stream, &A, sizeof(A));
}

extern "C" int dompc_ekf_step_batch_device(dompc_ekf* h, int32_t B, double* x, double* P, const double* y, const double* u,
                                           const double* tvp, const double* p, const double* Q, const double* R,
                                           int32_t shared_mask, int32_t* status, void* stream) {
  return step_device(h, B, x, P, y, u, nullptr, tvp, p, Q, R, shared_mask, nullptr, status, stream);
}

extern "C" int dompc_ekf_step_dae_batch_device(dompc_ekf* h, int32_t B, double* x, double* P, const double* y, const double* u, double* z,
                                               const double* tvp, const double* p, const double* Q, const double* R,
                                               int32_t shared_mask, int32_t* newton, int32_t* status, void* stream) {
  return step_device(h, B, x, P, y, u, z, tvp, p, Q, R, shared_mask, newton, status, stream);
}

static int step_host(dompc_ekf* h, int32_t B, const double* x, const double* P, const double* y, const double* u, const double* z,
                     const double* tvp, const double* p, const double* Q, const double* R, int32_t shared_mask, double* x_out,
                     double* P_out, double* z_out, int32_t* newton, int32_t* status) {
  if (!h) return 1;
  if (B <= 0) return 0;
  const dompc_ekf_desc& d = h->d;
  if (!x || !P || !Q || !x_out || !P_out || (d.ny && (!y || !R)) || (d.nu && !u) || (d.ntvp && !tvp) || (d.np && !p)) { h->error = "null pointer"; return 1; }
  if (h->set_device()) return 1;
  const size_t D = sizeof(double);
  if (h->grow_staging(&h->cap, B, {{(void**)&h->s_x, D * d.nx}, {(void**)&h->s_P, D * d.nx * d.nx}, {(void**)&h->s_y, D * d.ny},
                                   {(void**)&h->s_u, D * d.nu}, {(void**)&h->s_tvp, D * d.ntvp}, {(void**)&h->s_p, D * d.np},
                                   {(void**)&h->s_Q, D * d.nx * d.nx}, {(void**)&h->s_R, D * d.ny * d.ny}, {(void**)&h->s_st, sizeof(int32_t)},
                                   {(void**)&h->s_z, D * d.nz}, {(void**)&h->s_nw, sizeof(int32_t)}}))
    return 1;
  auto rows = [&](int bit) { return (shared_mask & bit) ? (size_t)1 : (size_t)B; };
  // (a null host pointer: an optional array the caller left out)
  auto up = [&](void* dst, const void* src, size_t bytes) { return src ? h->h2d(dst, src, bytes) : 0; };
  auto down = [&](void* dst, const void* src, size_t bytes) { return dst ? h->d2h(dst, src, bytes) : 0; };
  if (up(h->s_x, x, D * B * d.nx) || up(h->s_P, P, D * B * d.nx * d.nx) || up(h->s_y, y, D * B * d.ny) ||
      up(h->s_u, u, D * rows(1) * d.nu) || up(h->s_tvp, tvp, D * rows(2) * d.ntvp) || up(h->s_p, p, D * rows(4) * d.np) ||
      up(h->s_Q, Q, D * rows(8) * d.nx * d.nx) || up(h->s_R, R, D * rows(16) * d.ny * d.ny) || up(h->s_z, z, D * B * d.nz))
    return 1;
  // (the consistent algebraic states take the place of the guess; without a guess the kernel starts from 0 and hands nothing back)
  if (step_device(h, B, h->s_x, h->s_P, h->s_y, h->s_u, z ? h->s_z : nullptr, h->s_tvp, h->s_p, h->s_Q, h->s_R, shared_mask, h->s_nw,
                  h->s_st, h->stream_ptr()))
    return 1;
  if (down(x_out, h->s_x, D * B * d.nx) || down(P_out, h->s_P, D * B * d.nx * d.nx) || down(status, h->s_st, sizeof(int32_t) * (size_t)B) ||
      (d.nz && ((z && down(z_out, h->s_z, D * B * d.nz)) || down(newton, h->s_nw, sizeof(int32_t) * (size_t)B))))
    return 1;
  return h->sync();
}

extern "C" int dompc_ekf_step_batch(dompc_ekf* h, int32_t B, const double* x, const double* P, const double* y, const double* u,
                                    const double* tvp, const double* p, const double* Q, const double* R, int32_t shared_mask,
                                    double* x_out, double* P_out, int32_t* status) {
  return step_host(h, B, x, P, y, u, nullptr, tvp, p, Q, R, shared_mask, x_out, P_out, nullptr, nullptr, status);
}

extern "C" int dompc_ekf_step_dae_batch(dompc_ekf* h, int32_t B, const double* x, const double* P, const double* y, const double* u,
                                        const double* z, const double* tvp, const double* p, const double* Q, const double* R,
                                        int32_t shared_mask, double* x_out, double* P_out, double* z_out, int32_t* newton,
                                        int32_t* status) {
  return step_host(h, B, x, P, y, u, z, tvp, p, Q, R, shared_mask, x_out, P_out, z_out, newton, status);
}
