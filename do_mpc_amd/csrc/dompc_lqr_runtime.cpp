// dompc_lqr_runtime.cpp - host side of the batched LQR design behind the C ABI of include/dompc_ipm.h (dompc_lqr_*).
// Generic: sizes come from the per-design code object (dompc_lqr_info_kernel).
// Build flavours as dompc_ekf_runtime.cpp: product = part of libdompc_ipm.so (HIP only); test = g++ -DDOMPC_HOST_EMU together with
// dompc_lqr.hip compiled as C++ (tests/_hostemu; never shipped).  dompc_host.h knows which one this is; this file does not.
#include "../../include/dompc_ipm.h"
#include "dompc_host.h"
#include "dompc_lqr_args.h"

// the host twins of the kernels (dompc_lqr.hip)
extern "C" void dompc_lqr_hostemu_info(const void* args);
extern "C" void dompc_lqr_hostemu_run(const void* args);

static thread_local std::string g_lqr_create_error;

struct dompc_lqr : dompc_host::Context {
  dompc_lqr_desc d;
  int32_t cap = 0;
  double *s_A = nullptr, *s_B = nullptr, *s_x = nullptr, *s_u = nullptr, *s_tvp = nullptr, *s_p = nullptr, *s_Q = nullptr, *s_R = nullptr,
         *s_Pf = nullptr, *s_K = nullptr, *s_P = nullptr, *s_z = nullptr;
  int32_t* s_st = nullptr;
  dompc_host::Kernel fn;
};

extern "C" const char* dompc_lqr_last_error(const dompc_lqr* h) { return h ? h->error.c_str() : g_lqr_create_error.c_str(); }

extern "C" void dompc_lqr_destroy(dompc_lqr* h) {
  if (!h) return;
  h->close();
  delete h;
}

extern "C" int dompc_lqr_create(const dompc_lqr_desc* desc, dompc_lqr** out) {
  if (!desc || !out) { g_lqr_create_error = "null argument"; return 1; }
  dompc_lqr* h = new dompc_lqr();
  h->d = *desc;
  h->device = desc->device;
  auto fail = [&]() { g_lqr_create_error = h->error; dompc_lqr_destroy(h); *out = nullptr; return 1; };
  if (desc->nx <= 0 || desc->nu <= 0) { h->error = "design without states or without inputs"; return fail(); }
  if (desc->has_model && !desc->discrete && !(desc->t_step > 0.0)) { h->error = "t_step must be positive"; return fail(); }
  if (desc->n_horizon < 0) { h->error = "n_horizon must not be negative"; return fail(); }
  if (desc->nz < 0 || desc->nz > 16 || (desc->nz && !desc->has_model)) { h->error = "algebraic states: 0 <= nz <= 16, with a model"; return fail(); }
  int64_t info[16] = {0};
  char hash[64] = {0};
  if (h->open("LQR design", desc->code_object_path, nullptr, {{"dompc_lqr_kernel", &h->fn, DOMPC_TWIN(dompc_lqr_hostemu_run)}},
              "code object lacks the design kernels", "dompc_lqr_info_kernel", DOMPC_TWIN(dompc_lqr_hostemu_info), info, hash))
    return fail();
  const int64_t want[8] = {desc->nx, desc->nu, desc->n, desc->rate ? 1 : 0, desc->has_model ? 1 : 0,
                           (desc->discrete || !desc->has_model) ? 1 : 0, desc->np, desc->ntvp};
  if (h->check_info("design ", info, want, 8, 8, sizeof(dompc_lqrk::Args), hash, desc->model_hash)) return fail();
  if (info[9] != desc->nz) { h->error = "design code object was built for another number of algebraic states"; return fail(); }
  h->d.code_object_path = nullptr; h->d.model_hash = nullptr;
  *out = h;
  return 0;
}

static int design_device(dompc_lqr* h, int32_t B, double* A, double* Bm, const double* x, const double* u, const double* z,
                         const double* tvp, const double* p, const double* Q, const double* R, const double* Pf, int32_t shared_mask,
                         double* K, double* P, double* z_out, int32_t* status, void* stream) {
  if (!h) return 1;
  if (B <= 0) return 0;
  const dompc_lqr_desc& d = h->d;
  if (!Q || !R || !K || !P || (d.n_horizon > 0 && !Pf) || (!d.has_model && (!A || !Bm)) ||
      (d.has_model && (!x || !u || (d.ntvp && !tvp) || (d.np && !p) || (d.nz && !z)))) { h->error = "null pointer"; return 1; }
  dompc_lqrk::Args G;
  memset(&G, 0, sizeof(G));
  G.A = A; G.B = Bm; G.x = x; G.u = u; G.tvp = tvp; G.p = p; G.Q = Q; G.R = R; G.Pf = Pf; G.K = K; G.P = P; G.status = status;
  G.batch = B;
  G.stride_q = (shared_mask & 1) ? 0 : d.n * d.n; G.stride_r = (shared_mask & 2) ? 0 : d.nu * d.nu;
  G.stride_pf = (shared_mask & 4) ? 0 : d.n * d.n;
  G.stride_tvp = (shared_mask & 8) ? 0 : d.ntvp; G.stride_p = (shared_mask & 16) ? 0 : d.np;
  G.n_horizon = d.n_horizon;
  G.max_iter = d.max_iter > 0 ? d.max_iter : 50;
  G.t_step = d.t_step; G.tol = d.tol > 0 ? d.tol : 1e-13;
  G.z = z; G.z_out = z_out;
  G.z_tol = d.z_tol > 0 ? d.z_tol : 1e-10;
  G.z_max_iter = d.z_max_iter > 0 ? (d.z_max_iter < 127 ? d.z_max_iter : 127) : 20;
  if (h->set_device()) return 1;
  // one wavefront per workgroup, four designs per wavefront
  return h->run(h->fn, (unsigned)((B + 3) / 4), 64, 0, stream, &G, sizeof(G));
}

extern "C" int dompc_lqr_design_batch_device(dompc_lqr* h, int32_t B, double* A, double* Bm, const double* x, const double* u,
                                             const double* tvp, const double* p, const double* Q, const double* R, const double* Pf,
                                             int32_t shared_mask, double* K, double* P, int32_t* status, void* stream) {
  return design_device(h, B, A, Bm, x, u, nullptr, tvp, p, Q, R, Pf, shared_mask, K, P, nullptr, status, stream);
}

extern "C" int dompc_lqr_design_dae_batch_device(dompc_lqr* h, int32_t B, double* A, double* Bm, const double* x, const double* u,
                                                 const double* z, const double* tvp, const double* p, const double* Q, const double* R,
                                                 const double* Pf, int32_t shared_mask, double* K, double* P, double* z_out,
                                                 int32_t* status, void* stream) {
  return design_device(h, B, A, Bm, x, u, z, tvp, p, Q, R, Pf, shared_mask, K, P, z_out, status, stream);
}

static int design_host(dompc_lqr* h, int32_t B, const double* A, const double* Bm, const double* x, const double* u, const double* z,
                       const double* tvp, const double* p, const double* Q, const double* R, const double* Pf, int32_t shared_mask,
                       double* K_out, double* P_out, double* A_out, double* B_out, double* Z_out, int32_t* status) {
  if (!h) return 1;
  if (B <= 0) return 0;
  const dompc_lqr_desc& d = h->d;
  if (!K_out || !P_out) { h->error = "null pointer"; return 1; }
  if (h->set_device()) return 1;
  const size_t D = sizeof(double);
  if (h->grow_staging(&h->cap, B, {{(void**)&h->s_A, D * d.nx * d.nx}, {(void**)&h->s_B, D * d.nx * d.nu}, {(void**)&h->s_x, D * d.nx},
                                   {(void**)&h->s_u, D * d.nu}, {(void**)&h->s_tvp, D * d.ntvp}, {(void**)&h->s_p, D * d.np},
                                   {(void**)&h->s_Q, D * d.n * d.n}, {(void**)&h->s_R, D * d.nu * d.nu}, {(void**)&h->s_Pf, D * d.n * d.n},
                                   {(void**)&h->s_K, D * d.nu * d.n}, {(void**)&h->s_P, D * d.n * d.n}, {(void**)&h->s_st, sizeof(int32_t)},
                                   {(void**)&h->s_z, D * d.nz}}))
    return 1;
  auto rows = [&](int bit) { return (shared_mask & bit) ? (size_t)1 : (size_t)B; };
  // (a null host pointer: an array this kind of design does not read, or an output the caller left out)
  auto up = [&](void* dst, const void* src, size_t bytes) { return src ? h->h2d(dst, src, bytes) : 0; };
  auto down = [&](void* dst, const void* src, size_t bytes) { return dst ? h->d2h(dst, src, bytes) : 0; };
  if (up(h->s_A, A, D * B * d.nx * d.nx) || up(h->s_B, Bm, D * B * d.nx * d.nu) || up(h->s_x, x, D * B * d.nx) || up(h->s_u, u, D * B * d.nu) ||
      up(h->s_tvp, tvp, D * rows(8) * d.ntvp) || up(h->s_p, p, D * rows(16) * d.np) || up(h->s_Q, Q, D * rows(1) * d.n * d.n) ||
      up(h->s_R, R, D * rows(2) * d.nu * d.nu) || up(h->s_Pf, Pf, D * rows(4) * d.n * d.n) || up(h->s_z, z, D * B * d.nz))
    return 1;
  // (the consistent algebraic states take the place of the guess)
  if (design_device(h, B, (A || d.has_model) ? h->s_A : nullptr, (Bm || d.has_model) ? h->s_B : nullptr, x ? h->s_x : nullptr,
                    u ? h->s_u : nullptr, z ? h->s_z : nullptr, tvp ? h->s_tvp : nullptr, p ? h->s_p : nullptr, Q ? h->s_Q : nullptr,
                    R ? h->s_R : nullptr, Pf ? h->s_Pf : nullptr, shared_mask, h->s_K, h->s_P, (z && Z_out) ? h->s_z : nullptr, h->s_st,
                    h->stream_ptr()))
    return 1;
  if (down(K_out, h->s_K, D * B * d.nu * d.n) || down(P_out, h->s_P, D * B * d.n * d.n) ||
      (d.has_model && (down(A_out, h->s_A, D * B * d.nx * d.nx) || down(B_out, h->s_B, D * B * d.nx * d.nu))) ||
      (d.nz && z && down(Z_out, h->s_z, D * B * d.nz)) || down(status, h->s_st, sizeof(int32_t) * (size_t)B))
    return 1;
  return h->sync();
}

extern "C" int dompc_lqr_design_batch(dompc_lqr* h, int32_t B, const double* A, const double* Bm, const double* x, const double* u,
                                      const double* tvp, const double* p, const double* Q, const double* R, const double* Pf,
                                      int32_t shared_mask, double* K_out, double* P_out, double* A_out, double* B_out, int32_t* status) {
  return design_host(h, B, A, Bm, x, u, nullptr, tvp, p, Q, R, Pf, shared_mask, K_out, P_out, A_out, B_out, nullptr, status);
}

extern "C" int dompc_lqr_design_dae_batch(dompc_lqr* h, int32_t B, const double* x, const double* u, const double* z, const double* tvp,
                                          const double* p, const double* Q, const double* R, const double* Pf, int32_t shared_mask,
                                          double* K_out, double* P_out, double* A_out, double* B_out, double* Z_out, int32_t* status) {
  return design_host(h, B, nullptr, nullptr, x, u, z, tvp, p, Q, R, Pf, shared_mask, K_out, P_out, A_out, B_out, Z_out, status);
}
