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
extern "C" void dompc_lqr_hostemu_pairs(const void* args);
extern "C" void dompc_lqr_hostemu_tv(const void* args);

static thread_local std::string g_lqr_create_error;

struct dompc_lqr : dompc_host::Context {
  dompc_lqr_desc d;
  int32_t cap = 0;
  double *s_A = nullptr, *s_B = nullptr, *s_x = nullptr, *s_u = nullptr, *s_tvp = nullptr, *s_p = nullptr, *s_Q = nullptr, *s_R = nullptr,
         *s_Pf = nullptr, *s_K = nullptr, *s_P = nullptr, *s_z = nullptr;
  int32_t* s_st = nullptr;
  dompc_host::Kernel fn, fn_pairs, fn_tv;
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
  if (h->open("LQR design", desc->code_object_path, nullptr, {{"dompc_lqr_kernel", &h->fn, DOMPC_TWIN(dompc_lqr_hostemu_run)},
               {"dompc_lqr_pairs_kernel", &h->fn_pairs, DOMPC_TWIN(dompc_lqr_hostemu_pairs)},
               {"dompc_lqr_tv_kernel", &h->fn_tv, DOMPC_TWIN(dompc_lqr_hostemu_tv)}},
              "code object lacks the design kernels", "dompc_lqr_info_kernel", DOMPC_TWIN(dompc_lqr_hostemu_info), info, hash))
    return fail();
  const int64_t want[8] = {desc->nx, desc->nu, desc->n, desc->rate ? 1 : 0, desc->has_model ? 1 : 0,
                           (desc->discrete || !desc->has_model) ? 1 : 0, desc->np, desc->ntvp};
  if (h->check_info("design ", info, want, 8, 8, sizeof(dompc_lqrk::Args), hash, desc->model_hash)) return fail();
  if (info[10] != (int64_t)sizeof(dompc_lqrk::PairsArgs)) { h->error = "design argument layout mismatch between runtime and code object (dompc_lqr_pairs_kernel)"; return fail(); }
  if (info[11] != (int64_t)sizeof(dompc_lqrk::TvArgs)) { h->error = "design argument layout mismatch between runtime and code object (dompc_lqr_tv_kernel)"; return fail(); }
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

// ---- time-varying LQR along trajectories: the pairs of the B x K knots (one launch), then the backward recursion (one launch)
extern "C" int dompc_lqr_pairs_device(dompc_lqr* h, int32_t B, int32_t K, const double* x_traj, const double* u_traj, const double* z0,
                                      const double* tvp, const double* p, int32_t shared_mask, double* A_traj, double* B_traj,
                                      double* z_out, int32_t* status, void* stream) {
  if (!h) return 1;
  const dompc_lqr_desc& d = h->d;
  if (!d.has_model) { h->error = "pairs: the code object has no model (designs of this handle read their pairs)"; return 1; }
  if (B <= 0) return 0;
  if (K <= 0) {
    if (A_traj || B_traj || z_out || status) { h->error = "pairs: K <= 0 with outputs"; return 1; }
    return 0;
  }
  if (!x_traj || !u_traj || !A_traj || !B_traj) { h->error = "pairs: null trajectory"; return 1; }
  if ((d.ntvp && !tvp) || (d.np && !p) || (d.nz && !z0)) { h->error = "pairs: null pointer"; return 1; }
  if ((int64_t)B * K > INT32_MAX / 256) { h->error = "pairs: too many knots for one launch"; return 1; }
  dompc_lqrk::PairsArgs G;
  memset(&G, 0, sizeof(G));
  G.x = x_traj; G.u = u_traj; G.tvp = tvp; G.p = p; G.z = z0; G.A = A_traj; G.B = B_traj; G.z_out = z_out; G.status = status;
  G.batch = B; G.steps = K;
  G.stride_tvp_step = (shared_mask & 8) ? d.ntvp : (int64_t)B * d.ntvp;
  G.stride_tvp_loop = (shared_mask & 8) ? 0 : d.ntvp;
  G.stride_p = (shared_mask & 16) ? 0 : d.np;
  G.t_step = d.t_step;
  G.z_tol = d.z_tol > 0 ? d.z_tol : 1e-10;
  G.z_max_iter = d.z_max_iter > 0 ? (d.z_max_iter < 127 ? d.z_max_iter : 127) : 20;
  if (h->set_device()) return 1;
  return h->run(h->fn_pairs, (unsigned)(((int64_t)B * K + 3) / 4), 64, 0, stream, &G, sizeof(G));
}

extern "C" int dompc_lqr_tv_device(dompc_lqr* h, int32_t B, int32_t K, const double* A_traj, const double* B_traj,
                                   const int32_t* pair_status, const double* Q, const double* R, const double* Pf, int32_t shared_mask,
                                   double* K_traj, double* law_M, int32_t ld, double* P_traj, double* P0, int32_t* status, void* stream) {
  if (!h) return 1;
  const dompc_lqr_desc& d = h->d;
  if (law_M && d.rate) { h->error = "tv: the law layout is written in standard mode only, not in inputRatePenalization mode"; return 1; }
  if (B <= 0) return 0;
  if (K <= 0) {
    if (K_traj || law_M || P_traj || P0 || status) { h->error = "tv: K <= 0 with outputs"; return 1; }
    return 0;
  }
  if (!A_traj || !B_traj) { h->error = "tv: null trajectory"; return 1; }
  if (!Q || !R || !Pf || !P0) { h->error = "tv: null pointer"; return 1; }
  if (law_M && ld < B) { h->error = "tv: ld < B"; return 1; }
  if ((int64_t)B * (K + 1) > INT32_MAX / 256) { h->error = "tv: too many knots for one launch"; return 1; }
  dompc_lqrk::TvArgs G;
  memset(&G, 0, sizeof(G));
  G.A = A_traj; G.B = B_traj; G.pair_status = pair_status; G.Q = Q; G.R = R; G.Pf = Pf; G.K = K_traj; G.M = law_M; G.P = P_traj; G.P0 = P0;
  G.status = status;
  G.batch = B; G.steps = K; G.ld = ld;
  G.stride_q = (shared_mask & 1) ? 0 : d.n * d.n; G.stride_r = (shared_mask & 2) ? 0 : d.nu * d.nu;
  G.stride_pf = (shared_mask & 4) ? 0 : d.n * d.n;
  if (h->set_device()) return 1;
  return h->run(h->fn_tv, (unsigned)((B + 3) / 4), 64, 0, stream, &G, sizeof(G));
}

// host buffers: with a model the knots (x_traj, u_traj, z0, tvp, p) -> pairs -> recursion; without one the pairs (A_traj, B_traj)
// themselves.  Outputs that are not wanted may be null (K_out and P0_out may not).
extern "C" int dompc_lqr_tv(dompc_lqr* h, int32_t B, int32_t K, const double* A_traj, const double* B_traj, const double* x_traj,
                            const double* u_traj, const double* z0, const double* tvp, const double* p, const double* Q, const double* R,
                            const double* Pf, int32_t shared_mask, double* K_out, double* P0_out, double* P_out, double* A_out,
                            double* B_out, double* Z_out, int32_t* pair_status, int32_t* status) {
  if (!h) return 1;
  if (B <= 0) return 0;
  const dompc_lqr_desc& d = h->d;
  if (K <= 0) { h->error = "tv: K <= 0 with outputs"; return 1; }
  if (!K_out || !P0_out || !Q || !R || !Pf) { h->error = "tv: null pointer"; return 1; }
  if (d.has_model ? (!x_traj || !u_traj) : (!A_traj || !B_traj)) { h->error = "tv: null trajectory"; return 1; }
  if (d.has_model && ((d.ntvp && !tvp) || (d.np && !p))) { h->error = "tv: null pointer"; return 1; }
  if (h->set_device()) return 1;
  const size_t D = sizeof(double), KB = (size_t)K * B, n = d.n, nx = d.nx, nu = d.nu;
  auto rows = [&](int bit) { return (shared_mask & bit) ? (size_t)1 : (size_t)B; };
  std::vector<void*> mine;
  auto take = [&](void** q, size_t bytes) { if (h->alloc(q, bytes)) return 1; mine.push_back(*q); return 0; };
  auto done = [&](int rc) { for (void* q : mine) h->release(q); return rc; };
  double *dA = nullptr, *dB = nullptr, *dx = nullptr, *du = nullptr, *dz = nullptr, *dtvp = nullptr, *dp = nullptr, *dQ = nullptr, *dR = nullptr,
         *dPf = nullptr, *dK = nullptr, *dP = nullptr, *dP0 = nullptr;
  int32_t *dps = nullptr, *dst = nullptr;
  if (take((void**)&dA, D * KB * nx * nx) || take((void**)&dB, D * KB * nx * nu) || take((void**)&dQ, D * rows(1) * n * n) ||
      take((void**)&dR, D * rows(2) * nu * nu) || take((void**)&dPf, D * rows(4) * n * n) || take((void**)&dK, D * KB * nu * n) ||
      take((void**)&dP0, D * B * n * n) || take((void**)&dst, sizeof(int32_t) * B) || (P_out && take((void**)&dP, D * (KB + B) * n * n)))
    return done(1);
  if (h->h2d(dQ, Q, D * rows(1) * n * n) || h->h2d(dR, R, D * rows(2) * nu * nu) || h->h2d(dPf, Pf, D * rows(4) * n * n)) return done(1);
  if (d.has_model) {
    const size_t tvp_rows = (shared_mask & 8) ? (size_t)K : KB;
    if (take((void**)&dx, D * KB * nx) || take((void**)&du, D * KB * nu) || take((void**)&dz, D * KB * d.nz) ||
        take((void**)&dtvp, D * tvp_rows * d.ntvp) || take((void**)&dp, D * rows(16) * d.np) || take((void**)&dps, sizeof(int32_t) * KB))
      return done(1);
    if (h->h2d(dx, x_traj, D * KB * nx) || h->h2d(du, u_traj, D * KB * nu) || (d.ntvp && h->h2d(dtvp, tvp, D * tvp_rows * d.ntvp)) ||
        (d.np && h->h2d(dp, p, D * rows(16) * d.np)))
      return done(1);
    if (d.nz && (z0 ? h->h2d(dz, z0, D * KB * d.nz) : h->fill(dz, 0, D * KB * d.nz, h->stream_ptr()))) return done(1);
    if (dompc_lqr_pairs_device(h, B, K, dx, du, dz, dtvp, dp, shared_mask, dA, dB, (d.nz && Z_out) ? dz : nullptr, dps, h->stream_ptr()))
      return done(1);
  } else if (h->h2d(dA, A_traj, D * KB * nx * nx) || h->h2d(dB, B_traj, D * KB * nx * nu)) {
    return done(1);
  }
  if (dompc_lqr_tv_device(h, B, K, dA, dB, dps, dQ, dR, dPf, shared_mask, dK, nullptr, 0, dP, dP0, dst, h->stream_ptr())) return done(1);
  auto down = [&](void* dst_, const void* src, size_t bytes) { return dst_ ? h->d2h(dst_, src, bytes) : 0; };
  if (down(K_out, dK, D * KB * nu * n) || down(P0_out, dP0, D * B * n * n) || down(P_out, dP, D * (KB + B) * n * n) ||
      down(status, dst, sizeof(int32_t) * B) ||
      (d.has_model && (down(A_out, dA, D * KB * nx * nx) || down(B_out, dB, D * KB * nx * nu) || down(pair_status, dps, sizeof(int32_t) * KB) ||
                       (d.nz && down(Z_out, dz, D * KB * d.nz)))))
    return done(1);
  return done(h->sync());
}
