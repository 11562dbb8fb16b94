// dompc_plant_runtime.cpp - host side of the batched plant integrator behind the C ABI of include/dompc_ipm.h
// (dompc_plant_*).  Generic: sizes come from the per-model code object (dompc_plant_info_kernel).
// Build flavours as dompc_runtime.cpp: product = part of libdompc_ipm.so (HIP only); test = g++ -DDOMPC_HOST_EMU
// together with dompc_plant.hip compiled as C++ (tests/_hostemu; never shipped).  dompc_host.h knows which one this is; this file
// does not.
#include "../../include/dompc_ipm.h"
#include "dompc_host.h"
#include "dompc_plant_args.h"
#include "dompc_ampc_loop_args.h"

// the host twins of the kernels (dompc_plant.hip)
extern "C" void dompc_plant_hostemu_info(const void* args);
extern "C" void dompc_plant_hostemu_run(const void* args);
extern "C" void dompc_plant_hostemu_rollout(const void* args);
extern "C" void dompc_plant_hostemu_loop(const void* args);
extern "C" void dompc_plant_hostemu_tvloop(const void* args);
// ... and of the fused approximate-MPC loop (dompc_ampc_loop.hip): there only in the host library of a (plant, network shape) pair
extern "C" void dompc_ampc_loop_hostemu_info(const void* args) __attribute__((weak));
extern "C" void dompc_ampc_loop_hostemu_run(const void* args) __attribute__((weak));

static_assert(sizeof(dompc_affine_law) == sizeof(dompc_affine::Law), "dompc_affine_law of the C ABI and the kernels' law record");

static thread_local std::string g_plant_create_error;

struct dompc_plant : dompc_host::Context {
  dompc_plant_desc d;
  int32_t cap = 0;
  double *s_x = nullptr, *s_u = nullptr, *s_tvp = nullptr, *s_p = nullptr, *s_w = nullptr, *s_v = nullptr, *s_xn = nullptr, *s_y = nullptr;
  int32_t* s_st = nullptr;
  int32_t nz = 0;                       // algebraic states of the model (from the code object)
  int32_t method = 0, explicit_limit = 4000;
  std::vector<double> z0;               // Newton start of the algebraic states (dompc_plant_set_z0; zeros by default)
  double* z_dev = nullptr;              // [z_cap][nz]: per-sample start values, carried from call to call
  int32_t z_cap = 0, z_alloc = 0;       // rows with valid start values / rows allocated
  bool z_carry_host = false;            // host entry (dompc_plant_step_batch): rows of consecutive calls are the same trajectories (dompc_plant_set_z_carry)
  bool z_reseed_next = false;
  dompc_host::Module module = nullptr;
  dompc_host::Kernel fn, fn_rollout, fn_loop, fn_tvloop;
  // the fused approximate-MPC loop of a pair object, looked up on first use: 0 not looked for yet, 1 there, -1 the object has none
  int ampc_loop_state = 0;
  dompc_host::Kernel fn_ampc_loop;
  int64_t ampc_loop_info[16] = {0};     // what dompc_ampc_loop_info_kernel reported: sizeof(AmpcLoopArgs), then the network's shape
};

extern "C" const char* dompc_plant_last_error(const dompc_plant* h) { return h ? h->error.c_str() : g_plant_create_error.c_str(); }

extern "C" void dompc_plant_destroy(dompc_plant* h) {
  if (!h) return;
  h->close();
  delete h;
}

extern "C" int dompc_plant_create(const dompc_plant_desc* desc, dompc_plant** out) {
  if (!desc || !out) { g_plant_create_error = "null argument"; return 1; }
  dompc_plant* h = new dompc_plant();
  h->d = *desc;
  h->device = desc->device;
  auto fail = [&]() { g_plant_create_error = h->error; dompc_plant_destroy(h); *out = nullptr; return 1; };
  if (desc->nx <= 0) { h->error = "plant without states"; return fail(); }
  if (!(desc->t_step > 0.0) && !desc->discrete) { h->error = "t_step must be positive"; return fail(); }
  int64_t info[16] = {0};
  char hash[64] = {0};
  if (h->open("plant integrator", desc->code_object_path, &h->module, {{"dompc_plant_kernel", &h->fn, DOMPC_TWIN(dompc_plant_hostemu_run)}},
              "code object lacks the plant kernels", "dompc_plant_info_kernel", DOMPC_TWIN(dompc_plant_hostemu_info), info, hash))
    return fail();
  const int64_t want[8] = {desc->nx, desc->nu, desc->np, desc->ntvp, desc->nw, desc->nv, desc->ny, desc->discrete ? 1 : 0};
  if (h->check_info("plant ", info, want, 8, 8, sizeof(dompc_plantk::Args), hash, desc->model_hash)) return fail();
  if (info[9] == 0) {                    // (the rollout entry exists for plants without algebraic states only)
    if (info[10] != (int64_t)sizeof(dompc_plantk::RolloutArgs)) { h->error = "plant rollout argument layout mismatch between runtime and code object"; return fail(); }
    if (!h->find(h->module, {"dompc_plant_rollout_kernel", &h->fn_rollout, DOMPC_TWIN(dompc_plant_hostemu_rollout)})) { h->error = "code object lacks the plant kernels"; return fail(); }
  }
  // the general rollout: every plant has it
  if (info[11] != (int64_t)sizeof(dompc_plantk::LoopArgs)) { h->error = "plant loop argument layout mismatch between runtime and code object"; return fail(); }
  if (!h->find(h->module, {"dompc_plant_loop_kernel", &h->fn_loop, DOMPC_TWIN(dompc_plant_hostemu_loop)})) { h->error = "code object lacks the plant kernels"; return fail(); }
  if (info[12] != (int64_t)sizeof(dompc_plantk::TvLoopArgs)) { h->error = "plant loop argument layout mismatch between runtime and code object (dompc_plant_tvloop_kernel)"; return fail(); }
  if (!h->find(h->module, {"dompc_plant_tvloop_kernel", &h->fn_tvloop, DOMPC_TWIN(dompc_plant_hostemu_tvloop)})) { h->error = "code object lacks the plant kernels"; return fail(); }
  h->d.code_object_path = nullptr; h->d.model_hash = nullptr;
  h->nz = (int32_t)info[9];
  h->z0.assign((size_t)(h->nz > 0 ? h->nz : 0), 0.0);
  *out = h;
  return 0;
}

extern "C" int dompc_plant_set_method(dompc_plant* h, int32_t method, int32_t explicit_limit) {
  if (!h) return 1;
  if (method < 0 || method > 2) { h->error = "method must be 0 (explicit, implicit for stiff samples), 1 (explicit) or 2 (implicit)"; return 1; }
  h->method = method;
  if (explicit_limit > 0) h->explicit_limit = explicit_limit;
  return 0;
}

extern "C" int32_t dompc_plant_num_alg_states(const dompc_plant* h) { return h ? h->nz : 0; }

extern "C" int dompc_plant_set_z0(dompc_plant* h, const double* z0) {
  if (!h) return 1;
  for (int i = 0; i < h->nz; ++i) h->z0[(size_t)i] = z0 ? z0[i] : 0.0;
  h->z_cap = 0;                          // (the per-sample values are re-seeded by the next call)
  return 0;
}

// per-sample start values of the algebraic states for B samples: seeded with z0 when the buffer is (re)created, when it grows, and on
// request (`reseed`).  Row b of the buffer belongs to sample b of the CALLS: carried values only make sense when the rows of consecutive
// calls are the same trajectories (the device closed loops, Simulator.make_step); a host call on unrelated samples reseeds.
static int ensure_z(dompc_plant* h, int32_t B, bool reseed) {
  if (h->nz <= 0) return 0;
  if (B <= h->z_cap && !reseed) return 0;
  if (B > h->z_alloc) {
    h->release(h->z_dev);
    h->z_dev = nullptr;
    h->z_cap = 0; h->z_alloc = 0;
    if (h->alloc((void**)&h->z_dev, sizeof(double) * (size_t)B * h->nz)) return 1;
    h->z_alloc = B;
  }
  std::vector<double> seed((size_t)B * h->nz);
  for (int32_t b = 0; b < B; ++b)
    for (int i = 0; i < h->nz; ++i) seed[(size_t)b * h->nz + i] = h->z0[(size_t)i];
  if (h->h2d_now(h->z_dev, seed.data(), seed.size() * sizeof(double))) return 1;      // (`seed` goes away on return)
  if (B > h->z_cap) h->z_cap = B;        // a reseed of the first B rows leaves the carried rows behind them alone
  return 0;
}

extern "C" int dompc_plant_set_z_carry(dompc_plant* h, int32_t on) {
  if (!h) return 1;
  h->z_carry_host = on != 0;
  return 0;
}

static int launch_plant(dompc_plant* h, dompc_plantk::Args& A, void* stream) {
  return h->run(h->fn, (A.batch + 63) / 64, 64, 0, stream, &A, sizeof(A));
}

static void fill_args(const dompc_plant* h, dompc_plantk::Args& A, int32_t B, int32_t shared_mask) {
  const dompc_plant_desc& d = h->d;
  A.batch = B;
  A.stride_u = (shared_mask & 1) ? 0 : d.nu; A.stride_tvp = (shared_mask & 2) ? 0 : d.ntvp; A.stride_p = (shared_mask & 4) ? 0 : d.np;
  A.stride_w = (shared_mask & 8) ? 0 : d.nw; A.stride_v = (shared_mask & 16) ? 0 : d.nv;
  A.max_steps = d.max_steps > 0 ? d.max_steps : 200000; A.pad = 0;
  A.method = h->method; A.explicit_limit = h->explicit_limit;
  A.z_guess = (h->nz > 0 && B <= h->z_cap) ? h->z_dev : nullptr;
  A.t_step = d.t_step; A.rtol = d.reltol > 0 ? d.reltol : 1e-10; A.atol = d.abstol > 0 ? d.abstol : 1e-10;
}

extern "C" int dompc_plant_step_batch_device(dompc_plant* h, int32_t B, const double* x, const double* u, const double* tvp,
                                             const double* p, const double* w, const double* v, int32_t shared_mask,
                                             double* x_next, double* y, int32_t* status, void* stream) {
  if (!h) return 1;
  if (B <= 0) return 0;
  const dompc_plant_desc& d = h->d;
  if (!x || !x_next || (d.nu && !u) || (d.ntvp && !tvp) || (d.np && !p)) { h->error = "null pointer"; return 1; }
  if (h->set_device()) return 1;
  if (ensure_z(h, B, h->z_reseed_next)) return 1;
  h->z_reseed_next = false;
  dompc_plantk::Args A;
  memset(&A, 0, sizeof(A));
  A.x = x; A.u = u; A.tvp = tvp; A.p = p; A.w = w; A.v = v; A.x_next = x_next; A.y = y; A.status = status;
  fill_args(h, A, B, shared_mask);
  return launch_plant(h, A, stream);
}

extern "C" int dompc_plant_step_batch(dompc_plant* h, int32_t B, const double* x, const double* u, const double* tvp,
                                      const double* p, const double* w, const double* v, int32_t shared_mask,
                                      double* x_next, double* y, int32_t* status) {
  if (!h) return 1;
  if (B <= 0) return 0;
  const dompc_plant_desc& d = h->d;
  if (!x || !x_next || (d.nu && !u) || (d.ntvp && !tvp) || (d.np && !p)) { h->error = "null pointer"; return 1; }
  if (h->set_device()) return 1;
  const size_t D = sizeof(double);
  if (h->grow_staging(&h->cap, B, {{(void**)&h->s_x, D * d.nx}, {(void**)&h->s_u, D * d.nu}, {(void**)&h->s_tvp, D * d.ntvp},
                                   {(void**)&h->s_p, D * d.np}, {(void**)&h->s_w, D * d.nw}, {(void**)&h->s_v, D * d.nv},
                                   {(void**)&h->s_xn, D * d.nx}, {(void**)&h->s_y, D * d.ny}, {(void**)&h->s_st, sizeof(int32_t)}}))
    return 1;
  auto rows = [&](int bit) { return (shared_mask & bit) ? (size_t)1 : (size_t)B; };
  // (a null host pointer: an optional array the caller left out)
  auto up = [&](void* dst, const void* src, size_t bytes) { return src ? h->h2d(dst, src, bytes) : 0; };
  auto down = [&](void* dst, const void* src, size_t bytes) { return dst ? h->d2h(dst, src, bytes) : 0; };
  if (up(h->s_x, x, D * B * d.nx) || up(h->s_u, u, D * rows(1) * d.nu) || up(h->s_tvp, tvp, D * rows(2) * d.ntvp) ||
      up(h->s_p, p, D * rows(4) * d.np) || up(h->s_w, w, D * rows(8) * d.nw) || up(h->s_v, v, D * rows(16) * d.nv))
    return 1;
  h->z_reseed_next = !h->z_carry_host;       // unrelated samples per call unless the caller says the rows are the same trajectories
  if (dompc_plant_step_batch_device(h, B, h->s_x, h->s_u, h->s_tvp, h->s_p, w ? h->s_w : nullptr, v ? h->s_v : nullptr, shared_mask,
                                    h->s_xn, y ? h->s_y : nullptr, h->s_st, h->stream_ptr()))
    return 1;
  if (down(x_next, h->s_xn, D * B * d.nx) || down(y, h->s_y, D * B * d.ny) || down(status, h->s_st, sizeof(int32_t) * (size_t)B)) return 1;
  return h->sync();
}

extern "C" int dompc_plant_rollout_affine_device(dompc_plant* h, int32_t B, int32_t K, const dompc_affine_law* law, double* X_traj,
                                                 double* U_traj, const double* tvp_rows, const double* p_rows, int32_t* plant_status,
                                                 int32_t* law_status, void* stream) {
  if (!h) return 1;
  if (B <= 0 || K <= 0) return 0;
  const dompc_plant_desc& d = h->d;
  if (h->nz > 0) {
    h->error = "dompc_plant_rollout_affine_device: plants with algebraic states are not served by the rollout (use dompc_plant_step_batch_device per step)";
    return 1;
  }
  if (d.nu <= 0) { h->error = "dompc_plant_rollout_affine_device: the plant has no inputs"; return 1; }
  if (!law || !X_traj || !U_traj || (d.ntvp && !tvp_rows) || (d.np && !p_rows)) { h->error = "null pointer"; return 1; }
  if (!law->x_ref || !law->u_ref || !law->M || !law->x_scale || (law->clip && (!law->lb || !law->ub)) || law->ld < B) {
    h->error = "dompc_plant_rollout_affine_device: incomplete law record (x_ref, u_ref, M, x_scale, with clip lb and ub; ld >= B)";
    return 1;
  }
  if (h->set_device()) return 1;
  dompc_plantk::RolloutArgs R;
  memset(&R, 0, sizeof(R));
  fill_args(h, R.plant, B, 2 | 4 | 8 | 16);
  R.plant.z_guess = nullptr;
  memcpy(&R.law, law, sizeof(R.law));
  R.X_traj = X_traj; R.U_traj = U_traj; R.tvp_rows = tvp_rows; R.p_rows = p_rows;
  R.plant_status = plant_status; R.law_status = law_status; R.K = K;
  return h->run(h->fn_rollout, (unsigned)((B + 63) / 64), 64, 0, stream, &R, sizeof(R));
}

extern "C" int dompc_plant_rollout_device(dompc_plant* h, int32_t B, int32_t K, const dompc_plant_rollout_desc* r, void* stream) {
  if (!h) return 1;
  if (B <= 0 || K <= 0) return 0;
  const dompc_plant_desc& d = h->d;
  const char* me = "dompc_plant_rollout_device: ";
  auto refuse = [&](const char* what) { h->error = std::string(me) + what; return 1; };
  if (!r) return refuse("null description");
  if (!r->X_traj) return refuse("X_traj is null");
  if (d.nu && !r->U_traj) return refuse("U_traj is null");
  if (d.np && !r->p_rows && !r->p_loops) return refuse("the plant has parameters: p_rows or p_loops is needed");
  if (r->p_rows && r->p_loops) return refuse("p_rows and p_loops are both given (one of them)");
  if (d.ntvp && !r->tvp_rows) return refuse("the plant has time-varying parameters: tvp_rows is needed");
  const dompc_affine_law* law = r->law;
  if (law && d.nu <= 0) return refuse("a law on a plant without inputs");
  if (law && (!law->x_ref || !law->u_ref || !law->M || !law->x_scale || (law->clip && (!law->lb || !law->ub)) || law->ld < B))
    return refuse("incomplete law record (x_ref, u_ref, M, x_scale, with clip lb and ub; ld >= B)");
  if (r->G && !law) return refuse("G without a law");
  if (r->G && !r->up_ref) return refuse("G without up_ref");
  if (r->G && !r->U_prev0) return refuse("G without U_prev0");
  if (r->law_step < 0) return refuse("law_step is negative");
  if (r->law_step > 0 && !law) return refuse("law_step without a law");
  if (r->law_step > 0 && (r->G || r->up_ref)) return refuse("law_step with G / up_ref (the time-varying input-rate law is not built)");
  if (r->law_step > 0 && r->law_step < B) return refuse("law_step < B");
  if (r->Z_traj && h->nz <= 0) return refuse("Z_traj on a plant without algebraic states");
  if (h->set_device()) return 1;
  // the per-loop Newton starts of the algebraic states: as dompc_plant_step_batch_device treats them, or seeded from z0 first
  if (ensure_z(h, B, r->reseed_z != 0 || h->z_reseed_next)) return 1;
  h->z_reseed_next = false;
  dompc_plantk::LoopArgs R;
  memset(&R, 0, sizeof(R));
  fill_args(h, R.plant, B, 0);
  if (law) { memcpy(&R.law, law, sizeof(R.law)); R.has_law = 1; }
  R.G = law ? r->G : nullptr; R.up_ref = r->up_ref; R.U_prev0 = r->U_prev0;
  R.X_traj = r->X_traj; R.U_traj = r->U_traj; R.W_traj = r->W_traj; R.V_traj = r->V_traj; R.Y_traj = r->Y_traj; R.Z_traj = r->Z_traj;
  R.tvp_rows = r->tvp_rows; R.p_rows = r->p_rows; R.p_loops = r->p_loops;
  R.plant_status = r->plant_status; R.law_status = r->law_status; R.K = K;
  if (r->law_step > 0) {                 // a law record per step: an entry of its own, the one above is what it was
    dompc_plantk::TvLoopArgs T;
    memset(&T, 0, sizeof(T));
    T.loop = R; T.law_step = r->law_step;
    return h->run(h->fn_tvloop, (unsigned)((B + 63) / 64), 64, 0, stream, &T, sizeof(T));
  }
  return h->run(h->fn_loop, (unsigned)((B + 63) / 64), 64, 0, stream, &R, sizeof(R));
}

extern "C" int dompc_plant_z_guess_device(dompc_plant* h, int32_t B, int32_t reseed, double** z_guess) {
  if (!h) return 1;
  if (!z_guess) { h->error = "null pointer"; return 1; }
  *z_guess = nullptr;
  if (h->nz <= 0 || B <= 0) return 0;
  if (h->set_device()) return 1;
  if (ensure_z(h, B, reseed != 0 || h->z_reseed_next)) return 1;
  h->z_reseed_next = false;
  *z_guess = h->z_dev;
  return 0;
}

// the loop kernel of a pair object and what its info kernel reports, looked up once per handle
static int find_ampc_loop(dompc_plant* h) {
  if (h->ampc_loop_state != 0) return h->ampc_loop_state > 0 ? 0 : 1;
  h->ampc_loop_state = -1;
  dompc_host::Kernel k_info;
  h->find(h->module, {"dompc_ampc_loop_kernel", &h->fn_ampc_loop, DOMPC_TWIN(dompc_ampc_loop_hostemu_run)});
  h->find(h->module, {"dompc_ampc_loop_info_kernel", &k_info, DOMPC_TWIN(dompc_ampc_loop_hostemu_info)});
  if (!h->fn_ampc_loop || !k_info) return 1;
  char hash[64] = {0};
  if (h->query(k_info, "dompc_ampc_loop_info_kernel", h->ampc_loop_info, hash)) return 1;
  h->ampc_loop_state = 1;
  return 0;
}

extern "C" int dompc_plant_ampc_loop_device(dompc_plant* h, int32_t B, int32_t K, const dompc_plant_ampc_loop_desc* r, void* stream) {
  if (!h) return 1;
  if (B <= 0 || K <= 0) return 0;
  const dompc_plant_desc& d = h->d;
  const char* me = "dompc_plant_ampc_loop_device: ";
  auto refuse = [&](const char* what) { h->error = std::string(me) + what; return 1; };
  if (!r) return refuse("null description");
  if (!r->X_traj) return refuse("X_traj is null");
  if (!r->U_traj) return refuse("U_traj is null");
  if (d.np && !r->p_rows && !r->p_loops) return refuse("the plant has parameters: p_rows or p_loops is needed");
  if (r->p_rows && r->p_loops) return refuse("p_rows and p_loops are both given (one of them)");
  if (d.ntvp && !r->tvp_rows) return refuse("the plant has time-varying parameters: tvp_rows is needed");
  if (r->Z_traj && h->nz <= 0) return refuse("Z_traj on a plant without algebraic states");
  if (r->n_out != d.nu) return refuse("the network's n_out differs from the plant's nu");
  if (r->n_in != d.nx && r->n_in != d.nx + d.nu) return refuse("the network's n_in is neither the plant's nx nor nx + nu");
  if (r->n_in > d.nx && !r->U_prev0) return refuse("the network has an rterm (n_in = nx + nu): U_prev0 is needed");
  if (!r->w || !r->par) return refuse("the network's weights (w, par) are null");
  if (h->set_device()) return 1;
  if (find_ampc_loop(h)) {
    if (h->ampc_loop_state < 0 && !h->fn_ampc_loop) return refuse("the handle's code object has no loop kernel (dompc_ampc_loop_kernel: create the handle on the object of a (plant, network) pair)");
    return refuse("dompc_ampc_loop_info_kernel failed");
  }
  const int64_t* info = h->ampc_loop_info;
  if (info[0] != (int64_t)sizeof(dompc_ampc_loopk::AmpcLoopArgs)) return refuse("loop argument layout mismatch between runtime and code object");
  const int64_t want[7] = {r->n_in, r->n_out, r->n_hidden_layers, r->n_neurons, r->act, r->out_act, r->scaling ? 1 : 0};
  for (int i = 0; i < 7; ++i)
    if (info[1 + i] != want[i]) return refuse("the code object was built for another network shape");
  // the per-loop Newton starts of the algebraic states: the caller's (another handle's, dompc_plant_z_guess_device) or this handle's own
  double* z = nullptr;
  if (h->nz > 0) {
    if (r->z_guess) z = r->z_guess;
    else {
      if (ensure_z(h, B, r->reseed_z != 0 || h->z_reseed_next)) return 1;
      h->z_reseed_next = false;
      z = h->z_dev;
    }
  }
  dompc_ampc_loopk::AmpcLoopArgs R;
  memset(&R, 0, sizeof(R));
  dompc_plantk::LoopArgs& L = R.loop;
  fill_args(h, L.plant, B, 0);
  L.plant.z_guess = z;
  L.U_prev0 = r->n_in > d.nx ? r->U_prev0 : nullptr;
  L.X_traj = r->X_traj; L.U_traj = r->U_traj; L.W_traj = r->W_traj; L.V_traj = r->V_traj; L.Y_traj = r->Y_traj; L.Z_traj = r->Z_traj;
  L.tvp_rows = r->tvp_rows; L.p_rows = r->p_rows; L.p_loops = r->p_loops;
  L.plant_status = r->plant_status; L.K = K; L.has_law = 0;
  R.w = r->w; R.par = r->par; R.nx = d.nx; R.clip = r->clip ? 1 : 0;
  // one wavefront per workgroup, 64 loops per wavefront
  return h->run(h->fn_ampc_loop, (unsigned)(((int64_t)B + 63) / 64), 64, 0, stream, &R, sizeof(R));
}
