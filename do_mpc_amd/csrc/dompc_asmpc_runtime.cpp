// dompc_asmpc_runtime.cpp - host side of the sensitivity-based MPC law behind the C ABI of include/dompc_ipm.h (dompc_asmpc_*).
// Generic: sizes come from the per-shape code object (dompc_asmpc_info_kernel); the law record, the bounds and the scaling are data
// of the handle.  Build flavours as dompc_ampc_runtime.cpp: product = part of libdompc_ipm.so (HIP only); test = g++ -DDOMPC_HOST_EMU
// together with dompc_asmpc.hip compiled as C++ (tests/_hostemu; never shipped).  dompc_host.h knows which one this is; this file does not.
#include "../../include/dompc_ipm.h"
#include "dompc_host.h"
#include "dompc_asmpc_args.h"

// the host twins of the kernels (dompc_asmpc.hip)
extern "C" void dompc_asmpc_hostemu_info(const void* args);
extern "C" void dompc_asmpc_hostemu_prepare(const void* args);
extern "C" void dompc_asmpc_hostemu_step(const void* args);
extern "C" void dompc_asmpc_hostemu_select_count(const void* args);
extern "C" void dompc_asmpc_hostemu_select_write(const void* args);

static_assert(sizeof(dompc_affine_law) == sizeof(dompc_affine::Law), "dompc_affine_law of the C ABI and the kernels' law record");

static thread_local std::string g_asmpc_create_error;

struct dompc_asmpc : dompc_host::Context {
  dompc_asmpc_desc d;
  double *lb = nullptr, *ub = nullptr, *xs = nullptr;          // [nu], [nu], [nx]
  int32_t clip = 1;
  double max_dx = INFINITY;
  // the law record: [nx][ld], [nu][ld], [nu][nx][ld], [ld] with ld = law_B
  double *x_ref = nullptr, *u_ref = nullptr, *M = nullptr;
  int32_t* flags = nullptr;
  int32_t law_cap = 0, law_B = 0;
  // staging of the host entries
  int32_t cap = 0;
  double *s_x = nullptr, *s_u = nullptr, *s_J = nullptr, *s_G = nullptr;
  int32_t *s_ok = nullptr, *s_st = nullptr, *s_slot = nullptr;
  // per-workgroup counts of the selection: one entry per SELECT_SPAN loops
  int32_t sel_cap = 0;
  int32_t* sel_count = nullptr;
  dompc_host::Kernel fn_prep, fn_step, fn_sel_count, fn_sel_write;
  int grow_host_staging(int32_t B) {
    const size_t D = sizeof(double);
    return grow_staging(&cap, B, {{(void**)&s_x, D * d.nx}, {(void**)&s_u, D * d.nu}, {(void**)&s_J, D * d.nx * d.nu},
                                  {(void**)&s_G, D * d.nu * d.nu}, {(void**)&s_ok, sizeof(int32_t)}, {(void**)&s_st, sizeof(int32_t)},
                                  {(void**)&s_slot, sizeof(int32_t)}});
  }
};

static const int32_t MAX_BATCH = 1 << 20;      // (index arithmetic of the law preparation: 16 * 64 * ld stays an int)

extern "C" const char* dompc_asmpc_last_error(const dompc_asmpc* h) { return h ? h->error.c_str() : g_asmpc_create_error.c_str(); }

extern "C" void dompc_asmpc_destroy(dompc_asmpc* h) {
  if (!h) return;
  h->close();
  delete h;
}

extern "C" int dompc_asmpc_create(const dompc_asmpc_desc* desc, dompc_asmpc** out) {
  if (!desc || !out) { g_asmpc_create_error = "null argument"; return 1; }
  dompc_asmpc* h = new dompc_asmpc();
  h->d = *desc;
  h->device = desc->device;
  auto fail = [&]() { g_asmpc_create_error = h->error; dompc_asmpc_destroy(h); *out = nullptr; return 1; };
  if (desc->nx <= 0 || desc->nu <= 0) { h->error = "law without states or without inputs"; return fail(); }
  int64_t info[16] = {0};
  char hash[64] = {0};
  if (h->open("sensitivity-based MPC law", desc->code_object_path, nullptr,
              {{"dompc_asmpc_prepare_kernel", &h->fn_prep, DOMPC_TWIN(dompc_asmpc_hostemu_prepare)},
               {"dompc_asmpc_step_kernel", &h->fn_step, DOMPC_TWIN(dompc_asmpc_hostemu_step)},
               {"dompc_asmpc_select_count_kernel", &h->fn_sel_count, DOMPC_TWIN(dompc_asmpc_hostemu_select_count)},
               {"dompc_asmpc_select_write_kernel", &h->fn_sel_write, DOMPC_TWIN(dompc_asmpc_hostemu_select_write)}},
              "code object lacks the law kernels", "dompc_asmpc_info_kernel", DOMPC_TWIN(dompc_asmpc_hostemu_info), info, hash))
    return fail();
  const int64_t want[2] = {desc->nx, desc->nu};
  if (h->check_info("law ", info, want, 2, 2, sizeof(dompc_asmpck::PrepArgs), hash, desc->model_hash)) return fail();
  if (info[3] != (int64_t)sizeof(dompc_asmpck::StepArgs) || info[4] != (int64_t)sizeof(dompc_asmpck::SelectArgs)) { h->error = "law argument layout mismatch between runtime and code object"; return fail(); }
  const size_t D = sizeof(double);
  if (h->alloc((void**)&h->lb, D * desc->nu) || h->alloc((void**)&h->ub, D * desc->nu) || h->alloc((void**)&h->xs, D * desc->nx)) return fail();
  std::vector<double> lo((size_t)desc->nu, -INFINITY), hi((size_t)desc->nu, INFINITY), one((size_t)desc->nx, 1.0);
  if (h->h2d(h->lb, lo.data(), D * lo.size()) || h->h2d(h->ub, hi.data(), D * hi.size()) || h->h2d(h->xs, one.data(), D * one.size()) || h->sync())
    return fail();
  h->d.code_object_path = nullptr; h->d.model_hash = nullptr;
  *out = h;
  return 0;
}

extern "C" int dompc_asmpc_set_options(dompc_asmpc* h, const double* lbu, const double* ubu, const double* x_scale, int32_t clip,
                                       double max_dx) {
  if (!h) return 1;
  if (!lbu || !ubu || !x_scale) { h->error = "null pointer"; return 1; }
  if (!(max_dx >= 0.0)) { h->error = "max_dx must not be negative"; return 1; }
  if (h->set_device() || h->drain()) return 1;     // no step that still reads the old bounds is in flight on any stream
  const size_t D = sizeof(double);
  if (h->h2d(h->lb, lbu, D * h->d.nu) || h->h2d(h->ub, ubu, D * h->d.nu) || h->h2d(h->xs, x_scale, D * h->d.nx) || h->sync()) return 1;
  h->clip = clip ? 1 : 0;
  h->max_dx = max_dx;
  return 0;
}

static void fill_law(const dompc_asmpc* h, dompc_affine::Law& L) {
  L.x_ref = h->x_ref; L.u_ref = h->u_ref; L.M = h->M; L.flags = h->flags;
  L.lb = h->lb; L.ub = h->ub; L.x_scale = h->xs;
  L.ld = h->law_B; L.max_dx = h->max_dx; L.clip = h->clip; L.pad = 0;
}

extern "C" int32_t dompc_asmpc_law_batch(const dompc_asmpc* h) { return h ? h->law_B : 0; }

extern "C" int dompc_asmpc_law(dompc_asmpc* h, dompc_affine_law* out) {
  if (!h) return 1;
  if (!out) { h->error = "null pointer"; return 1; }
  if (h->law_B <= 0) { h->error = "no law: nothing has been solved yet (dompc_asmpc_prepare_device / dompc_asmpc_set_law)"; return 1; }
  dompc_affine::Law L;
  fill_law(h, L);
  memcpy(out, &L, sizeof(L));
  return 0;
}

// the law preparation for n entries: into the columns 0 .. n-1 of the record (slot null) or into the columns slot[j]
static int launch_prepare(dompc_asmpc* h, int32_t n, const int32_t* slot, const double* x_prev, const double* u0, const double* J,
                          int64_t row_J, int64_t batch_J, const double* G, int64_t row_G, int64_t batch_G, const int32_t* ok, void* stream) {
  dompc_asmpck::PrepArgs A;
  memset(&A, 0, sizeof(A));
  A.x_prev = x_prev; A.u0 = u0; A.J = J; A.G = G; A.ok = ok; A.slot = slot;
  A.row_J = row_J; A.batch_J = batch_J; A.row_G = row_G; A.batch_G = batch_G;
  fill_law(h, A.law);
  A.batch = n;
  // one wavefront per workgroup, four loops per wavefront
  return h->run(h->fn_prep, (unsigned)((n + 3) / 4), 64, 0, stream, &A, sizeof(A));
}

extern "C" int dompc_asmpc_prepare_device(dompc_asmpc* h, int32_t B, const double* x_prev, const double* u0, const double* J, int64_t row_J,
                                          int64_t batch_J, const double* G, int64_t row_G, int64_t batch_G, const int32_t* ok, void* stream) {
  if (!h) return 1;
  if (B <= 0) { h->error = "empty batch"; return 1; }
  if (B > MAX_BATCH) { h->error = "batch larger than 1048576 loops"; return 1; }
  if (!x_prev || !u0 || !J || !G) { h->error = "null pointer"; return 1; }
  if (row_J <= 0 || row_G <= 0 || row_J > INT32_MAX || row_G > INT32_MAX) { h->error = "row strides of J and G must be positive"; return 1; }
  const dompc_asmpc_desc& d = h->d;
  if (h->set_device()) return 1;
  h->law_B = 0;
  const size_t D = sizeof(double);
  if (h->grow_staging(&h->law_cap, B, {{(void**)&h->x_ref, D * d.nx}, {(void**)&h->u_ref, D * d.nu}, {(void**)&h->M, D * d.nx * d.nu},
                                       {(void**)&h->flags, sizeof(int32_t)}}))
    return 1;
  h->law_B = B;
  return launch_prepare(h, B, nullptr, x_prev, u0, J, row_J, batch_J, G, row_G, batch_G, ok, stream);
}

extern "C" int dompc_asmpc_update_device(dompc_asmpc* h, int32_t n, const int32_t* slot, const double* x_prev, const double* u0,
                                         const double* J, int64_t row_J, int64_t batch_J, const double* G, int64_t row_G, int64_t batch_G,
                                         const int32_t* ok, void* stream) {
  if (!h) return 1;
  if (h->law_B <= 0) { h->error = "no law to update: nothing has been solved yet (dompc_asmpc_prepare_device / dompc_asmpc_set_law)"; return 1; }
  if (n < 0 || n > h->law_B) {
    char buf[160];
    snprintf(buf, sizeof(buf), "the law holds %d loops, the update names %d", (int)h->law_B, (int)n);
    h->error = buf;
    return 1;
  }
  if (n == 0) return 0;
  if (!slot || !x_prev || !u0 || !J || !G) { h->error = "null pointer"; return 1; }
  if (row_J <= 0 || row_G <= 0 || row_J > INT32_MAX || row_G > INT32_MAX) { h->error = "row strides of J and G must be positive"; return 1; }
  if (h->set_device()) return 1;
  return launch_prepare(h, n, slot, x_prev, u0, J, row_J, batch_J, G, row_G, batch_G, ok, stream);
}

extern "C" int dompc_asmpc_update_law(dompc_asmpc* h, int32_t n, const int32_t* slot, const double* x_prev, const double* u0,
                                      const double* J, const double* G, const int32_t* ok) {
  if (!h) return 1;
  if (h->law_B <= 0) { h->error = "no law to update: nothing has been solved yet (dompc_asmpc_prepare_device / dompc_asmpc_set_law)"; return 1; }
  if (n < 0 || n > h->law_B) { h->error = "the update names more loops than the law holds"; return 1; }
  if (n == 0) return 0;
  if (!slot || !x_prev || !u0 || !J || !G) { h->error = "null pointer"; return 1; }
  const dompc_asmpc_desc& d = h->d;
  if (h->set_device()) return 1;
  const size_t D = sizeof(double), N = (size_t)n;
  if (h->grow_host_staging(n)) return 1;
  if (h->h2d(h->s_x, x_prev, D * N * d.nx) || h->h2d(h->s_u, u0, D * N * d.nu) || h->h2d(h->s_J, J, D * N * d.nx * d.nu) ||
      h->h2d(h->s_G, G, D * N * d.nu * d.nu) || h->h2d(h->s_slot, slot, sizeof(int32_t) * N) || (ok && h->h2d(h->s_ok, ok, sizeof(int32_t) * N)))
    return 1;
  if (dompc_asmpc_update_device(h, n, h->s_slot, h->s_x, h->s_u, h->s_J, d.nx, (int64_t)d.nx * d.nu, h->s_G, d.nu, (int64_t)d.nu * d.nu,
                                ok ? h->s_ok : nullptr, h->stream_ptr()))
    return 1;
  return h->sync();
}

extern "C" int dompc_asmpc_select_device(dompc_asmpc* h, int32_t B, const int32_t* status, int32_t mask, int32_t* idx, int32_t* count,
                                         void* stream) {
  if (!h) return 1;
  if (B <= 0) { h->error = "empty batch"; return 1; }
  if (B > MAX_BATCH) { h->error = "batch larger than 1048576 loops"; return 1; }
  if (!status || !idx || !count) { h->error = "null pointer"; return 1; }
  if (h->set_device()) return 1;
  const int32_t groups = (B + dompc_asmpck::SELECT_SPAN - 1) / dompc_asmpck::SELECT_SPAN;
  if (groups > h->sel_cap) {
    if (h->drain()) return 1;              // no selection that still uses the old counts is in flight on any stream
    if (h->grow_staging(&h->sel_cap, groups, {{(void**)&h->sel_count, sizeof(int32_t)}})) return 1;
  }
  dompc_asmpck::SelectArgs A;
  memset(&A, 0, sizeof(A));
  A.status = status; A.idx = idx; A.count = count; A.group_count = h->sel_count;
  A.batch = B; A.mask = mask;
  if (h->run(h->fn_sel_count, (unsigned)groups, dompc_asmpck::SELECT_THREADS, 0, stream, &A, sizeof(A))) return 1;
  return h->run(h->fn_sel_write, (unsigned)groups, dompc_asmpck::SELECT_THREADS, 0, stream, &A, sizeof(A));
}

extern "C" int dompc_asmpc_set_law(dompc_asmpc* h, int32_t B, const double* x_prev, const double* u0, const double* J, const double* G,
                                   const int32_t* ok) {
  if (!h) return 1;
  if (B <= 0) { h->error = "empty batch"; return 1; }
  if (!x_prev || !u0 || !J || !G) { h->error = "null pointer"; return 1; }
  const dompc_asmpc_desc& d = h->d;
  if (h->set_device()) return 1;
  const size_t D = sizeof(double);
  if (h->grow_host_staging(B)) return 1;
  if (h->h2d(h->s_x, x_prev, D * B * d.nx) || h->h2d(h->s_u, u0, D * B * d.nu) || h->h2d(h->s_J, J, D * B * d.nx * d.nu) ||
      h->h2d(h->s_G, G, D * B * d.nu * d.nu) || (ok && h->h2d(h->s_ok, ok, sizeof(int32_t) * (size_t)B)))
    return 1;
  if (dompc_asmpc_prepare_device(h, B, h->s_x, h->s_u, h->s_J, d.nx, (int64_t)d.nx * d.nu, h->s_G, d.nu, (int64_t)d.nu * d.nu,
                                 ok ? h->s_ok : nullptr, h->stream_ptr()))
    return 1;
  return h->sync();
}

extern "C" int dompc_asmpc_get_law(dompc_asmpc* h, double* x_ref, double* u_ref, double* M, int32_t* flags) {
  if (!h) return 1;
  if (h->law_B <= 0) { h->error = "no law: nothing has been solved yet"; return 1; }
  const dompc_asmpc_desc& d = h->d;
  const size_t B = (size_t)h->law_B, D = sizeof(double);
  if (h->set_device() || h->drain()) return 1;     // a preparation on a stream of the caller has finished
  std::vector<double> xr(B * d.nx), ur(B * d.nu), m(B * d.nx * d.nu);
  if (h->d2h(xr.data(), h->x_ref, D * xr.size()) || h->d2h(ur.data(), h->u_ref, D * ur.size()) || h->d2h(m.data(), h->M, D * m.size()) ||
      (flags && h->d2h(flags, h->flags, sizeof(int32_t) * B)) || h->sync())
    return 1;
  for (size_t b = 0; b < B; ++b) {
    if (x_ref) for (int k = 0; k < d.nx; ++k) x_ref[b * d.nx + k] = xr[k * B + b];
    if (u_ref) for (int i = 0; i < d.nu; ++i) u_ref[b * d.nu + i] = ur[i * B + b];
    if (M) for (int e = 0; e < d.nx * d.nu; ++e) M[b * d.nx * d.nu + e] = m[e * B + b];
  }
  return 0;
}

extern "C" int dompc_asmpc_step_batch_device(dompc_asmpc* h, int32_t B, const double* x, double* u, int32_t* status, void* stream) {
  if (!h) return 1;
  if (B <= 0) return 0;
  if (h->law_B <= 0) { h->error = "no law: nothing has been solved yet (dompc_asmpc_prepare_device / dompc_asmpc_set_law)"; return 1; }
  if (B != h->law_B) {
    char buf[160];
    snprintf(buf, sizeof(buf), "the law was prepared for %d loops, the step asks for %d", (int)h->law_B, (int)B);
    h->error = buf;
    return 1;
  }
  if (!x || !u) { h->error = "null pointer"; return 1; }
  dompc_asmpck::StepArgs A;
  memset(&A, 0, sizeof(A));
  A.x = x; A.u = u; A.status = status;
  fill_law(h, A.law);
  A.batch = B;
  if (h->set_device()) return 1;
  return h->run(h->fn_step, (unsigned)((B + 63) / 64), 64, 0, stream, &A, sizeof(A));
}

// the law step on a record of the CALLER's (e.g. one step of a time-varying law, dompc_lqr_tv_device): the handle lends its kernel
extern "C" int dompc_asmpc_step_law_device(dompc_asmpc* h, const dompc_affine_law* law, int32_t B, const double* x, double* u,
                                           int32_t* status, void* stream) {
  if (!h) return 1;
  if (B <= 0) return 0;
  if (!law || !x || !u) { h->error = "null pointer"; return 1; }
  if (!law->x_ref || !law->u_ref || !law->M || !law->x_scale || (law->clip && (!law->lb || !law->ub)) || law->ld < B) {
    h->error = "dompc_asmpc_step_law_device: incomplete law record (x_ref, u_ref, M, x_scale, with clip lb and ub; ld >= B)";
    return 1;
  }
  dompc_asmpck::StepArgs A;
  memset(&A, 0, sizeof(A));
  A.x = x; A.u = u; A.status = status;
  memcpy(&A.law, law, sizeof(A.law));
  A.batch = B;
  if (h->set_device()) return 1;
  return h->run(h->fn_step, (unsigned)((B + 63) / 64), 64, 0, stream, &A, sizeof(A));
}

extern "C" int dompc_asmpc_step_batch(dompc_asmpc* h, int32_t B, const double* x, double* u_out, int32_t* status) {
  if (!h) return 1;
  if (B <= 0) return 0;
  if (!x || !u_out) { h->error = "null pointer"; return 1; }
  const dompc_asmpc_desc& d = h->d;
  if (h->set_device()) return 1;
  const size_t D = sizeof(double);
  if (h->grow_host_staging(B)) return 1;
  if (h->h2d(h->s_x, x, D * B * d.nx)) return 1;
  if (dompc_asmpc_step_batch_device(h, B, h->s_x, h->s_u, h->s_st, h->stream_ptr())) return 1;
  if (h->d2h(u_out, h->s_u, D * B * d.nu) || (status && h->d2h(status, h->s_st, sizeof(int32_t) * (size_t)B))) return 1;
  return h->sync();
}
