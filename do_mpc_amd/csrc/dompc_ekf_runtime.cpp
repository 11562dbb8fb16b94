// dompc_ekf_runtime.cpp - host side of the batched extended Kalman filter behind the C ABI of include/dompc_ipm.h (dompc_ekf_*).
// Generic: sizes come from the per-model code object (dompc_ekf_info_kernel).
// Build flavours as dompc_plant_runtime.cpp: product = part of libdompc_ipm.so (HIP only); test = g++ -DDOMPC_HOST_EMU together with
// dompc_ekf.hip compiled as C++ (tests/_hostemu; never shipped).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dompc_ipm.h"
#include "dompc_ekf_args.h"

#ifndef DOMPC_HOST_EMU
#include <hip/hip_runtime.h>
#else
extern "C" void dompc_ekf_hostemu_info(int64_t* out, char* hash);
extern "C" void dompc_ekf_hostemu_run(const dompc_ekfk::Args* A);
#endif

static thread_local std::string g_ekf_create_error;

struct dompc_ekf {
  dompc_ekf_desc d;
  std::string error;
  int32_t cap = 0;
  double *s_x = nullptr, *s_P = nullptr, *s_y = nullptr, *s_u = nullptr, *s_tvp = nullptr, *s_p = nullptr, *s_Q = nullptr, *s_R = nullptr;
  int32_t* s_st = nullptr;
  std::vector<void*> allocs;
#ifndef DOMPC_HOST_EMU
  hipModule_t module = nullptr;
  hipFunction_t fn = nullptr, fn_info = nullptr;
  hipStream_t stream = nullptr;
#endif
};

#ifndef DOMPC_HOST_EMU
#define EHIP(h, expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) { (h)->error = std::string(#expr) + ": " + hipGetErrorString(_e); return 1; } \
  } while (0)
static int ealloc(dompc_ekf* h, void** p, size_t bytes) {
  EHIP(h, hipMalloc(p, bytes ? bytes : 8));
  h->allocs.push_back(*p);
  return 0;
}
static void efree(void* p) { (void)hipFree(p); }
#else
static int ealloc(dompc_ekf* h, void** p, size_t bytes) {
  *p = calloc(1, bytes ? bytes : 8);
  if (!*p) { h->error = "out of memory"; return 1; }
  h->allocs.push_back(*p);
  return 0;
}
static void efree(void* p) { free(p); }
#endif

extern "C" const char* dompc_ekf_last_error(const dompc_ekf* h) { return h ? h->error.c_str() : g_ekf_create_error.c_str(); }

extern "C" void dompc_ekf_destroy(dompc_ekf* h) {
  if (!h) return;
#ifndef DOMPC_HOST_EMU
  (void)hipSetDevice(h->d.device);
#endif
  for (void* p : h->allocs) efree(p);
#ifndef DOMPC_HOST_EMU
  if (h->module) (void)hipModuleUnload(h->module);
  if (h->stream) (void)hipStreamDestroy(h->stream);
#endif
  delete h;
}

extern "C" int dompc_ekf_create(const dompc_ekf_desc* desc, dompc_ekf** out) {
  if (!desc || !out) { g_ekf_create_error = "null argument"; return 1; }
  dompc_ekf* h = new dompc_ekf();
  h->d = *desc;
  auto fail = [&]() { g_ekf_create_error = h->error; dompc_ekf_destroy(h); *out = nullptr; return 1; };
  if (desc->nx <= 0) { h->error = "filter without states"; return fail(); }
  if (!(desc->t_step > 0.0) && !desc->discrete) { h->error = "t_step must be positive"; return fail(); }
  int64_t info[16] = {0};
  char hash[64] = {0};
#ifndef DOMPC_HOST_EMU
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    h->error = "no HIP device available: the dompc extended Kalman filter requires an AMD GPU (gfx950)";
    return fail();
  }
  if (hipSetDevice(desc->device) != hipSuccess) { h->error = "hipSetDevice failed"; return fail(); }
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { h->error = "hipStreamCreate failed"; return fail(); }
  if (!desc->code_object_path || hipModuleLoad(&h->module, desc->code_object_path) != hipSuccess) {
    h->error = std::string("hipModuleLoad failed for ") + (desc->code_object_path ? desc->code_object_path : "(null)");
    return fail();
  }
  if (hipModuleGetFunction(&h->fn, h->module, "dompc_ekf_kernel") != hipSuccess ||
      hipModuleGetFunction(&h->fn_info, h->module, "dompc_ekf_info_kernel") != hipSuccess) {
    h->error = "code object lacks the filter kernels"; return fail();
  }
  {
    int64_t* out_d; char* hash_d;
    if (ealloc(h, (void**)&out_d, sizeof(info)) || ealloc(h, (void**)&hash_d, sizeof(hash))) return fail();
    struct { int64_t* a; char* b; } args = {out_d, hash_d};
    size_t sz = sizeof(args);
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
    if (hipModuleLaunchKernel(h->fn_info, 1, 1, 1, 64, 1, 1, 0, h->stream, nullptr, cfg) != hipSuccess ||
        hipMemcpyAsync(info, out_d, sizeof(info), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipMemcpyAsync(hash, hash_d, sizeof(hash), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess) {
      h->error = "dompc_ekf_info_kernel failed"; return fail();
    }
  }
#else
  dompc_ekf_hostemu_info(info, hash);
#endif
  const int64_t want[6] = {desc->nx, desc->nu, desc->np, desc->ntvp, desc->ny, desc->discrete ? 1 : 0};
  for (int i = 0; i < 6; ++i)
    if (info[i] != want[i]) {
      char buf[200];
      snprintf(buf, sizeof(buf), "filter code object was built for different model dimensions (field %d: %lld vs %lld)", i,
               (long long)info[i], (long long)want[i]);
      h->error = buf;
      return fail();
    }
  if (info[6] != (int64_t)sizeof(dompc_ekfk::Args)) { h->error = "filter argument layout mismatch between runtime and code object"; return fail(); }
  if (desc->model_hash && strncmp(desc->model_hash, hash, 63) != 0) { h->error = "filter model hash mismatch"; return fail(); }
  h->d.code_object_path = nullptr; h->d.model_hash = nullptr;
  *out = h;
  return 0;
}

extern "C" int dompc_ekf_step_batch_device(dompc_ekf* h, int32_t B, double* x, double* P, const double* y, const double* u,
                                           const double* tvp, const double* p, const double* Q, const double* R,
                                           int32_t shared_mask, int32_t* status, void* stream) {
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
#ifndef DOMPC_HOST_EMU
  EHIP(h, hipSetDevice(d.device));
  size_t sz = sizeof(A);
  void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &A, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
  // one wavefront per workgroup, four filters per wavefront
  EHIP(h, hipModuleLaunchKernel(h->fn, (unsigned)((B + 3) / 4), 1, 1, 64, 1, 1, 0, (hipStream_t)stream, nullptr, cfg));
#else
  (void)stream;
  dompc_ekf_hostemu_run(&A);
#endif
  return 0;
}

extern "C" int dompc_ekf_step_batch(dompc_ekf* h, int32_t B, const double* x, const double* P, const double* y, const double* u,
                                    const double* tvp, const double* p, const double* Q, const double* R, int32_t shared_mask,
                                    double* x_out, double* P_out, int32_t* status) {
  if (!h) return 1;
  if (B <= 0) return 0;
  const dompc_ekf_desc& d = h->d;
  if (!x || !P || !Q || !x_out || !P_out || (d.ny && (!y || !R)) || (d.nu && !u) || (d.ntvp && !tvp) || (d.np && !p)) { h->error = "null pointer"; return 1; }
#ifndef DOMPC_HOST_EMU
  EHIP(h, hipSetDevice(d.device));
#endif
  if (B > h->cap) {
    // the staging buffers are invalid from here until ALL new ones exist (see dompc_plant_step_batch)
    h->cap = 0;
    void** slots[] = {(void**)&h->s_x, (void**)&h->s_P, (void**)&h->s_y, (void**)&h->s_u, (void**)&h->s_tvp, (void**)&h->s_p,
                      (void**)&h->s_Q, (void**)&h->s_R, (void**)&h->s_st};
    for (void** sp : slots) {
      void* q = *sp;
      *sp = nullptr;
      if (q) {
        for (size_t i = 0; i < h->allocs.size(); ++i)
          if (h->allocs[i] == q) { h->allocs.erase(h->allocs.begin() + i); efree(q); break; }
      }
    }
    const size_t n = (size_t)B * sizeof(double);
    if (ealloc(h, (void**)&h->s_x, n * d.nx) || ealloc(h, (void**)&h->s_P, n * d.nx * d.nx) || ealloc(h, (void**)&h->s_y, n * d.ny) ||
        ealloc(h, (void**)&h->s_u, n * d.nu) || ealloc(h, (void**)&h->s_tvp, n * d.ntvp) || ealloc(h, (void**)&h->s_p, n * d.np) ||
        ealloc(h, (void**)&h->s_Q, n * d.nx * d.nx) || ealloc(h, (void**)&h->s_R, n * d.ny * d.ny) ||
        ealloc(h, (void**)&h->s_st, (size_t)B * sizeof(int32_t)))
      return 1;
    h->cap = B;
  }
  auto rows = [&](int bit) { return (shared_mask & bit) ? (size_t)1 : (size_t)B; };
#ifndef DOMPC_HOST_EMU
  auto up = [&](void* dst, const void* src, size_t bytes) -> int {
    if (!bytes || !src) return 0;
    EHIP(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    return 0;
  };
  auto down = [&](void* dst, const void* src, size_t bytes) -> int {
    if (!bytes || !dst) return 0;
    EHIP(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    return 0;
  };
  void* st = (void*)h->stream;
#else
  auto up = [&](void* dst, const void* src, size_t bytes) -> int { if (bytes && src) memcpy(dst, src, bytes); return 0; };
  auto down = [&](void* dst, const void* src, size_t bytes) -> int { if (bytes && dst) memcpy(dst, src, bytes); return 0; };
  void* st = nullptr;
#endif
  const size_t D = sizeof(double);
  if (up(h->s_x, x, D * B * d.nx) || up(h->s_P, P, D * B * d.nx * d.nx) || up(h->s_y, y, D * B * d.ny) ||
      up(h->s_u, u, D * rows(1) * d.nu) || up(h->s_tvp, tvp, D * rows(2) * d.ntvp) || up(h->s_p, p, D * rows(4) * d.np) ||
      up(h->s_Q, Q, D * rows(8) * d.nx * d.nx) || up(h->s_R, R, D * rows(16) * d.ny * d.ny))
    return 1;
  if (dompc_ekf_step_batch_device(h, B, h->s_x, h->s_P, h->s_y, h->s_u, h->s_tvp, h->s_p, h->s_Q, h->s_R, shared_mask, h->s_st, st))
    return 1;
  if (down(x_out, h->s_x, D * B * d.nx) || down(P_out, h->s_P, D * B * d.nx * d.nx) || down(status, h->s_st, sizeof(int32_t) * (size_t)B)) return 1;
#ifndef DOMPC_HOST_EMU
  EHIP(h, hipStreamSynchronize(h->stream));
#endif
  return 0;
}
