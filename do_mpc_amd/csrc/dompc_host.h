// dompc_host.h - the host device layer shared by dompc_runtime.cpp, dompc_plant_runtime.cpp and dompc_ekf_runtime.cpp: the one
// place that knows both build flavours of the runtimes (product: HIP; test: -DDOMPC_HOST_EMU, "device" memory = host memory).
// Host only - no .hip file and no kernel header includes it.  Everything is inline: the three .cpp files are three translation
// units of libdompc_ipm.so and, each one alone, a host-emulation library of the tests.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#ifndef DOMPC_HOST_EMU
#include <hip/hip_runtime.h>
// `c`: pointer to a Context (or to a handle that derives from it); leaves the calling function with 1 and the error text in c->error
#define HIPCHK(c, expr)                                                                     \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess) {                                                                 \
      (c)->error = std::string(#expr) + ": " + hipGetErrorString(_e);                       \
      return 1;                                                                             \
    }                                                                                       \
  } while (0)
#endif

namespace dompc_host {

struct StagingSlot { void** slot; size_t bytes_per_row; };      // one staging buffer of a host-pointer entry point

// What every handle owns on its device.  The handle structs derive from it; every operation returns 0 or 1 with `error` set.
struct Context {
  std::string error;
  int32_t device = 0;
  std::vector<void*> allocs;             // every live device allocation of the handle: freed by close()

  void release(void* p) {                // free one tracked allocation
    if (!p) return;
    for (size_t i = 0; i < allocs.size(); ++i)
      if (allocs[i] == p) { allocs.erase(allocs.begin() + i); free_dev(p); return; }
  }

  // Staging buffers for a batch of B rows.   They are invalid from the first line until ALL new ones exist: capacity 0
  // and null pointers first, so that a failed allocation cannot leave a later call (B <= old capacity) copying into freed device
  // memory; the capacity is set after the last allocation succeeded.
  int grow_staging(int32_t* cap, int32_t B, std::initializer_list<StagingSlot> slots) {
    if (B <= *cap) return 0;
    *cap = 0;
    for (const StagingSlot& s : slots) { void* old = *s.slot; *s.slot = nullptr; release(old); }
    for (const StagingSlot& s : slots)
      if (alloc(s.slot, (size_t)B * s.bytes_per_row)) return 1;
    *cap = B;
    return 0;
  }

#ifndef DOMPC_HOST_EMU
  hipStream_t stream = nullptr;          // the stream of the staging copies
  std::vector<hipModule_t> modules;

  int alloc(void** p, size_t bytes) {
    HIPCHK(this, hipMalloc(p, bytes ? bytes : 8));
    allocs.push_back(*p);
    return 0;
  }
  static void free_dev(void* p) { (void)hipFree(p); }
  int h2d(void* dst, const void* src, size_t bytes) {
    if (!bytes) return 0;
    HIPCHK(this, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
    return 0;
  }
  int d2h(void* dst, const void* src, size_t bytes) {
    if (!bytes) return 0;
    HIPCHK(this, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream));
    return 0;
  }
  int sync() {
    HIPCHK(this, hipStreamSynchronize(stream));
    return 0;
  }
  int set_device() {
    HIPCHK(this, hipSetDevice(device));
    return 0;
  }
  void* stream_ptr() const { return (void*)stream; }

  // `component` names the caller in the message a user without a GPU reads ("plant integrator", ...)
  int open_device(const char* component) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
      error = std::string("no HIP device available: the dompc ") + component + " requires an AMD GPU (gfx950)";
      return 1;
    }
    if (hipSetDevice(device) != hipSuccess) { error = "hipSetDevice failed"; return 1; }
    if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) { error = "hipStreamCreate failed"; return 1; }
    return 0;
  }

  struct Kernel { const char* name; hipFunction_t* fn; };
  // load the code object at `path` and look the kernels up; `lacks`: the message when one of them is missing
  int load_module(const char* path, hipModule_t* module, std::initializer_list<Kernel> kernels, const std::string& lacks) {
    if (!path || hipModuleLoad(module, path) != hipSuccess) {
      error = std::string("hipModuleLoad failed for ") + (path ? path : "(null)");
      return 1;
    }
    modules.push_back(*module);
    for (const Kernel& k : kernels)
      if (hipModuleGetFunction(k.fn, *module, k.name) != hipSuccess) { error = lacks; return 1; }
    return 0;
  }
  void unload_module(hipModule_t m) {
    for (size_t i = 0; i < modules.size(); ++i)
      if (modules[i] == m) { modules.erase(modules.begin() + i); (void)hipModuleUnload(m); return; }
  }

  // launch with the argument block passed as a parameter buffer; `lds_bytes`: dynamic LDS
  int launch(hipFunction_t fn, unsigned grid, unsigned block, unsigned lds_bytes, hipStream_t st, void* args, size_t args_bytes) {
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &args_bytes, HIP_LAUNCH_PARAM_END};
    HIPCHK(this, hipModuleLaunchKernel(fn, grid, 1, 1, block, 1, 1, lds_bytes, st, nullptr, cfg));
    return 0;
  }

  // info kernel of a code object (1 x 64 threads, arguments {int64_t* info, char* hash}): what it was built for
  int query_info(hipFunction_t fn, const char* kernel_name, int64_t (&info)[16], char (&hash)[64]) {
    int64_t* info_d; char* hash_d;
    if (alloc((void**)&info_d, sizeof(info)) || alloc((void**)&hash_d, sizeof(hash))) return 1;
    struct { int64_t* a; char* b; } args = {info_d, hash_d};
    if (launch(fn, 1, 64, 0, stream, &args, sizeof(args)) || d2h(info, info_d, sizeof(info)) || d2h(hash, hash_d, sizeof(hash)) || sync()) {
      error = std::string(kernel_name) + " failed";
      return 1;
    }
    return 0;
  }

  void close() {                         // everything the context owns; the handle itself is deleted by the caller
    (void)hipSetDevice(device);
    for (void* p : allocs) free_dev(p);
    for (hipModule_t m : modules) (void)hipModuleUnload(m);
    if (stream) (void)hipStreamDestroy(stream);
  }
#else
  int alloc(void** p, size_t bytes) {
    *p = calloc(1, bytes ? bytes : 8);
    if (!*p) { error = "out of memory"; return 1; }
    allocs.push_back(*p);
    return 0;
  }
  static void free_dev(void* p) { free(p); }
  int h2d(void* dst, const void* src, size_t bytes) { if (bytes) memcpy(dst, src, bytes); return 0; }
  int d2h(void* dst, const void* src, size_t bytes) { if (bytes) memcpy(dst, src, bytes); return 0; }
  int sync() { return 0; }
  int set_device() { return 0; }
  void* stream_ptr() const { return nullptr; }
  void close() { for (void* p : allocs) free_dev(p); }
#endif

  // What the info kernel reported against what the description asks for: the first n_want entries of info[], sizeof(Args) at
  // info[i_args], the model hash.  `what` starts the messages ("plant ", "filter ", "" for the solver).
  int check_info(const char* what, const int64_t* info, const int64_t* want, int n_want, int i_args, size_t args_bytes,
                 const char* hash, const char* want_hash) {
    for (int i = 0; i < n_want; ++i)
      if (info[i] != want[i]) {
        char buf[256];
        snprintf(buf, sizeof(buf), "%scode object was built for different model dimensions (field %d: %lld vs %lld)", what, i,
                 (long long)info[i], (long long)want[i]);
        error = buf;
        return 1;
      }
    if (info[i_args] != (int64_t)args_bytes) { error = std::string(what) + "argument layout mismatch between runtime and code object"; return 1; }
    if (want_hash && strncmp(want_hash, hash, 63) != 0) {
      error = std::string(what) + "model hash mismatch: code object " + hash + " vs description " + want_hash;
      return 1;
    }
    return 0;
  }
};

}  // namespace dompc_host
