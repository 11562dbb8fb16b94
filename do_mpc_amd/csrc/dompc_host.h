// dompc_host.h - the host device layer shared by the six runtimes (dompc_runtime.cpp and dompc_{plant,ekf,lqr,ampc,asmpc}_runtime.cpp):
// the one place that knows both build flavours of the runtimes (product: HIP; test: -DDOMPC_HOST_EMU, "device" memory = host memory,
// a kernel = its host twin, the same kernel text compiled by g++).  It hides the device, the stream, tracked allocations, staging
// buffers and copies, and - behind one Kernel handle - loading a code object, asking its info kernel what it was built for, and
// launching; a runtime forks on the flavour only for what exists with HIP alone (dompc_runtime.cpp: RCCL, mapped host words, ...).
// Host only - no .hip file and no kernel header includes it.  Everything is inline: the six .cpp files are six translation
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
#define DOMPC_TWIN(f) nullptr            // the product build launches the kernel; its host twin is declared, never defined
#else
#define DOMPC_TWIN(f) (f)
#endif

namespace dompc_host {

// The host twin of a kernel (host emulation): called with the argument block the kernel is launched with.
using Twin = void (*)(const void* args);

// What a runtime holds per kernel entry of its code object: the loaded function, or the twin in the host emulation.
#ifndef DOMPC_HOST_EMU
using Module = hipModule_t;
struct Kernel { hipFunction_t fn = nullptr; explicit operator bool() const { return fn != nullptr; } };
#else
using Module = void*;                    // (nothing is loaded: always null)
struct Kernel { Twin twin = nullptr; explicit operator bool() const { return twin != nullptr; } };
#endif
struct Entry { const char* name; Kernel* kernel; Twin twin; };     // a kernel to look up: Entry{"..._kernel", &k, DOMPC_TWIN(..._hostemu_...)}

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
  int h2d_now(void* dst, const void* src, size_t bytes) {      // has completed on return: `src` may go away
    HIPCHK(this, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
  }
  int fill(void* p, int byte, size_t bytes, void* st) {        // byte fill of an allocation, in the order of stream `st`
    HIPCHK(this, hipMemsetAsync(p, byte, bytes, (hipStream_t)st));
    return 0;
  }
  int drain() {                          // nothing is in flight on any stream of this device
    HIPCHK(this, hipDeviceSynchronize());
    return 0;
  }

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

  // load the code object at `path` and look the kernels up; `lacks`: the message when one of them is missing
  int load(const char* path, Module* module, std::initializer_list<Entry> kernels, const std::string& lacks) {
    if (!path || hipModuleLoad(module, path) != hipSuccess) {
      (void)hipGetLastError();           // (see find)
      error = std::string("hipModuleLoad failed for ") + (path ? path : "(null)");
      return 1;
    }
    modules.push_back(*module);
    for (const Entry& e : kernels)
      if (!find(*module, e)) { error = lacks; return 1; }
    return 0;
  }
  // one more entry of a loaded code object (an optional kernel, or one looked up on first use): false when it is not there.  The
  // refusal is the caller's to report: HIP's sticky last error is taken back, or the next launch check of another library in the
  // process (torch's) reports "named symbol not found" for a kernel of its own.
  bool find(Module module, const Entry& e) {
    if (hipModuleGetFunction(&e.kernel->fn, module, e.name) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
  }
  void unload(Module m) {
    for (size_t i = 0; i < modules.size(); ++i)
      if (modules[i] == m) { modules.erase(modules.begin() + i); (void)hipModuleUnload(m); return; }
  }

  // launch on stream `st` with the argument block passed as a parameter buffer; `lds_bytes`: dynamic LDS
  int run(Kernel k, unsigned grid, unsigned block, unsigned lds_bytes, void* st, const void* args, size_t args_bytes) {
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, const_cast<void*>(args), HIP_LAUNCH_PARAM_BUFFER_SIZE, &args_bytes, HIP_LAUNCH_PARAM_END};
    HIPCHK(this, hipModuleLaunchKernel(k.fn, grid, 1, 1, block, 1, 1, lds_bytes, (hipStream_t)st, nullptr, cfg));
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
  int h2d_now(void* dst, const void* src, size_t bytes) { return h2d(dst, src, bytes); }
  int fill(void* p, int byte, size_t bytes, void*) { memset(p, byte, bytes); return 0; }
  int drain() { return 0; }
  int open_device(const char*) { return 0; }
  // (nothing to load: the twins are bound, `module` stays null)
  int load(const char*, Module* module, std::initializer_list<Entry> kernels, const std::string&) {
    *module = nullptr;
    for (const Entry& e : kernels) find(*module, e);
    return 0;
  }
  bool find(Module, const Entry& e) { e.kernel->twin = e.twin; return true; }
  void unload(Module) {}
  int run(Kernel k, unsigned, unsigned, unsigned, void*, const void* args, size_t) { k.twin(args); return 0; }
  void close() { for (void* p : allocs) free_dev(p); }
#endif

  // The info kernel of a code object (1 x 64 threads): what it was built for.  Its arguments are {info, hash}, after a copy of the
  // input block `in` when there is one (the solver's: {in, info, hash}).
  template <int N>
  int query(Kernel k, const char* kernel_name, int64_t (&info)[N], char (&hash)[64], const void* in = nullptr, size_t in_bytes = 0) {
    void* args[3] = {nullptr, nullptr, nullptr};
    void **in_d = &args[0], **info_d = &args[in ? 1 : 0], **hash_d = info_d + 1;
    if ((in && alloc(in_d, in_bytes)) || alloc(info_d, sizeof(info)) || alloc(hash_d, sizeof(hash))) return 1;
    if ((in && h2d(*in_d, in, in_bytes)) || fill(*info_d, 0, sizeof(info), stream_ptr()) ||
        run(k, 1, 64, 0, stream_ptr(), args, (in ? 3 : 2) * sizeof(void*)) || d2h(info, *info_d, sizeof(info)) ||
        d2h(hash, *hash_d, sizeof(hash)) || sync()) {
      error = std::string(kernel_name) + " failed";
      return 1;
    }
    return 0;
  }

  // The start of every create: the device (`component` names the caller to a user without a GPU), the code object at `path` with
  // `kernels` (`lacks`: the message when one is missing, the info kernel included) and what its info kernel `info_kernel` reports.
  // `module`: null unless the caller looks further entries up later (find).
  template <int N>
  int open(const char* component, const char* path, Module* module, std::initializer_list<Entry> kernels, const std::string& lacks,
           const char* info_kernel, Twin info_twin, int64_t (&info)[N], char (&hash)[64], const void* in = nullptr, size_t in_bytes = 0) {
    Module m;
    Kernel k_info;
    if (open_device(component) || load(path, &m, kernels, lacks)) return 1;
    if (module) *module = m;
    if (!find(m, Entry{info_kernel, &k_info, info_twin})) { error = lacks; return 1; }
    return query(k_info, info_kernel, info, hash, in, in_bytes);
  }

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
