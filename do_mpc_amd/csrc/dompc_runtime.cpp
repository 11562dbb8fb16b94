// dompc_runtime.cpp - generic host runtime behind the C ABI of include/dompc_ipm.h.
//
// Owns: the loaded per-model gfx950 code object, device copies of the tree tables, the workspace
// slots of the persistent workgroups, staging buffers for the host-pointer entry points.
// It contains no model-dependent code: sizes come from the code object (dompc_model_info_kernel).
//
// Build flavours (do_mpc_amd/build.py):
//   product : hipcc -shared -fPIC dompc_runtime.cpp            -> libdompc_ipm.so   (HIP only)
//   test    : g++ -DDOMPC_HOST_EMU dompc_runtime.cpp dompc_device.hip(as C++) -> tests/_hostemu/*.so
//             ("device" memory = host memory, a workgroup = the calling thread).  Never shipped.
// Loading, the info query and the launches go through dompc_host.h in both flavours; a DOMPC_HOST_EMU conditional in this file marks
// something that exists with HIP only (RCCL, the mapped host words and the exchange loop, the shard stream, the watchdog, the occupancy
// query, the launch-shape overrides and wide mode) or the emulation's one slot.
#include <chrono>
#include <dlfcn.h>
#include <cmath>
#include <thread>

#include "dompc_host.h"
#include "dompc_kargs.h"
#include "dompc_shape.h"

using dompc_launch::BATCH_ONE_WAVE;
using dompc_launch::fit_block;

using dompc_host::Kernel;

// the host twins of the kernels (dompc_device.hip)
extern "C" void dompc_hostemu_model_info(const void* args);
extern "C" void dompc_hostemu_run(const void* args);
extern "C" void dompc_hostemu_sens_prep(const void* args);
extern "C" void dompc_hostemu_sens_finish(const void* args);

static thread_local std::string g_create_error;

struct dompc_handle : dompc_host::Context {
  dompc_problem_desc d;
  std::string code_path;
  int32_t e_pad = 0, n_slots = 0, block = 256, occupancy = 0, n_leaves = 1;
  bool batch_object_stale = false;       // a `_batch` sibling exists but was built from other sources / another model: not used
  bool block_auto = true;          // threads per problem chosen per call from the batch size
  int32_t slots64 = 0, slots256 = 0;   // resident workgroups at 64 / 256 threads
  int64_t ws_stride = 0, sweep_block = 0, el_size = 0, edges_per_wave = 1, riccati_kind = 0;
  dompc::KArgs base;       // tables + workspace filled in, I/O pointers zero
  // staging for host-pointer calls
  double *s_x0 = nullptr, *s_lbx = nullptr, *s_ubx = nullptr, *s_lbg = nullptr, *s_ubg = nullptr, *s_p = nullptr;
  double *s_x = nullptr, *s_g = nullptr, *s_lamx = nullptr, *s_lamg = nullptr, *s_f = nullptr;
  dompc_stats* s_stats = nullptr;
  double *s_dbg[8] = {nullptr};
  double* s_trace = nullptr;
  int32_t trace_cap = 4096;
  int32_t cap_batch = 0;
  // tree sharding
  int64_t xlayout[4] = {0, 0, 0, 0};   // RED_MAX, ASM_N, CUT1, CUT2 of the code object
  bool sharded = false, shard_capable = false;
  dompc_allreduce_fn allreduce = nullptr;
  void* allreduce_ctx = nullptr;
  uint32_t* x_words = nullptr;           // pinned host memory: [req, ack, count, off] (device build)
  int32_t* abort_word = nullptr;         // pinned host memory (device build) / plain word: stop request read by the kernel
  double watchdog_s = 600.0;
  int64_t n_exchanges = 0;                      // cross-rank exchanges served during the last sharded solve
  // sensitivities (dompc_sens_batch_device): parameter rows and selected direction entries of a chunk of points; staging of the host twin
  double* sn_work = nullptr;
  int64_t sn_work_doubles = 0;
  double *s_sn_mu = nullptr, *s_sn_S = nullptr, *s_sn_res = nullptr;
  int32_t *s_sn_ok = nullptr, *s_sn_tab = nullptr;
  int32_t sn_cap_batch = 0;
  int64_t sn_cap_S = 0, sn_cap_tab = 0;
  dompc_host::Module module = nullptr, module_batch = nullptr;      // the general object and its batch-only sibling (build.py: batch_only)
  Kernel fn_solve, fn_solve_batch;
  Kernel fn_sens, fn_sens_batch, fn_sens_prep, fn_sens_finish;     // looked up by the first sensitivity call
#ifndef DOMPC_HOST_EMU
  // native RCCL collective (dlopen'ed): communicator of the sharded problem and its stream
  struct RcclUid { char internal[128]; };
  void* rccl_lib = nullptr;
  int (*nccl_get_unique_id)(RcclUid*) = nullptr;
  int (*nccl_comm_init_rank)(void**, int, RcclUid, int) = nullptr;
  int (*nccl_all_reduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*nccl_comm_destroy)(void*) = nullptr;
  const char* (*nccl_error_string)(int) = nullptr;
  void* rccl_comm = nullptr;
  hipStream_t rccl_stream = nullptr;
  hipStream_t shard_stream = nullptr;    // lowest priority: never shares a hardware queue with the collective's kernels
#endif
};

// ------------------------------------------------------------------------------------------------
#ifndef DOMPC_HOST_EMU
// Wait for `st` with the watchdog: after watchdog_s the stop request is raised (the kernel leaves its IPM loops with
// status 6); if the stream still has not drained after a grace period the call fails instead of blocking forever.
// The limit is per ROUND over the resident problem slots (a batch of B problems on n_slots slots takes ceil(B / n_slots) rounds): a
// legitimately long batch is not cut short by a limit that was sized for one problem.  A watchdog that fired leaves a message in
// dompc_last_error even though the call succeeds (the problems it stopped carry status 6, `User_Requested_Stop`).
static int dev_sync_watchdog(dompc_handle* h, hipStream_t st, int rounds = 1) {
  const auto t0 = std::chrono::steady_clock::now();
  bool raised = false;
  const double limit = h->watchdog_s * (rounds > 1 ? rounds : 1);
  while (true) {
    const hipError_t q = hipStreamQuery(st);
    if (q == hipSuccess) break;
    if (q != hipErrorNotReady) { h->error = std::string("hipStreamQuery: ") + hipGetErrorString(q); return 1; }
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!raised && dt > limit) { int32_t z_ = 0; __atomic_compare_exchange_n(h->abort_word, &z_, 1, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE); raised = true; }   // (0 -> 1: a user's request, 2, is left alone)
    if (raised && dt > limit + 30.0) {
      h->error = "watchdog: the solver kernel did not finish and did not react to the stop request";
      return 1;
    }
    if (dt > 0.002) std::this_thread::sleep_for(std::chrono::microseconds(dt > 0.2 ? 500 : 20));
  }
  if (raised) {
    // only the watchdog's own request is withdrawn (compare-exchange 1 -> 0: a user's dompc_abort(h, 1) writes 2 and stays -
    // it is documented as sticky until dompc_abort(h, 0)); the caller learns about it through the error string and status 6
    int32_t expect = 1;
    __atomic_compare_exchange_n(h->abort_word, &expect, 0, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE);
    char msg[200];
    snprintf(msg, sizeof msg, "watchdog: stop request raised after %.0f s (DOMPC_WATCHDOG_S = %.0f s per round over the problem slots, %d round(s)); "
             "unfinished problems return status 6", limit, h->watchdog_s, rounds > 1 ? rounds : 1);
    h->error = msg;
  }
  return 0;
}
#endif

extern "C" int dompc_abort(dompc_handle* h, int32_t stop) {
  if (!h || !h->abort_word) return 1;
  __atomic_store_n(h->abort_word, stop ? 2 : 0, __ATOMIC_RELEASE);     // (2: the user's request - the watchdog only withdraws its own 1)
  return 0;
}

template <typename Tp>
static int upload(dompc_handle* h, const Tp** dst, const Tp* src, size_t n) {
  void* p = nullptr;
  if (h->alloc(&p, n * sizeof(Tp))) return 1;
  if (n && !src) { h->error = "null table pointer in problem description"; return 1; }
  if (h->h2d(p, src, n * sizeof(Tp))) return 1;
  *dst = (const Tp*)p;
  return 0;
}

// ------------------------------------------------------------------------------------------------
extern "C" void dompc_default_options(dompc_options* o) {
  o->tol = 1e-8; o->dual_inf_tol = 1.0; o->constr_viol_tol = 1e-4; o->compl_inf_tol = 1e-4;
  o->acceptable_tol = 1e-6; o->mu_init = 0.1; o->kappa_mu = 0.2; o->theta_mu = 1.5; o->kappa_eps = 10.0;
  o->tau_min = 0.99; o->bound_push = 0.01; o->bound_frac = 0.01; o->bound_relax_factor = 1e-8;
  o->nlp_scaling_max_gradient = 100.0; o->delta_w_0 = 1e-4; o->delta_w_min = 1e-20; o->delta_w_max = 1e20;
  o->kappa_w_minus = 1.0 / 3.0; o->kappa_w_plus = 8.0; o->kappa_w_plus_bar = 100.0;
  o->max_iter = 3000; o->acceptable_iter = 15; o->obj_scaling = 1; o->max_soc = 4;
  o->constr_mult_init_max = 1000.0;
  o->watchdog_shortened_iter_trigger = 10; o->watchdog_trial_iter_max = 3;
}

extern "C" const char* dompc_status_string(int32_t s) {
  switch (s) {
    case 0: return "Solve_Succeeded";
    case 1: return "Solved_To_Acceptable_Level";
    case 2: return "Maximum_Iterations_Exceeded";
    case 3: return "Error_In_Step_Computation";
    case 4: return "Invalid_Number_Detected";
    case 6: return "User_Requested_Stop";
    default: return "Internal_Error";
  }
}

extern "C" const char* dompc_last_error(const dompc_handle* h) { return h ? h->error.c_str() : g_create_error.c_str(); }

extern "C" void dompc_destroy(dompc_handle* h) {
  if (!h) return;
  h->close();
#ifndef DOMPC_HOST_EMU
  if (h->x_words) hipHostFree(h->x_words);
  if (h->abort_word) hipHostFree(h->abort_word);
  if (h->shard_stream) hipStreamDestroy(h->shard_stream);
  if (h->rccl_comm && h->nccl_comm_destroy) h->nccl_comm_destroy(h->rccl_comm);
  if (h->rccl_stream) hipStreamDestroy(h->rccl_stream);
#else
  free(h->abort_word);
#endif
  delete h;
}

static int ensure_staging(dompc_handle* h, int B) {
  if (B <= h->cap_batch) return 0;
  const dompc_problem_desc& d = h->d;
  const size_t D = sizeof(double);
  if (!h->s_ubg) {      // per problem, not per batch row: allocated once
    if (h->alloc((void**)&h->s_lbx, D * d.n_opt_x) || h->alloc((void**)&h->s_ubx, D * d.n_opt_x) ||
        h->alloc((void**)&h->s_lbg, D * d.n_g) || h->alloc((void**)&h->s_ubg, D * d.n_g))
      return 1;
  }
  // (re)allocate for the larger batch; the superseded per-batch buffers are released now
  if (h->sync()) return 1;
  return h->grow_staging(&h->cap_batch, B, {{(void**)&h->s_x0, D * d.n_opt_x}, {(void**)&h->s_p, D * d.n_opt_p}, {(void**)&h->s_x, D * d.n_opt_x},
                                            {(void**)&h->s_g, D * d.n_g}, {(void**)&h->s_lamx, D * d.n_opt_x}, {(void**)&h->s_lamg, D * d.n_g},
                                            {(void**)&h->s_f, D}, {(void**)&h->s_stats, sizeof(dompc_stats)}});
}

static void* own_stream(dompc_handle* h) {
#ifndef DOMPC_HOST_EMU
  return (void*)((h->sharded && h->shard_stream) ? h->shard_stream : h->stream);
#else
  (void)h;
  return nullptr;
#endif
}

// what the launch shape is decided from (dompc_shape.h)
static dompc_shape_facts shape_facts(const dompc_handle* h) {
  return dompc_shape_facts{h->d.n_edges, h->n_leaves, (int32_t)h->edges_per_wave, h->el_size, h->slots64, h->slots256, h->n_slots, h->block,
                           h->block_auto ? 1 : 0, h->sharded ? 1 : 0};
}
#ifndef DOMPC_HOST_EMU
// DOMPC_WIDE / DOMPC_WIDE_SPREAD / DOMPC_WIDE_BLOCK, read at every solve.  Values that the decision never told apart are folded: a
// DOMPC_WIDE below 1 is one workgroup per problem like 0, and a DOMPC_WIDE_BLOCK other than 64/128/256/512 ran 256 threads like 256.
static dompc_shape_overrides shape_overrides() {
  dompc_shape_overrides o = {-1, -1, 0};
  if (const char* we = getenv("DOMPC_WIDE")) { const int v = atoi(we); o.wide = v > 0 ? v : 0; }
  if (const char* se = getenv("DOMPC_WIDE_SPREAD")) o.wide_spread = atoi(se) != 0 ? 1 : 0;
  if (const char* wb = getenv("DOMPC_WIDE_BLOCK")) { const int v = atoi(wb); o.wide_block = (v == 64 || v == 128 || v == 256 || v == 512) ? v : 256; }
  return o;
}
#endif

extern "C" int dompc_launch_shape(const dompc_shape_facts* facts, const dompc_shape_overrides* overrides, int32_t B, dompc_shape* out) {
  if (!facts || !overrides || !out || B < 1) return 1;
  *out = dompc_launch::solve_shape(*facts, *overrides, B);
  return 0;
}

// doubles of the LDS pool of a workgroup of `block` threads: one edge working set per wavefront, or the reduction rows if they are larger
static int64_t pool_doubles(const dompc_handle* h, int block) {
  const int64_t per_wave = (int64_t)(block / 64) * h->el_size, red = h->xlayout[0] * (int64_t)block;
  return per_wave > red ? per_wave : red;
}

// `block` threads per workgroup (a multiple of 64): the LDS pool is sized for block/64 wavefronts
// `stream`: nullptr = HIP default stream.  `other`: another entry of the code object with the same argument block and LDS pool
// (dompc_sens_kernel) in place of the solver kernel.
static int launch(dompc_handle* h, dompc::KArgs& A, int grid, int block, void* stream, Kernel other = Kernel()) {
  if (h->fill(A.work_counter, 0, sizeof(int32_t), stream)) return 1;
  A.pool_doubles = (int32_t)pool_doubles(h, block);
  // (batch launches of the solver with one 64-thread workgroup per problem, not sharded, run the build of the kernels that is compiled for
  //  exactly that shape when it was loaded: build.py batch_only)
  Kernel k = (h->fn_solve_batch && (A.mode == 0 || A.mode == 2) && A.wide <= 1 && block == 64 && !h->sharded) ? h->fn_solve_batch : h->fn_solve;
  if (other) k = other;
  return h->run(k, grid, block, (unsigned)(A.pool_doubles * sizeof(double)), stream, &A, sizeof(A));
}

extern "C" int dompc_create(const dompc_problem_desc* desc, dompc_handle** out) {
  if (!desc || !out) { g_create_error = "null argument"; return 1; }
  dompc_handle* h = new dompc_handle();
  h->d = *desc;
  h->device = desc->device;
  auto fail = [&](int) { g_create_error = h->error; dompc_destroy(h); *out = nullptr; return 1; };
  const dompc_problem_desc& d = h->d;
  if (d.n_edges <= 0 || d.n_nodes <= 0 || d.n_opt_x <= 0) { h->error = "empty problem description"; return fail(1); }
  // threads per problem in batch mode: one wavefront per problem (4x the problem slots, no workgroup barriers, no idle
  // wavefronts in the tree recursion) once the batch fills every resident wavefront at least twice, else four
  // wavefronts per problem (measured on MI355X, industrial_poly: B = 1024: 256 threads 1832 vs 64 threads 1152
  // steps/s; B = 4096: 3093 vs 3221)
  // The choice is made per call from the batch size unless the description fixes it (block_auto).
  h->block = d.block_threads > 0 ? d.block_threads : 256;
  h->block_auto = d.block_threads <= 0;
  if (const char* be = getenv("DOMPC_BLOCK")) { h->block = atoi(be); h->block_auto = false; }   // tuning aid (64/128/256)
  if (h->block != 64 && h->block != 128 && h->block != 256) { h->error = "block_threads must be 64, 128 or 256"; return fail(1); }
  if (!d.code_object_path) { h->error = "code_object_path is null"; return fail(1); }
  h->code_path = d.code_object_path;
  if (const char* wd = getenv("DOMPC_WATCHDOG_S")) h->watchdog_s = atof(wd);
  h->e_pad = ((d.n_edges + 15) / 16) * 16;
  // ---- the code object and its model info
  const int32_t in_h[5] = {d.n_opt_x, d.n_g, d.n_edges, h->e_pad, d.n_nodes};
  int64_t info[24] = {0};
  char hash[64] = {0};
  const char* const info_kernel = "dompc_model_info_kernel";
  if (h->open("IPM backend", h->code_path.c_str(), &h->module, {{"dompc_solve_kernel", &h->fn_solve, DOMPC_TWIN(dompc_hostemu_run)}},
              "code object lacks dompc kernels: " + h->code_path, info_kernel, DOMPC_TWIN(dompc_hostemu_model_info), info, hash, in_h, sizeof(in_h)))
    return fail(1);
  {
    // optional sibling `<name>_batch.hsaco` (build.py: batch_only): the same kernels compiled for "one 64-thread workgroup per problem" only
    std::string bp = h->code_path;
    const size_t dot = bp.rfind(".hsaco");
    FILE* f = nullptr;
    if (dot != std::string::npos && !getenv("DOMPC_NO_BATCH_OBJECT")) f = fopen(bp.insert(dot, "_batch").c_str(), "rb");
    if (f) {
      fclose(f);
      if (h->load(bp.c_str(), &h->module_batch, {{"dompc_solve_kernel", &h->fn_solve_batch, DOMPC_TWIN(dompc_hostemu_run)}}, "hipModuleLoad failed for " + bp))
        return fail(1);
      // The sibling is only ever launched with the general object's argument block and workspace layout: it must come from the same
      // sources and the same model (a handle with a small max_batch rebuilds only the general object after a kernel change;
      // a stale sibling with another KArgs layout would then be launched for every 64-thread batch).  A sibling that does not match is
      // not used - the general object runs those launches instead.
      int64_t info_b[24] = {0};
      char hash_b[64] = {0};
      Kernel k_info_b;
      bool same = h->find(h->module_batch, {info_kernel, &k_info_b, DOMPC_TWIN(dompc_hostemu_model_info)}) &&
                  !h->query(k_info_b, info_kernel, info_b, hash_b, in_h, sizeof(in_h));
      for (int i = 0; same && i < 24; ++i) same = info_b[i] == info[i];
      same = same && strncmp(hash, hash_b, 63) == 0;
      if (!same) {
        h->unload(h->module_batch);
        h->module_batch = nullptr;
        h->fn_solve_batch = Kernel();
        h->batch_object_stale = true;
        h->error.clear();
      }
    }
  }
#ifndef DOMPC_HOST_EMU
  if (hipHostMalloc((void**)&h->abort_word, 64, hipHostMallocMapped) != hipSuccess) { h->error = "hipHostMalloc failed"; return fail(1); }
  *h->abort_word = 0;
#else
  h->block = 1;
  h->abort_word = (int32_t*)calloc(16, sizeof(int32_t));
#endif
  const int64_t want[9] = {d.nx, d.nu, d.np, d.ntvp, d.ne, d.ns, d.M == 0 ? 0 : d.deg, d.M == 0 ? 1 : d.ni, d.M};
  if (h->check_info("", info, want, 9, 11, sizeof(dompc::KArgs), hash, d.model_hash)) return fail(1);
  h->ws_stride = info[9];
  h->sweep_block = info[10];
  for (int i = 0; i < 4; ++i) h->xlayout[i] = info[12 + i];
  h->shard_capable = info[16] != 0;
  h->el_size = info[17];
  h->edges_per_wave = info[19] > 0 ? info[19] : 1;
  h->riccati_kind = info[20];
  // ---- slots: one per workgroup the device can keep resident (occupancy of the solver kernel at this block size
  //      and LDS pool, times the number of CUs); more problems than slots are pulled from a work counter
  int max_batch = d.max_batch > 0 ? d.max_batch : 1;
  auto resident_at = [&](int block) -> int {
    int resident = 512 * (256 / block);
#ifndef DOMPC_HOST_EMU
    const size_t lds = sizeof(double) * (size_t)pool_doubles(h, block);
    int occ = 0, cus = 0;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&occ, h->fn_solve.fn, block, lds) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, d.device) == hipSuccess && occ > 0 && cus > 0)
      resident = occ * cus;
    h->occupancy = occ;
#endif
    return resident;
  };
  h->slots64 = resident_at(64);
  h->slots256 = resident_at(fit_block(h->el_size, 256));
  {
    // batches of >= BATCH_ONE_WAVE problems run one wavefront per problem and need that many more slots
    const int resident = h->block_auto ? (max_batch >= BATCH_ONE_WAVE ? h->slots64 : h->slots256) : resident_at(h->block);
    h->n_slots = d.n_slots > 0 ? d.n_slots : (max_batch < resident ? max_batch : resident);
  }
  if (const char* se = getenv("DOMPC_SLOTS")) { const int v = atoi(se); if (v >= 1) h->n_slots = v; }      // (tuning aid; nonsense values are ignored)
  if (h->n_slots < 1) h->n_slots = 1;
#ifdef DOMPC_HOST_EMU
  h->n_slots = 1;
#endif
  // ---- tables
  dompc::KArgs& A = h->base;
  memset(&A, 0, sizeof(A));
  int rc = 0;
  rc |= upload(h, &A.level_node_start, d.level_node_start, d.N + 2);
  rc |= upload(h, &A.node_level, d.node_level, d.n_nodes);
  rc |= upload(h, &A.node_x_off, d.node_x_off, d.n_nodes);
  rc |= upload(h, &A.node_u_off, d.node_u_off, d.n_nodes);
  rc |= upload(h, &A.node_eps_off, d.node_eps_off, d.n_nodes);
  rc |= upload(h, &A.node_child_start, d.node_child_start, d.n_nodes);
  rc |= upload(h, &A.node_child_count, d.node_child_count, d.n_nodes);
  rc |= upload(h, &A.node_parent, d.node_parent, d.n_nodes);
  rc |= upload(h, &A.node_in_edge, d.node_in_edge, d.n_nodes);
  rc |= upload(h, &A.edge_parent, d.edge_parent, d.n_edges);
  rc |= upload(h, &A.edge_child, d.edge_child, d.n_edges);
  rc |= upload(h, &A.edge_pidx, d.edge_pidx, d.n_edges);
  rc |= upload(h, &A.edge_w_off, d.edge_w_off, d.n_edges);
  rc |= upload(h, &A.edge_row0, d.edge_row0, d.n_edges);
  rc |= upload(h, &A.edge_level, d.edge_level, d.n_edges);
  rc |= upload(h, &A.edge_omega, d.edge_omega, d.n_edges);
  rc |= upload(h, &A.dummy_idx, d.dummy_idx, d.n_dummy);
  if (rc) return fail(1);
  {
    std::vector<int32_t> pack((size_t)d.n_edges * dompc::EP_N, 0);
    for (int e = 0; e < d.n_edges; ++e) {
      int32_t* q = pack.data() + (size_t)e * dompc::EP_N;
      const int n = d.edge_parent[e], cn = d.edge_child[e];
      q[dompc::EP_PARENT] = n; q[dompc::EP_CHILD] = cn; q[dompc::EP_LEVEL] = d.edge_level[e]; q[dompc::EP_WOFF] = d.edge_w_off[e];
      q[dompc::EP_PIDX] = d.edge_pidx[e]; q[dompc::EP_ROW0] = d.edge_row0[e];
      q[dompc::EP_XOFF_PARENT] = d.node_x_off[n]; q[dompc::EP_UOFF_PARENT] = d.node_u_off[n]; q[dompc::EP_XOFF_CHILD] = d.node_x_off[cn];
      q[dompc::EP_EPSOFF_PARENT] = d.node_eps_off ? d.node_eps_off[n] : -1;
      int64_t ob;
      memcpy(&ob, &d.edge_omega[e], sizeof ob);
      q[dompc::EP_OMEGA_LO] = (int32_t)(uint32_t)(ob & 0xffffffffll); q[dompc::EP_OMEGA_HI] = (int32_t)(uint32_t)((uint64_t)ob >> 32);
    }
    if (upload(h, &A.edge_pack, pack.data(), pack.size())) return fail(1);
  }
  {
    const int32_t nw = (int32_t)info[21];
    std::vector<int32_t> pack((size_t)d.n_nodes * dompc::NP_N, 0);
    for (int n = 0; n < d.n_nodes; ++n) {
      int32_t* q = pack.data() + (size_t)n * dompc::NP_N;
      const int ie = d.node_in_edge[n], pn = d.node_parent[n], cs = d.node_child_start[n], cc = d.node_child_count[n];
      const int c0 = cc > 0 ? d.edge_child[cs] : -1;
      q[dompc::NP_XOFF] = d.node_x_off[n]; q[dompc::NP_UOFF] = d.node_u_off[n]; q[dompc::NP_EPSOFF] = d.node_eps_off[n];
      q[dompc::NP_INEDGE] = ie; q[dompc::NP_NUROW] = ie >= 0 ? d.edge_row0[ie] + nw : 0;
      q[dompc::NP_PARENT] = pn; q[dompc::NP_UOFF_PARENT] = pn >= 0 ? d.node_u_off[pn] : -1;
      q[dompc::NP_CHILD_START] = cs; q[dompc::NP_CHILD_COUNT] = cc; q[dompc::NP_CHILD0] = c0;
      q[dompc::NP_XOFF_CHILD0] = cc > 0 ? d.node_x_off[c0] : -1; q[dompc::NP_ROW0_CHILD0] = cc > 0 ? d.edge_row0[cs] : -1;
      q[dompc::NP_LEVEL] = d.node_level[n]; q[dompc::NP_RW_EDGE] = cc > 0 ? cs : -1;
    }
    if (upload(h, &A.node_pack, pack.data(), pack.size())) return fail(1);
  }
  A.N = d.N; A.n_nodes = d.n_nodes; A.n_edges = d.n_edges; A.n_dummy = d.n_dummy;
  A.n_opt_x = d.n_opt_x; A.n_opt_p = d.n_opt_p; A.n_g = d.n_g; A.e_pad = h->e_pad;
  A.p_off_tvp = d.p_off_tvp; A.p_off_p = d.p_off_p; A.p_off_uprev = d.p_off_uprev;
  {
    // chain_level: first stage from which every node (k, s) has exactly one child, (k+1, s), over edge node_child_start[(k, 0)] + s
    // (the chain walks of the Riccati passes form these indices arithmetically)
    const int32_t* ls = desc->level_node_start;
    const int S = ls[d.N + 1] - ls[d.N];
    h->n_leaves = S > 0 ? S : 1;
    int cl = d.N;
    for (int k = d.N - 1; k >= 0; --k) {
      bool ok = (ls[k + 1] - ls[k]) == S;
      for (int s = 0; ok && s < S; ++s) {
        const int n = ls[k] + s;
        ok = desc->node_child_count[n] == 1 && desc->edge_child[desc->node_child_start[n]] == ls[k + 1] + s &&
             desc->node_child_start[n] == desc->node_child_start[ls[k]] + s;
      }
      if (!ok) break;
      cl = k;
    }
    A.chain_level = cl;
  }
  A.opt = d.opts;
  if (const char* mi = getenv("DOMPC_MAX_ITER")) A.opt.max_iter = atoi(mi);      // debugging aid
  if (const char* lf = getenv("DOMPC_LDS_FILL")) {                                 // debugging aid: "value[,lo,hi]"
    double v = 0.0; int lo = 0, hi = 1 << 30;
    sscanf(lf, "%lf,%d,%d", &v, &lo, &hi);
    A.lds_fill = v; A.lds_fill_lo = lo; A.lds_fill_hi = hi;
  }
  A.n_slots = h->n_slots;
  A.ws_stride = h->ws_stride;
#ifndef DOMPC_HOST_EMU
  {
    void* dw = nullptr;
    if (hipHostGetDevicePointer(&dw, h->abort_word, 0) != hipSuccess) { h->error = "hipHostGetDevicePointer failed"; return fail(1); }
    A.abort_flag = (const int32_t*)dw;
  }
#else
  A.abort_flag = h->abort_word;
#endif
  if (h->alloc((void**)&A.ws, sizeof(double) * (size_t)h->ws_stride * h->n_slots)) return fail(1);
  if (const char* fill = getenv("DOMPC_WS_FILL")) {      // debugging aid: poison the workspace (uninitialised reads)
    if (h->fill(A.ws, atoi(fill), sizeof(double) * (size_t)h->ws_stride * h->n_slots, h->stream_ptr())) return fail(1);
  }
  if (h->alloc((void**)&A.work_counter, 64)) return fail(1);
  A.lb_sh = A.ub_sh = nullptr;
  {
    const char* sb = getenv("DOMPC_SHARED_BOUNDS");      // (measurement aid: 0 = per-slot copies of the bounds)
    if (!sb || atoi(sb) != 0) {
      if (h->alloc((void**)&A.lb_sh, sizeof(double) * (size_t)d.n_opt_x)) return fail(1);
      if (h->alloc((void**)&A.ub_sh, sizeof(double) * (size_t)d.n_opt_x)) return fail(1);
    }
  }
  // wide mode (small batches): up to 64 slots x 32 workgroups
  if (h->alloc((void**)&A.wide_bar, sizeof(uint32_t) * dompc::WIDE_BAR_STRIDE * 64)) return fail(1);
  if (h->alloc((void**)&A.wide_flags, sizeof(int32_t) * 8 * 64)) return fail(1);
  if (h->alloc((void**)&A.wide_partials, sizeof(double) * 64 * 2 * 32 * 12)) return fail(1);
  for (int i = 0; i < 8; ++i)
    if (h->alloc((void**)&h->s_dbg[i], sizeof(double) * (size_t)(d.n_opt_x > d.n_g ? d.n_opt_x : d.n_g))) return fail(1);
  if (h->alloc((void**)&h->s_trace, sizeof(double) * 8 * h->trace_cap)) return fail(1);
  A.trace = h->s_trace; A.trace_cap = h->trace_cap;
  if (const char* xt = getenv("DOMPC_EXTRA_TRAFFIC")) A.trace_pad = atoi(xt);    // measurement aid, see sweep()
  if (h->sync()) return fail(1);
  // the description's table pointers are not valid after return
  h->d.level_node_start = nullptr;
  *out = h;
  return 0;
}

extern "C" int64_t dompc_workspace_bytes(const dompc_handle* h) { return h ? (int64_t)sizeof(double) * h->ws_stride * h->n_slots : 0; }
extern "C" int32_t dompc_num_slots(const dompc_handle* h) { return h ? h->n_slots : 0; }
extern "C" int64_t dompc_sweep_block_doubles(const dompc_handle* h) { return h ? h->sweep_block : 0; }

extern "C" int64_t dompc_exchange_doubles(const dompc_handle* h, int32_t world, int32_t n_cut) {
  if (!h || world < 1 || n_cut < 0) return 0;
  const int64_t* L = h->xlayout;
  return (int64_t)world * L[0] + (int64_t)n_cut * (L[1] + L[2] + L[3]) + 2 * (int64_t)world;
}

#ifndef DOMPC_HOST_EMU
static int rccl_open(dompc_handle* h, const char* path) {
  if (h->rccl_lib) return 0;
  h->rccl_lib = dlopen(path && *path ? path : "librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!h->rccl_lib) { h->error = std::string("dlopen(librccl) failed: ") + dlerror(); return 1; }
  h->nccl_get_unique_id = (int (*)(dompc_handle::RcclUid*))dlsym(h->rccl_lib, "ncclGetUniqueId");
  h->nccl_comm_init_rank = (int (*)(void**, int, dompc_handle::RcclUid, int))dlsym(h->rccl_lib, "ncclCommInitRank");
  h->nccl_all_reduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(h->rccl_lib, "ncclAllReduce");
  h->nccl_comm_destroy = (int (*)(void*))dlsym(h->rccl_lib, "ncclCommDestroy");
  h->nccl_error_string = (const char* (*)(int))dlsym(h->rccl_lib, "ncclGetErrorString");
  if (!h->nccl_get_unique_id || !h->nccl_comm_init_rank || !h->nccl_all_reduce || !h->nccl_comm_destroy) {
    h->error = "librccl does not export the expected nccl* entry points"; return 1;
  }
  return 0;
}
#define NCCLCHK(h, expr)                                                                                       \
  do {                                                                                                         \
    const int _r = (expr);                                                                                     \
    if (_r != 0) {                                                                                             \
      (h)->error = std::string(#expr) + ": " + ((h)->nccl_error_string ? (h)->nccl_error_string(_r) : "rccl error"); \
      return 1;                                                                                                \
    }                                                                                                          \
  } while (0)
#endif

extern "C" int dompc_rccl_unique_id(dompc_handle* h, const char* librccl_path, uint8_t id[128]) {
  if (!h || !id) return 1;
#ifndef DOMPC_HOST_EMU
  if (rccl_open(h, librccl_path)) return 1;
  dompc_handle::RcclUid u;
  NCCLCHK(h, h->nccl_get_unique_id(&u));
  memcpy(id, u.internal, 128);
  return 0;
#else
  (void)librccl_path; h->error = "no RCCL in the host emulation"; return 1;
#endif
}

extern "C" int dompc_rccl_init(dompc_handle* h, const char* librccl_path, const uint8_t id[128], int32_t rank, int32_t world) {
  if (!h || !id) return 1;
#ifndef DOMPC_HOST_EMU
  if (rccl_open(h, librccl_path)) return 1;
  HIPCHK(h, hipSetDevice(h->d.device));
  if (h->rccl_comm) { h->nccl_comm_destroy(h->rccl_comm); h->rccl_comm = nullptr; }
  dompc_handle::RcclUid u;
  memcpy(u.internal, id, 128);
  NCCLCHK(h, h->nccl_comm_init_rank(&h->rccl_comm, world, u, rank));
  if (!h->rccl_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->rccl_stream, hipStreamNonBlocking));
  return 0;
#else
  (void)librccl_path; (void)rank; (void)world; h->error = "no RCCL in the host emulation"; return 1;
#endif
}

extern "C" int dompc_set_sharding(dompc_handle* h, const dompc_shard_desc* s) {
  if (!h) return 1;
  dompc::KArgs& A = h->base;
  if (!s) {
    A.x_mask = A.g_mask = A.e_mask = A.n_mask = nullptr; A.node_cut = nullptr;
    A.n_cut = 0; A.cut_level = 0; A.shard_rank = 0; A.shard_world = 1; A.xbuf = nullptr; A.xbuf_len = 0;
    A.x_callback = nullptr; A.x_ctx = nullptr;
    h->sharded = false;
    return 0;
  }
  const dompc_problem_desc& d = h->d;
  if (!h->shard_capable) { h->error = "this code object was built without tree-sharding support (-DDOMPC_SHARD=1)"; return 1; }
  if (s->world < 1 || s->rank < 0 || s->rank >= s->world || s->cut_level < 1 || s->n_cut < 1) { h->error = "invalid shard description"; return 1; }
  if (!s->x_mask || !s->g_mask || !s->edge_mask || !s->node_mask || !s->node_cut || !s->xbuf) { h->error = "null pointer in shard description"; return 1; }
#ifndef DOMPC_HOST_EMU
  if (!s->allreduce && !h->rccl_comm) { h->error = "no collective: pass allreduce or call dompc_rccl_init first"; return 1; }
#else
  if (!s->allreduce) { h->error = "the host emulation needs an allreduce callback"; return 1; }
#endif
  if (h->set_device()) return 1;
  if (s->xbuf_doubles < dompc_exchange_doubles(h, s->world, s->n_cut)) { h->error = "exchange buffer too small (dompc_exchange_doubles)"; return 1; }
  int rc = 0;
  rc |= upload(h, &A.x_mask, s->x_mask, d.n_opt_x);
  rc |= upload(h, &A.g_mask, s->g_mask, d.n_g);
  rc |= upload(h, &A.e_mask, s->edge_mask, d.n_edges);
  rc |= upload(h, &A.n_mask, s->node_mask, d.n_nodes);
  rc |= upload(h, &A.node_cut, s->node_cut, d.n_nodes);
  if (rc) return 1;
  A.n_cut = s->n_cut; A.cut_level = s->cut_level; A.shard_rank = s->rank; A.shard_world = s->world;
  A.xbuf = s->xbuf; A.xbuf_len = (int32_t)dompc_exchange_doubles(h, s->world, s->n_cut);
  h->allreduce = s->allreduce; h->allreduce_ctx = s->ctx;
#ifndef DOMPC_HOST_EMU
  if (!h->x_words) {
    HIPCHK(h, hipHostMalloc((void**)&h->x_words, 64, hipHostMallocMapped));
    memset(h->x_words, 0, 64);
  }
  if (!h->shard_stream) {
    // The resident solver kernel of a sharded solve waits for collectives (RCCL kernels on the caller's streams).
    // Streams of different priorities never share a hardware queue, so it runs on its own lowest-priority stream
    // and the collective is never queued behind the kernel that is waiting for it.
    int least = 0, greatest = 0;
    HIPCHK(h, hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIPCHK(h, hipStreamCreateWithPriority(&h->shard_stream, hipStreamNonBlocking, least));
  }
  void* dw = nullptr;
  HIPCHK(h, hipHostGetDevicePointer(&dw, h->x_words, 0));
  A.x_req = (volatile uint32_t*)dw; A.x_ack = (volatile uint32_t*)dw + 1; A.x_count = (volatile uint32_t*)dw + 2;
  A.x_callback = nullptr; A.x_ctx = nullptr;
#else
  A.x_callback = s->allreduce; A.x_ctx = s->ctx;
#endif
  if (h->sync()) return 1;
  h->sharded = true;
  return 0;
}

#ifndef DOMPC_HOST_EMU
// Host side of the exchange handshake (Thr::xchg): serve the kernel's requests until it has finished.
static int serve_exchanges(dompc_handle* h, hipStream_t st) {
  hipEvent_t done;
  HIPCHK(h, hipEventCreateWithFlags(&done, hipEventDisableTiming));
  HIPCHK(h, hipEventRecord(done, st));
  volatile uint32_t* w = h->x_words;
  uint32_t served = 0;
  int rc = 0;
  const auto t0 = std::chrono::steady_clock::now();
  bool raised = false;
  unsigned polls = 0;
  while (true) {
    if ((++polls & 0xfffu) == 0) {               // watchdog (see dev_sync_watchdog)
      const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (!raised && dt > h->watchdog_s) { int32_t z_ = 0; __atomic_compare_exchange_n(h->abort_word, &z_, 1, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE); raised = true; }   // (0 -> 1: a user's request, 2, is left alone)
      if (raised && dt > h->watchdog_s + 30.0) { h->error = "watchdog: the sharded solve did not finish"; rc = 1; break; }
    }
    const uint32_t r = w[0];
    if (r != served) {
      __sync_synchronize();
      const uint32_t count = w[2], off = w[3];
      if ((int64_t)off + count > h->base.xbuf_len) { h->error = "exchange request outside the buffer"; rc = 1; w[1] = r; served = r; continue; }
      if (h->allreduce) {
        h->allreduce(h->allreduce_ctx, h->base.xbuf + off, (int32_t)count);
      } else {                                   // native RCCL: in-place sum of doubles (ncclFloat64 = 8, ncclSum = 0)
        double* buf = h->base.xbuf + off;
        const int e1 = h->nccl_all_reduce(buf, buf, (size_t)count, 8, 0, h->rccl_comm, h->rccl_stream);
        if (e1 != 0 || hipStreamSynchronize(h->rccl_stream) != hipSuccess) { h->error = "ncclAllReduce failed in the exchange loop"; rc = 1; }
      }
      served = r;
      __sync_synchronize();
      w[1] = r;
    } else {
      const hipError_t q = hipEventQuery(done);
      if (q == hipSuccess) break;
      if (q != hipErrorNotReady) { h->error = std::string("sharded solve: ") + hipGetErrorString(q); rc = 1; break; }
    }
  }
  hipEventDestroy(done);
  if (raised) { int32_t expect = 1; __atomic_compare_exchange_n(h->abort_word, &expect, 0, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE); }
  h->n_exchanges = (int64_t)served;             // (the kernel numbers its requests 1, 2, ...: the last one served = their count)
  return rc;
}
#endif

extern "C" int64_t dompc_last_exchange_count(const dompc_handle* h) { return h ? h->n_exchanges : 0; }

extern "C" int dompc_edges_per_wavefront(const dompc_handle* h) { return h ? (int)h->edges_per_wave : 0; }
extern "C" int dompc_riccati_kind(const dompc_handle* h) { return h ? (int)h->riccati_kind : 0; }
extern "C" int dompc_batch_object_state(const dompc_handle* h) {
  if (!h) return -1;
  if (h->fn_solve_batch) return 1;
  return h->batch_object_stale ? 2 : 0;
}

extern "C" int dompc_solve_batch_device(dompc_handle* h, int32_t B, const double* x0, const double* lbx, const double* ubx,
                                        const double* lbg, const double* ubg, const double* p, double* x, double* g,
                                        double* lam_x, double* lam_g, double* f, dompc_stats* stats, void* stream) {
  if (!h) return 1;
  if (B <= 0) return 0;
  if (!x0 || !lbx || !ubx || !lbg || !ubg || !p) { h->error = "null input pointer"; return 1; }
  if (h->set_device()) return 1;
  dompc::KArgs A = h->base;
  A.x0 = x0; A.lbx = lbx; A.ubx = ubx; A.lbg = lbg; A.ubg = ubg; A.p = p;
  A.x_out = x; A.g_out = g; A.lam_x_out = lam_x; A.lam_g_out = lam_g; A.f_out = f; A.stats = stats;
  A.batch = B; A.mode = 0;
  if (h->sharded) {
    if (B != 1) { h->error = "a sharded handle solves one problem per call"; return 1; }
#ifndef DOMPC_HOST_EMU
    if (!stream) { h->error = "sharded solve needs a non-blocking stream (not the default stream)"; return 1; }
    h->x_words[0] = h->x_words[1] = h->x_words[2] = h->x_words[3] = 0;
#endif
  }
#ifndef DOMPC_HOST_EMU
  const dompc_shape s = dompc_launch::solve_shape(shape_facts(h), shape_overrides(), B);
  if (s.wide > 1 && (h->fill(A.wide_bar, 0, sizeof(uint32_t) * dompc::WIDE_BAR_STRIDE * 64, stream) ||
                     h->fill(A.wide_flags, 0, sizeof(int32_t) * 8 * 64, stream)))
    return 1;
#else
  const dompc_shape s = dompc_launch::batch_shape(shape_facts(h), B);      // (a workgroup is the calling thread: grid and block are ignored)
#endif
  A.wide = s.wide;
  A.wide_spread = s.wide_spread;
  if (launch(h, A, s.grid, s.block, stream)) return 1;
#ifndef DOMPC_HOST_EMU
  if (h->sharded) return serve_exchanges(h, (hipStream_t)stream);
#endif
  return 0;
}

extern "C" int dompc_solve_batch(dompc_handle* h, int32_t B, const double* x0, const double* lbx, const double* ubx,
                                 const double* lbg, const double* ubg, const double* p, double* x, double* g,
                                 double* lam_x, double* lam_g, double* f, dompc_stats* stats) {
  if (!h) return 1;
  if (B <= 0) return 0;
  if (!x0 || !lbx || !ubx || !lbg || !ubg || !p) { h->error = "null input pointer"; return 1; }
  auto t0 = std::chrono::steady_clock::now();
  if (h->set_device()) return 1;
  const dompc_problem_desc& d = h->d;
  if (ensure_staging(h, B)) return 1;
  int rc = 0;
  rc |= h->h2d(h->s_x0, x0, sizeof(double) * (size_t)B * d.n_opt_x);
  rc |= h->h2d(h->s_p, p, sizeof(double) * (size_t)B * d.n_opt_p);
  rc |= h->h2d(h->s_lbx, lbx, sizeof(double) * d.n_opt_x);
  rc |= h->h2d(h->s_ubx, ubx, sizeof(double) * d.n_opt_x);
  rc |= h->h2d(h->s_lbg, lbg, sizeof(double) * d.n_g);
  rc |= h->h2d(h->s_ubg, ubg, sizeof(double) * d.n_g);
  if (rc) return 1;
  static const bool timing = getenv("DOMPC_TIMING") != nullptr;       // measurement aid: where the wall time of a host-buffer call goes (stderr)
  auto t1 = std::chrono::steady_clock::now();
  if (h->sharded && h->sync()) return 1;      // the sharded solve runs on its own stream: inputs must have landed
  if (dompc_solve_batch_device(h, B, h->s_x0, h->s_lbx, h->s_ubx, h->s_lbg, h->s_ubg, h->s_p, h->s_x, h->s_g, h->s_lamx,
                               h->s_lamg, h->s_f, h->s_stats, own_stream(h)))
    return 1;
#ifndef DOMPC_HOST_EMU
  // wait here (bounded by the watchdog) before the result copies are queued behind the kernel
  auto t2 = std::chrono::steady_clock::now();
  if (!h->sharded && dev_sync_watchdog(h, h->stream, (B + h->n_slots - 1) / (h->n_slots > 0 ? h->n_slots : 1))) return 1;
#else
  auto t2 = std::chrono::steady_clock::now();
#endif
  auto t3 = std::chrono::steady_clock::now();
  if (x) rc |= h->d2h(x, h->s_x, sizeof(double) * (size_t)B * d.n_opt_x);
  if (g) rc |= h->d2h(g, h->s_g, sizeof(double) * (size_t)B * d.n_g);
  if (lam_x) rc |= h->d2h(lam_x, h->s_lamx, sizeof(double) * (size_t)B * d.n_opt_x);
  if (lam_g) rc |= h->d2h(lam_g, h->s_lamg, sizeof(double) * (size_t)B * d.n_g);
  if (f) rc |= h->d2h(f, h->s_f, sizeof(double) * (size_t)B);
  if (stats) rc |= h->d2h(stats, h->s_stats, sizeof(dompc_stats) * (size_t)B);
  if (rc || h->sync()) return 1;
  if (timing) {
    auto t4 = std::chrono::steady_clock::now();
    auto us = [](auto a, auto b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
    fprintf(stderr, "[dompc timing] B=%d  inputs queued %.0f us | launch call %.0f us | wait for the kernel %.0f us | results copied %.0f us\n",
            (int)B, us(t0, t1), us(t1, t2), us(t2, t3), us(t3, t4));
  }
  if (stats) {
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int b = 0; b < B; ++b) stats[b].t_wall_total = dt;
  }
  return 0;
}

extern "C" int dompc_solve(dompc_handle* h, const double* x0, const double* lbx, const double* ubx, const double* lbg,
                           const double* ubg, const double* p, const double* /*lam_x0*/, const double* /*lam_g0*/,
                           double* x, double* g, double* lam_x, double* lam_g, double* f, dompc_stats* stats) {
  return dompc_solve_batch(h, 1, x0, lbx, ubx, lbg, ubg, p, x, g, lam_x, lam_g, f, stats);
}

extern "C" int dompc_sweep_batch_device(dompc_handle* h, int32_t B, const double* x, const double* lam, const double* p,
                                        double* g, double* blocks, void* stream) {
  if (!h) return 1;
  if (B <= 0) return 0;
  if (!x || !lam || !p || !g) { h->error = "null pointer"; return 1; }      // (blocks may be null: residuals only - the timing of the sweep itself, bench.py)
  if (h->set_device()) return 1;
  dompc::KArgs A = h->base;
  A.p = p; A.sw_x = x; A.sw_lam = lam; A.sw_g = g; A.sw_blocks = blocks;
  A.batch = B; A.mode = 2;
  // (same launch shape as a solve of that many problems: one 64-thread workgroup per iterate from BATCH_ONE_WAVE on)
  const dompc_shape s = dompc_launch::batch_shape(shape_facts(h), B);
  return launch(h, A, s.grid, s.block, stream);
}

static int newton_step_impl(dompc_handle* h, const double* x, const double* lam_g, const double* zl,
                            const double* zu, const double* lbx, const double* ubx, const double* lbg,
                            const double* ubg, const double* p, double mu, double delta_w, double* dx,
                            double* dlam, double* rd, double* c, int at_solution) {
  if (!h) return 1;
  if (h->set_device()) return 1;
  const dompc_problem_desc& d = h->d;
  if (h->sharded) { h->error = "dompc_debug_newton_step is not available on a sharded handle (call dompc_set_sharding(h, NULL) first)"; return 1; }
  if (ensure_staging(h, 1)) return 1;
  int rc = 0;
  rc |= h->h2d(h->s_x0, x, sizeof(double) * d.n_opt_x);
  rc |= h->h2d(h->s_p, p, sizeof(double) * d.n_opt_p);
  rc |= h->h2d(h->s_lbx, lbx, sizeof(double) * d.n_opt_x);
  rc |= h->h2d(h->s_ubx, ubx, sizeof(double) * d.n_opt_x);
  rc |= h->h2d(h->s_lbg, lbg, sizeof(double) * d.n_g);
  rc |= h->h2d(h->s_ubg, ubg, sizeof(double) * d.n_g);
  rc |= h->h2d(h->s_dbg[0], lam_g, sizeof(double) * d.n_g);
  rc |= h->h2d(h->s_dbg[1], zl, sizeof(double) * d.n_opt_x);
  rc |= h->h2d(h->s_dbg[2], zu, sizeof(double) * d.n_opt_x);
  if (rc) return 1;
  dompc::KArgs A = h->base;
  A.x0 = h->s_x0; A.lbx = h->s_lbx; A.ubx = h->s_ubx; A.lbg = h->s_lbg; A.ubg = h->s_ubg; A.p = h->s_p;
  A.dbg_lam = h->s_dbg[0]; A.dbg_zl = h->s_dbg[1]; A.dbg_zu = h->s_dbg[2];
  A.dbg_dx = h->s_dbg[3]; A.dbg_dlam = h->s_dbg[4]; A.dbg_rd = h->s_dbg[5]; A.dbg_c = h->s_dbg[6];
  A.dbg_mu = mu; A.dbg_delta = delta_w;
  A.batch = 1; A.mode = 1; A.dbg_at_solution = at_solution;
  if (launch(h, A, 1, fit_block(h->el_size, 256), h->stream_ptr())) return 1;
  if (dx) rc |= h->d2h(dx, h->s_dbg[3], sizeof(double) * d.n_opt_x);
  if (dlam) rc |= h->d2h(dlam, h->s_dbg[4], sizeof(double) * d.n_g);
  if (rd) rc |= h->d2h(rd, h->s_dbg[5], sizeof(double) * d.n_opt_x);
  if (c) rc |= h->d2h(c, h->s_dbg[6], sizeof(double) * d.n_g);
  if (rc || h->sync()) return 1;
  return 0;
}

extern "C" int dompc_debug_newton_step(dompc_handle* h, const double* x, const double* lam_g, const double* zl,
                                       const double* zu, const double* lbx, const double* ubx, const double* lbg,
                                       const double* ubg, const double* p, double mu, double delta_w, double* dx,
                                       double* dlam, double* rd, double* c) {
  return newton_step_impl(h, x, lam_g, zl, zu, lbx, ubx, lbg, ubg, p, mu, delta_w, dx, dlam, rd, c, 0);
}
extern "C" int dompc_newton_step_at_solution(dompc_handle* h, const double* x, const double* lam_g, const double* zl,
                                             const double* zu, const double* lbx, const double* ubx, const double* lbg,
                                             const double* ubg, const double* p, double mu, double* dx, double* dlam) {
  return newton_step_impl(h, x, lam_g, zl, zu, lbx, ubx, lbg, ubg, p, mu, 0.0, dx, dlam, nullptr, nullptr, 1);
}

// B parameter vectors at ONE point (dompc_ipm.h): one launch per chunk of resident slots, one workgroup per vector
extern "C" int dompc_newton_steps_at_solution(dompc_handle* h, int32_t B, const double* x, const double* lam_g, const double* zl,
                                              const double* zu, const double* lbx, const double* ubx, const double* lbg,
                                              const double* ubg, const double* p, double mu, double* dx, double* dlam) {
  if (!h || B < 1) return 1;
  if (h->set_device()) return 1;
  const dompc_problem_desc& d = h->d;
  if (h->sharded) { h->error = "dompc_newton_steps_at_solution is not available on a sharded handle"; return 1; }
  int chunk = h->n_slots < B ? h->n_slots : B;
#ifdef DOMPC_HOST_EMU
  chunk = B;
#endif
  if (chunk < 1) chunk = 1;
  if (ensure_staging(h, chunk)) return 1;
  int rc = 0;
  rc |= h->h2d(h->s_x0, x, sizeof(double) * d.n_opt_x);
  rc |= h->h2d(h->s_lbx, lbx, sizeof(double) * d.n_opt_x);
  rc |= h->h2d(h->s_ubx, ubx, sizeof(double) * d.n_opt_x);
  rc |= h->h2d(h->s_lbg, lbg, sizeof(double) * d.n_g);
  rc |= h->h2d(h->s_ubg, ubg, sizeof(double) * d.n_g);
  rc |= h->h2d(h->s_dbg[0], lam_g, sizeof(double) * d.n_g);
  rc |= h->h2d(h->s_dbg[1], zl, sizeof(double) * d.n_opt_x);
  rc |= h->h2d(h->s_dbg[2], zu, sizeof(double) * d.n_opt_x);
  if (rc) return 1;
  for (int b0 = 0; b0 < B; b0 += chunk) {
    const int nb = (B - b0 < chunk) ? B - b0 : chunk;
    if (h->h2d(h->s_p, p + (size_t)b0 * d.n_opt_p, sizeof(double) * (size_t)nb * d.n_opt_p)) return 1;
    dompc::KArgs A = h->base;
    A.x0 = h->s_x0; A.lbx = h->s_lbx; A.ubx = h->s_ubx; A.lbg = h->s_lbg; A.ubg = h->s_ubg; A.p = h->s_p;
    A.dbg_lam = h->s_dbg[0]; A.dbg_zl = h->s_dbg[1]; A.dbg_zu = h->s_dbg[2];
    A.dbg_dx = h->s_x; A.dbg_dlam = h->s_lamg; A.dbg_rd = h->s_lamx; A.dbg_c = h->s_g;        // (batch staging buffers: nb rows each)
    A.dbg_mu = mu; A.dbg_delta = 0.0;
    A.batch = nb; A.mode = 1; A.dbg_at_solution = 1;
    if (launch(h, A, nb, fit_block(h->el_size, 256), h->stream_ptr())) return 1;
    rc |= h->d2h(dx + (size_t)b0 * d.n_opt_x, h->s_x, sizeof(double) * (size_t)nb * d.n_opt_x);
    rc |= h->d2h(dlam + (size_t)b0 * d.n_g, h->s_lamg, sizeof(double) * (size_t)nb * d.n_g);
    if (rc || h->sync()) return 1;
  }
  return 0;
}

// Sensitivities at B points (dompc_ipm.h).  Three launches per chunk of points on `stream`: the parameter rows of the plan, the Newton
// directions (work items points x rows, pulled from the device-wide counter by one workgroup per workspace slot), the difference quotients.
// A chunk is as many points as the work buffer holds (rows of parameters and of selected direction entries).
extern "C" int dompc_sens_batch_device(dompc_handle* h, int32_t B, const double* x, const double* lam_g, const double* mu, const double* p,
                                       const double* lbx, const double* ubx, const double* lbg, const double* ubg, const int32_t* sel,
                                       int32_t n_sel, const int32_t* row_plan, int32_t n_rows, const int32_t* col_plan, int32_t n_cols,
                                       double fd_step, int32_t flags, double active_set_tol, double* S, double* residual_step,
                                       int32_t* ok, void* stream) {
  if (!h) return 1;
  if (B <= 0) return 0;
  if (!x || !lam_g || !mu || !p || !lbx || !ubx || !lbg || !ubg || !sel || !row_plan || !col_plan || !S || !residual_step || !ok) { h->error = "null pointer"; return 1; }
  if (n_sel < 1 || n_rows < 1 || n_cols < 1) { h->error = "dompc_sens_batch_device: empty selection or plan"; return 1; }
  if (h->set_device()) return 1;
  if (h->sharded) { h->error = "dompc_sens_batch_device is not available on a sharded handle"; return 1; }
  const dompc_problem_desc& d = h->d;
  if (!h->fn_sens) {
    Kernel f0;
    if (!h->find(h->module, {"dompc_sens_kernel", &f0, DOMPC_TWIN(dompc_hostemu_run)}) ||
        !h->find(h->module, {"dompc_sens_prep_kernel", &h->fn_sens_prep, DOMPC_TWIN(dompc_hostemu_sens_prep)}) ||
        !h->find(h->module, {"dompc_sens_finish_kernel", &h->fn_sens_finish, DOMPC_TWIN(dompc_hostemu_sens_finish)})) {
      h->error = "code object lacks the sensitivity kernels: " + h->code_path;
      return 1;
    }
    if (h->fn_solve_batch && !h->find(h->module_batch, {"dompc_sens_kernel", &h->fn_sens_batch, DOMPC_TWIN(dompc_hostemu_run)})) h->fn_sens_batch = Kernel();
    h->fn_sens = f0;
  }
  // work buffer: per point n_rows x (n_opt_p + n_sel) doubles; at most 32 Mi doubles (256 MiB) unless one point needs more
  const int64_t per_point = (int64_t)n_rows * (d.n_opt_p + n_sel);
  const int64_t cap_doubles = (int64_t)32 << 20;
  int64_t chunk = cap_doubles / per_point;
  if (chunk < 1) chunk = 1;
  if (chunk > B) chunk = B;
  if ((int64_t)chunk * n_rows > (int64_t)1 << 30) chunk = ((int64_t)1 << 30) / n_rows;      // (work items are 32-bit)
  if (chunk * per_point > h->sn_work_doubles) {
    double* old = h->sn_work;
    h->sn_work = nullptr; h->sn_work_doubles = 0;
    h->release(old);
    if (h->alloc((void**)&h->sn_work, sizeof(double) * (size_t)(chunk * per_point))) return 1;
    h->sn_work_doubles = chunk * per_point;
  }
  for (int64_t q0 = 0; q0 < B; q0 += chunk) {
    const int nq = (int)(B - q0 < chunk ? B - q0 : chunk);
    dompc::KArgs A = h->base;
    A.lb_sh = A.ub_sh = nullptr;           // per-slot bounds: with the active-set reduction every point has its own
    A.lbx = lbx; A.ubx = ubx; A.lbg = lbg; A.ubg = ubg;
    A.sn_x = x + q0 * d.n_opt_x; A.sn_lam = lam_g + q0 * d.n_g; A.sn_mu = mu + q0; A.sn_p = p + q0 * d.n_opt_p;
    A.sn_sel = sel; A.sn_nsel = n_sel; A.sn_rows = row_plan; A.sn_R = n_rows; A.sn_cols = col_plan; A.sn_ncols = n_cols;
    A.sn_flags = flags; A.sn_tol = active_set_tol; A.sn_fd_step = fd_step;
    A.sn_prow = h->sn_work; A.sn_D = h->sn_work + (int64_t)nq * n_rows * d.n_opt_p;
    A.p = A.sn_prow;
    A.sn_S = S + q0 * n_sel * n_cols; A.sn_res = residual_step + q0; A.sn_ok = ok + q0;
    A.batch = nq * n_rows; A.mode = 3; A.wide = 1; A.wide_spread = 0;
    const dompc_shape s = dompc_launch::batch_shape(shape_facts(h), A.batch);
    auto blocks_for = [](int64_t n) { const int64_t g = (n + 255) / 256; return (unsigned)(g < 1 ? 1 : (g > 65536 ? 65536 : g)); };
    if (h->run(h->fn_sens_prep, blocks_for((int64_t)A.batch * d.n_opt_p), 256, 0, stream, &A, sizeof(A))) return 1;
    if (launch(h, A, s.grid, s.block, stream, (s.block == 64 && h->fn_sens_batch) ? h->fn_sens_batch : h->fn_sens)) return 1;
    if (h->run(h->fn_sens_finish, blocks_for((int64_t)nq * n_sel * n_cols), 256, 0, stream, &A, sizeof(A))) return 1;
  }
  return 0;
}

// host-pointer twin: stages the points through the staging buffers of the solver and waits for the result
extern "C" int dompc_sens_batch(dompc_handle* h, int32_t B, const double* x, const double* lam_g, const double* mu, const double* p,
                                const double* lbx, const double* ubx, const double* lbg, const double* ubg, const int32_t* sel,
                                int32_t n_sel, const int32_t* row_plan, int32_t n_rows, const int32_t* col_plan, int32_t n_cols,
                                double fd_step, int32_t flags, double active_set_tol, double* S, double* residual_step, int32_t* ok) {
  if (!h) return 1;
  if (B <= 0) return 0;
  if (!x || !lam_g || !mu || !p || !lbx || !ubx || !lbg || !ubg || !sel || !row_plan || !col_plan || !S || !residual_step || !ok) { h->error = "null pointer"; return 1; }
  if (n_sel < 1 || n_rows < 1 || n_cols < 1) { h->error = "dompc_sens_batch: empty selection or plan"; return 1; }
  if (h->set_device()) return 1;
  if (h->sharded) { h->error = "dompc_sens_batch is not available on a sharded handle"; return 1; }
  const dompc_problem_desc& d = h->d;
  const size_t D = sizeof(double);
  if (ensure_staging(h, B)) return 1;
  if (B > h->sn_cap_batch) {
    if (h->sync()) return 1;
    if (h->grow_staging(&h->sn_cap_batch, B, {{(void**)&h->s_sn_mu, D}, {(void**)&h->s_sn_res, D}, {(void**)&h->s_sn_ok, sizeof(int32_t)}})) return 1;
  }
  const int64_t nS = (int64_t)B * n_sel * n_cols, nT = (int64_t)n_sel + 2 * (int64_t)n_rows + 3 * (int64_t)n_cols;
  if (nS > h->sn_cap_S) {
    if (h->sync()) return 1;
    double* old = h->s_sn_S; h->s_sn_S = nullptr; h->sn_cap_S = 0; h->release(old);
    if (h->alloc((void**)&h->s_sn_S, D * (size_t)nS)) return 1;
    h->sn_cap_S = nS;
  }
  if (nT > h->sn_cap_tab) {
    if (h->sync()) return 1;
    int32_t* old = h->s_sn_tab; h->s_sn_tab = nullptr; h->sn_cap_tab = 0; h->release(old);
    if (h->alloc((void**)&h->s_sn_tab, sizeof(int32_t) * (size_t)nT)) return 1;
    h->sn_cap_tab = nT;
  }
  int32_t* t_sel = h->s_sn_tab, *t_rows = t_sel + n_sel, *t_cols = t_rows + 2 * n_rows;
  int rc = 0;
  rc |= h->h2d(h->s_x, x, D * (size_t)B * d.n_opt_x);
  rc |= h->h2d(h->s_lamg, lam_g, D * (size_t)B * d.n_g);
  rc |= h->h2d(h->s_sn_mu, mu, D * (size_t)B);
  rc |= h->h2d(h->s_p, p, D * (size_t)B * d.n_opt_p);
  rc |= h->h2d(h->s_lbx, lbx, D * d.n_opt_x);
  rc |= h->h2d(h->s_ubx, ubx, D * d.n_opt_x);
  rc |= h->h2d(h->s_lbg, lbg, D * d.n_g);
  rc |= h->h2d(h->s_ubg, ubg, D * d.n_g);
  rc |= h->h2d(t_sel, sel, sizeof(int32_t) * (size_t)n_sel);
  rc |= h->h2d(t_rows, row_plan, sizeof(int32_t) * 2 * (size_t)n_rows);
  rc |= h->h2d(t_cols, col_plan, sizeof(int32_t) * 3 * (size_t)n_cols);
  if (rc) return 1;
  if (dompc_sens_batch_device(h, B, h->s_x, h->s_lamg, h->s_sn_mu, h->s_p, h->s_lbx, h->s_ubx, h->s_lbg, h->s_ubg, t_sel, n_sel, t_rows, n_rows,
                              t_cols, n_cols, fd_step, flags, active_set_tol, h->s_sn_S, h->s_sn_res, h->s_sn_ok, h->stream_ptr()))
    return 1;
  rc |= h->d2h(S, h->s_sn_S, D * (size_t)nS);
  rc |= h->d2h(residual_step, h->s_sn_res, D * (size_t)B);
  rc |= h->d2h(ok, h->s_sn_ok, sizeof(int32_t) * (size_t)B);
  if (rc || h->sync()) return 1;
  return 0;
}

// Iteration trace of problem 0 of the last solve call: rows of 8 doubles
// (it, mu, E0, inf_pr, inf_du, +-alpha (negative = line search failed), delta_w, obj).
extern "C" int dompc_debug_get_trace(dompc_handle* h, double* out, int32_t max_rows) {
  if (!h || !out) return 1;
  int rows = max_rows < h->trace_cap ? max_rows : h->trace_cap;
  if (h->d2h(out, h->s_trace, sizeof(double) * 8 * (size_t)rows) || h->sync()) return 1;
  return 0;
}
