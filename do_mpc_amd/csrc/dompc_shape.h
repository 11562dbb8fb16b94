// dompc_shape.h - the launch shape of the solver kernel (threads per workgroup, grid, workgroups per problem in the wide mode and
// whether they are spread over the XCDs) as pure functions of plain values: the one place where it is decided.  dompc_runtime.cpp
// fills the facts from a handle and the overrides from the environment; dompc_launch_shape (include/dompc_ipm.h) exports the
// decision without a handle, in both build flavours, and tests/test_launch_shape.py pins it on a CPU.
// Host only - no HIP header, no build flavour, no environment, no handle.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/dompc_ipm.h"

namespace dompc_launch {

static const int BATCH_ONE_WAVE = 4096;     // batch size from which a problem gets one wavefront instead of four (see dompc_create)

// largest workgroup size <= `block` whose LDS pool (one edge working set of `el_size` doubles per wavefront) fits the 160 KiB of a
// CU - models with a large dense edge working set (DAE path: 45 kB per wavefront for the double inverted pendulum) run with fewer
// wavefronts per workgroup
inline int fit_block(int64_t el_size, int block) {
  const int64_t lds_max = 160 * 1024 - 4096;                     // (static LDS of the kernel: filter, flags, counters)
  while (block > 64 && (int64_t)(block / 64) * el_size * (int64_t)sizeof(double) > lds_max) block /= 2;
  return block;
}

// One workgroup per item, as many as stay resident: the shape of a batch of `n_items` problems (solve), iterates (sweep) or
// Newton directions (sensitivities).  One 64-thread workgroup per item from BATCH_ONE_WAVE on.
inline dompc_shape batch_shape(const dompc_shape_facts& f, int n_items) {
  const int block = fit_block(f.el_size, f.block_auto ? (n_items >= BATCH_ONE_WAVE ? 64 : 256) : f.block);
  const int cap = (f.block_auto && block != 64 && f.slots256 < f.n_slots) ? f.slots256 : f.n_slots;   // resident workgroups at this block size
  return dompc_shape{block, n_items < cap ? n_items : cap, 1, 0};
}

// The shape of dompc_solve_batch_device for B >= 1 problems.
inline dompc_shape solve_shape(const dompc_shape_facts& f, const dompc_shape_overrides& o, int B) {
  dompc_shape s = batch_shape(f, B);
  const bool wenv = o.wide >= 0, senv = o.wide_spread >= 0;
  // small batches: several workgroups per problem so that one make_step can use many CUs
  // enough workgroups that every wavefront owns about two edges, fewer when the batch itself fills the chip
  // (measured on MI355X, single cold industrial_poly step, round-2 kernels: K = 4 / 8 / 16 / 32 -> 27.1 / 23.4 / 22.6 / 26.0 ms;
  //  CSTR 9.1 / - / 8.3 / 10.2 ms - the device-scope barriers grow with K faster than the phases shrink)
  int K = wenv ? o.wide : (B <= 8 ? 16 : (B <= 32 ? 8 : (B <= 64 ? 4 : 1)));
  if (!wenv && K > f.n_edges / 8) K = f.n_edges / 8 > 1 ? f.n_edges / 8 : 1;
  // Whole-chip placement (KArgs::wide_spread): the K workgroups of a problem are consecutive blocks, which the dispatcher spreads over
  // all XCDs, instead of K blocks of ONE XCD (<= 32 CUs); the device-scope barrier then keeps its L2 write-back (xcd_census sees the
  // placement).  One problem alone always runs this way: measured on MI355X (tools/gpu_wide_spread.py, profiles/r05_wide_spread.txt) the
  // 243-leaf tree of BASELINE configs[4] (4 008 edges) takes 72.3 ms with K = 32 on one XCD, 67.4 ms with the same K spread and
  // 49.7 / 48.9 / 49.3 / 55.6 / 63.8 ms with K = 64 / 96 / 128 / 192 / 256; the shipped 9-scenario problem (180 edges) 19.1 ms with 16
  // workgroups of one XCD and 18.2 / 18.0 / 18.8 ms with 16 / 24 / 32 spread - the barriers grow with K, the phases shrink with
  // sqrt-like returns: K ~ 12 sqrt(edges / 45).  DOMPC_WIDE_SPREAD=0/1 and DOMPC_WIDE override.
  int auto_block = 256;
  bool spread = senv ? o.wide_spread != 0 : (!f.sharded && (B == 1 || (B <= 4 && f.n_edges >= 2048)));
  if (spread && !wenv) {
    // Round 6 (tools/gpu_b1_k_sweep.sh, tools/gpu_tree_k_sweep.sh; the phases got faster, the barriers did not): the 180-edge problem
    // 24.7 / 22.8 / 22.9 / 23.1 / 23.5 / 24.0 / 25.7 ms (84 iterations) with K = 8 / 12 / 16 / 20 / 24 / 32 / 48, the 243-leaf tree 53.8 /
    // 49.5 / 38.9 / 39.5 / 39.6 / 39.8 / 40.1 ms with K = 32 / 48 / 64 / 80 / 96 / 112 / 128 - K ~ 6.4 sqrt(edges / 45) in steps of four,
    // and at least one wavefront per scenario chain (four wavefronts per workgroup): below that some wavefronts walk two chains of the
    // Riccati passes one after the other - the step between K = 48 and 64 on the tree.
    int Ks = 4 * (int)lround(1.6 * sqrt((double)f.n_edges / 45.0));
    if (4 * Ks < f.n_leaves) Ks = 4 * ((f.n_leaves + 15) / 16);
    // ... and for the small problems on the four-edge sweep two wavefronts per workgroup instead of four, twice the workgroups
    // (tools/gpu_b1_block_sweep.sh: the 180-edge problem 22.6 ms with 12 x 256 threads, 21.3 ms with 24 x 128 - 48 wavefronts either way,
    // one quad of edges each; 20 x 128: 22.6, 28 x 128: 21.7, 32 x 128: 21.7, 32 x 64: 23.2; the tree prefers 64 x 256: 38.9 against 42.6 ms
    // with 128 x 128 - there the barrier grows with the workgroups)
    if (f.edges_per_wave == 4 && Ks <= 16 && !o.wide_block) { auto_block = 128; Ks *= 2; }
    if (Ks > f.n_edges / 7) Ks = f.n_edges / 7;
    if (Ks > 256 / B) Ks = 256 / B;
    // (fewer than eight workgroups: the problem is too small for the whole chip - its few workgroups stay on one XCD with the light
    //  barrier; measured: CSTR nominal, 20 edges, 4.9 ms on one XCD against 5.6 ms with its two workgroups on two XCDs)
    if (Ks >= 8 || senv) K = Ks < 1 ? 1 : Ks; else spread = false;
  }
  if (K > (spread ? 256 : 32)) K = spread ? 256 : 32;
  if (spread && (int64_t)B * K > 2048) spread = false;       // (reduction partials: 64 x 32 workgroup rows)
  if (!spread && K > 32) K = 32;
  {
    // Co-residency: the device-scope barrier of the wide mode needs EVERY workgroup of the launch on the chip at the same time - a
    // workgroup that waits for a free CU never arrives and its peers spin until the watchdog.  The grid is therefore capped by what this
    // device keeps resident at the wide mode's workgroup size (occupancy of the kernel x compute units: a partitioned or smaller part,
    // a DOMPC_WIDE / DOMPC_WIDE_SPREAD override); K shrinks until it fits, down to one workgroup per problem.  (What this cannot see:
    // other kernels on the device - INTEGRATION.md section 4.)
    const int wb_ = fit_block(f.el_size, 256);
    const int64_t resident = (wb_ == 256 || f.slots64 <= 0) ? f.slots256 : (int64_t)f.slots64 * 64 / wb_;
    auto grid_of = [&](int k, bool sp) -> int64_t { return sp ? (int64_t)B * k : (int64_t)((B + 7) / 8) * 8 * k; };
    while (K > 1 && resident > 0 && grid_of(K, spread) > resident) --K;
  }
  if (K > 1 && B <= 64 && B <= f.n_slots) {
    s.wide = K;
    s.wide_spread = spread ? 1 : 0;
    s.grid = spread ? B * K : ((B + 7) / 8) * 8 * K;
  }
  // the workgroups of the wide mode (and of a sharded solve) have their own size
  int wide_block = (s.wide > 1 && s.wide_spread) ? auto_block : 256;
  if (o.wide_block) wide_block = o.wide_block;      // (512 needs a code object built with -DDOMPC_MAXBLOCK=512)
  if (s.wide > 1 || f.sharded) s.block = fit_block(f.el_size, wide_block);
  return s;
}

}  // namespace dompc_launch
