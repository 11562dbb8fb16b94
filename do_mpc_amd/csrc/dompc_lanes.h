// dompc_lanes.h - the lane-row layer: what a kernel written as "one problem per row of 16 lanes, four per wavefront" stands on
// (the edge sweep of dompc_quad.h, the filter of dompc_ekf.hip, the design of dompc_lqr.hip).  It reads no
// model macro.  Like the kernels it is built twice: by hipcc for the device and by g++ -DDOMPC_HOST_EMU for the tests.
//
// The lane value `lv`.  Kernel text is written once, on a type that is a double on the device (the value THIS lane holds) and the 16
// values of a row of lanes on the host, with element-wise operators.  A value "of the group" (the same in its 16 lanes) is a double
// in both flavours.  bc<L>(v) is lane L's value of v (v_mov_b64_dpp row_newbcast:L there, element L here), fmac_bc<L>(d, src, mul)
// is d += bc<L>(src) * mul (one v_fmac_f64_dpp there, an fma per element here), lane_bcast / lane_gather are the same with a lane
// that is known at run time only (ds_bpermute).
//
// Two rules keep the device flavour correct.  The layer cannot check them; its callers keep them:
//  1. UNIFORM CONTROL FLOW AROUND CROSS-LANE READS.  A DPP or ds_bpermute read takes its value from a lane that has to be executing
//     the instruction: bc, fmac_bc, lane_bcast, lane_gather (and gsum / gmax built on them) are never placed inside a branch, a
//     loop or a select arm that some lane of the wavefront does not take.  Loops run until the slowest group of the wavefront is
//     through (wave_any); a group that has finished keeps its values by sel.  Idle groups of the last wavefront repeat the last
//     entry of the batch and store nothing (group_entry).  once_per_group is the one sanctioned branch: no cross-lane read inside.
//  2. dpp_ready BEFORE fmac_bc.  On gfx9 a vector instruction that reads a register through DPP needs two wait states after the
//     vector instruction that wrote it.  For its own instructions the compiler inserts them; for bc (an intrinsic) it does so too,
//     and it never folds that move into the multiply-add that follows.  fmac_bc is therefore inline assembly, which the compiler's
//     hazard recogniser does not look into: the CALLER guarantees that `src` was not written by one of the two preceding vector
//     instructions.  dpp_ready(a) is that guarantee for a block of fmac_bc reads of a[]: it pins every a[i] (the value exists in
//     its register at this point, nothing is sunk behind it) and spends the two wait states (s_nop 1).  Within the block a
//     destination may be a later source only if two instructions lie in between (dompc_quad.h orders its updates that way).
//     -DDOMPC_LANES_FMAC_DPP=0 is the A/B switch: bc and fma as two instructions, every hazard the compiler's, dpp_ready empty.
#pragma once
#include <math.h>
#include <type_traits>
#include <utility>

#ifndef DOMPC_LANES_FMAC_DPP
#define DOMPC_LANES_FMAC_DPP 1
#endif

namespace dompc_lanes {

#ifndef DOMPC_HOST_EMU
// ---------------------------------------------------------------- device: a lane value is a double
#define DOMPC_LANES_FN __device__ inline
using lv = double;
struct Group { int j; double* lds; };            // lane inside its row of 16, LDS slice of the group
extern "C" __device__ double dompc_lanes_dpp_f64(double old, double src, int ctrl, int row_mask, int bank_mask, bool bound_ctrl) __asm("llvm.amdgcn.update.dpp.f64");
// value of `v` in lane L of this lane's row of 16 lanes (v_mov_b64_dpp row_newbcast:L)
template <int L>
__device__ inline double rbc(double v) {
  static_assert(L >= 0 && L < 16, "lane inside a row of 16");
  return dompc_lanes_dpp_f64(0.0, v, 0x150 + L, 0xf, 0xf, true);
}
// the value is computed HERE (an empty asm the optimiser cannot look through): without it the IR-level sinking pass moves whole chains of
// arithmetic next to their first use, hundreds of instructions later, and keeps their operands alive (in scratch) in between
__device__ inline void pin(double& v) { asm volatile("" : "+v"(v)); }
__device__ inline void pin(int& v) { asm volatile("" : "+v"(v)); }
// d += (value of `src` in lane L of the row of 16) * mul in ONE instruction (rule 2 above)
template <int L>
__device__ inline void fmac_rbc(double& d, const double& src, double mul) {
#if DOMPC_LANES_FMAC_DPP
  asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(d) : "v"(src), "v"(mul), "n"(L));
#else
  d = fma(rbc<L>(src), mul, d);
#endif
}
template <int N>
__device__ inline void dpp_ready(double (&a)[N]) {
#if DOMPC_LANES_FMAC_DPP
#pragma unroll
  for (int i = 0; i < N; ++i) pin(a[i]);
  asm volatile("s_nop 1");
#endif
}
template <int L> __device__ inline double bc(lv v) { return rbc<L>(v); }
template <int L> __device__ inline void fmac_bc(lv& d, const lv& src, lv mul) { fmac_rbc<L>(d, src, mul); }
__device__ inline lv splat(double v) { return v; }
__device__ inline lv lfabs(lv a) { return fabs(a); }
__device__ inline lv lfmax(lv a, lv b) { return fmax(a, b); }
__device__ inline lv lfma(lv a, lv b, lv c) { return fma(a, b, c); }
__device__ inline lv sel(bool c, lv a, lv b) { return c ? a : b; }                     // c: the same in every lane of the group
__device__ inline lv lsel(lv mask, lv a, lv b) { return mask != 0.0 ? a : b; }         // per lane: mask is 1 or 0
template <class G> __device__ inline lv unit(const G& g, int k) { return g.j == k ? 1.0 : 0.0; }        // 1 in lane k
template <class G> __device__ inline lv lane_lt(const G& g, int n) { return g.j < n ? 1.0 : 0.0; }      // 1 in the lanes below n
// value of `v` in lane `src` of the row of 16, `src` known at run time only (ds_bpermute; executed by every lane)
__device__ inline double lane_bcast(lv v, int src) { return __shfl(v, src, 16); }
__device__ inline lv lane_gather(lv v, lv src) { return __shfl(v, (int)src, 16); }
__device__ inline void group_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
template <class G, class F> __device__ inline void once_per_group(const G& g, F&& f) { if (g.j == 0) f(); }
__device__ inline bool wave_any(bool c) { return __ballot(c) != 0ull; }
// Kernel entry (one wavefront per workgroup, four groups per wavefront): entry b of the batch and the LDS slice of this lane's group,
// GSZ doubles of `lds`, zeroed.  Groups beyond the batch repeat its last entry with act = false.
struct Entry { int b; bool act; Group G; };
template <int GSZ>
__device__ inline Entry group_entry(double* lds, int batch) {
  const int lane = (int)(threadIdx.x & 63u), g = lane >> 4, j = lane & 15;
  const int f = (int)blockIdx.x * 4 + g;
  const bool act = f < batch;
  const int b = act ? f : batch - 1;
  double* L = lds + g * GSZ;
  for (int i = j; i < GSZ; i += 16) L[i] = 0.0;
  group_sync();
  return Entry{b, act, Group{j, L}};
}
#else
// ---------------------------------------------------------------- host: the 16 values of a row of lanes
#define DOMPC_LANES_FN inline
struct lv { double e[16]; };
struct Group { double* lds; };
#define DOMPC_LV_BIN(op)                                                                                                      \
  inline lv operator op(const lv& a, const lv& b) { lv r; for (int l = 0; l < 16; ++l) r.e[l] = a.e[l] op b.e[l]; return r; } \
  inline lv operator op(const lv& a, double b) { lv r; for (int l = 0; l < 16; ++l) r.e[l] = a.e[l] op b; return r; }         \
  inline lv operator op(double a, const lv& b) { lv r; for (int l = 0; l < 16; ++l) r.e[l] = a op b.e[l]; return r; }
DOMPC_LV_BIN(+) DOMPC_LV_BIN(-) DOMPC_LV_BIN(*) DOMPC_LV_BIN(/)
#undef DOMPC_LV_BIN
inline lv splat(double v) { lv r; for (int l = 0; l < 16; ++l) r.e[l] = v; return r; }
inline lv lfabs(const lv& a) { lv r; for (int l = 0; l < 16; ++l) r.e[l] = fabs(a.e[l]); return r; }
inline lv lfmax(const lv& a, const lv& b) { lv r; for (int l = 0; l < 16; ++l) r.e[l] = fmax(a.e[l], b.e[l]); return r; }
inline lv lfma(const lv& a, const lv& b, const lv& c) { lv r; for (int l = 0; l < 16; ++l) r.e[l] = fma(a.e[l], b.e[l], c.e[l]); return r; }
inline lv lfma(const lv& a, double b, const lv& c) { lv r; for (int l = 0; l < 16; ++l) r.e[l] = fma(a.e[l], b, c.e[l]); return r; }
inline lv sel(bool c, const lv& a, const lv& b) { return c ? a : b; }
inline lv lsel(const lv& mask, const lv& a, const lv& b) { lv r; for (int l = 0; l < 16; ++l) r.e[l] = mask.e[l] != 0.0 ? a.e[l] : b.e[l]; return r; }
template <class G> inline lv unit(const G&, int k) { lv r; for (int l = 0; l < 16; ++l) r.e[l] = l == k ? 1.0 : 0.0; return r; }
template <class G> inline lv lane_lt(const G&, int n) { lv r; for (int l = 0; l < 16; ++l) r.e[l] = l < n ? 1.0 : 0.0; return r; }
inline double lane_bcast(const lv& v, int src) { return v.e[src & 15]; }
inline lv lane_gather(const lv& v, const lv& src) { lv r; for (int l = 0; l < 16; ++l) r.e[l] = v.e[(int)src.e[l] & 15]; return r; }
template <int L> inline double bc(const lv& v) { return v.e[L]; }
template <int L> inline void fmac_bc(lv& d, const lv& src, const lv& mul) { for (int l = 0; l < 16; ++l) d.e[l] = fma(src.e[L], mul.e[l], d.e[l]); }
template <int N> inline void dpp_ready(lv (&)[N]) {}
inline void group_sync() {}
template <class G, class F> inline void once_per_group(const G&, F&& f) { f(); }
inline bool wave_any(bool c) { return c; }
// the run loop of the emulation: f(b, group) for every entry of the batch, one group at a time on a zeroed slice of GSZ doubles
template <int GSZ, class F>
inline void for_each_entry(int batch, F&& f) {
  for (int b = 0; b < batch; ++b) {
    double L[GSZ];
    for (int i = 0; i < GSZ; ++i) L[i] = 0.0;
    f(b, Group{L});
  }
}
#endif

// ---------------------------------------------------------------- both
template <class F, int... I>
DOMPC_LANES_FN void sfor_(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
// f(integral_constant<int, i>) for i = 0 .. N-1: loops whose index has to be a constant expression
template <int N, class F>
DOMPC_LANES_FN void sfor(F&& f) { sfor_(f, std::make_integer_sequence<int, (N > 0 ? N : 0)>{}); }

}  // namespace dompc_lanes
