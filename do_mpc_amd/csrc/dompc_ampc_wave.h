// dompc_ampc_wave.h - the wave-level layer under dompc_ampc.hip: one f32 value per lane of a 64-lane wavefront (`wf`), a 32 x 32 f32
// accumulator tile (`Tile`: 16 registers per lane) and the one matrix step the kernel is made of, v_mfma_f32_32x32x2_f32.
//
// Lane maps of the instruction (lane l, r = l & 31, h = l >> 5):  A[i = r][k = h],  B[k = h][j = r],
// C/D register g of lane l = element [i = 8 (g >> 2) + 4 h + (g & 3)][j = r].
//
// Two flavours, like dompc_lanes.h (which is the 16-lane float64 layer and knows nothing of this one): the product is the
// instruction; the host emulation (-DDOMPC_HOST_EMU, g++) keeps 64 lane slots per value and computes every element as the
// k-ordered std::fmaf chain the instruction is bit for bit: D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)).
#pragma once
#include <math.h>
#include <stdint.h>
#ifndef DOMPC_HOST_EMU
#include <hip/hip_runtime.h>
#else
#include <cmath>
#endif

namespace dompc_ampck {

// row of a tile that register g holds in lane half h
#define AMPC_ROW(g, h) (8 * ((g) >> 2) + 4 * (h) + ((g) & 3))

#ifndef DOMPC_HOST_EMU
#define AMPC_DEV __device__ __forceinline__
typedef float wf;
typedef float f32x16 __attribute__((ext_vector_type(16)));
struct Tile { f32x16 v; };

template <class F> AMPC_DEV void lanes(F f) { f((int)(threadIdx.x & 63)); }
AMPC_DEV float wget(const wf& w, int) { return w; }
AMPC_DEV void wset(wf& w, int, float x) { w = x; }
AMPC_DEV float tget(const Tile& t, int g, int) { return t.v[g]; }
AMPC_DEV void tset(Tile& t, int g, int, float x) { t.v[g] = x; }
AMPC_DEV wf tcol(const Tile& t, int g) { return t.v[g]; }
AMPC_DEV void mfma_32x32x2(const wf& a, const wf& b, Tile& c) { c.v = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c.v, 0, 0, 0); }
// p, as a value the compiler knows nothing about: loads through it are not hoisted out of the loop this is called in
template <class T> AMPC_DEV const T* reloaded(const T* p) { asm volatile("" : "+s"(p)); return p; }
AMPC_DEV float ampc_tanh(float x) { return tanhf(x); }
AMPC_DEV float ampc_exp(float x) { return expf(x); }
#else
#define AMPC_DEV inline
struct wf { float v[64]; };
struct Tile { float v[16][64]; };

template <class F> AMPC_DEV void lanes(F f) { for (int l = 0; l < 64; ++l) f(l); }
AMPC_DEV float wget(const wf& w, int l) { return w.v[l]; }
AMPC_DEV void wset(wf& w, int l, float x) { w.v[l] = x; }
AMPC_DEV float tget(const Tile& t, int g, int l) { return t.v[g][l]; }
AMPC_DEV void tset(Tile& t, int g, int l, float x) { t.v[g][l] = x; }
AMPC_DEV wf tcol(const Tile& t, int g) {
  wf w;
  for (int l = 0; l < 64; ++l) w.v[l] = t.v[g][l];
  return w;
}
AMPC_DEV void mfma_32x32x2(const wf& a, const wf& b, Tile& c) {
  for (int g = 0; g < 16; ++g)
    for (int l = 0; l < 64; ++l) {
      const int i = AMPC_ROW(g, l >> 5), j = l & 31;
      float acc = c.v[g][l];
      acc = std::fmaf(a.v[i], b.v[j], acc);                   // k = 0: A[i][0] sits in lane i, B[0][j] in lane j
      acc = std::fmaf(a.v[32 + i], b.v[32 + j], acc);         // k = 1: the upper lane half
      c.v[g][l] = acc;
    }
}
template <class T> AMPC_DEV const T* reloaded(const T* p) { return p; }
AMPC_DEV float ampc_tanh(float x) { return std::tanh(x); }
AMPC_DEV float ampc_exp(float x) { return std::exp(x); }
#endif

}  // namespace dompc_ampck
