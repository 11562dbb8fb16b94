// dompc_ampc.hip - one step of the approximate MPC (do_mpc.approximateMPC.ApproxMPC.make_step) for a batch: scale the input,
// evaluate the feed-forward network, rescale and clip - ONE launch.  The network's sizes and activations come from the generated
// header (lowering.py:lower_ampc); weights, biases, scaling and bounds are runtime data (retraining never rebuilds this object).
//
// One wavefront owns 32 samples; the sample sits on lane & 31.  A layer is H' <- act(W H' + b) on v_mfma_f32_32x32x2_f32
// (dompc_ampc_wave.h): the neurons of a 32-row tile are the 16 accumulator registers of the two lane halves, register g of half h
// = row 8 (g >> 2) + 4 h + (g & 3); the bias is the initial accumulator.  The accumulator tile of one layer IS the B operand of
// the next: step g of the next layer sums over the two rows that register g holds in the two lane halves (a sum has no order to
// keep), so no value moves between lanes and nothing goes through LDS.  The host packs W's columns in that order
// (do_mpc_amd/ampc.py:pack_weights): per layer [out tile][in tile][step g][lane] = W[32 to + (lane & 31)][32 tk + row(g, lane >> 5)],
// then the bias in natural order; rows and columns beyond the layer's sizes are zero, which keeps padded neurons inert whatever
// their activation is (sigmoid(0) = 0.5 meets a zero column).  Steps whose two rows are both padding are skipped at compile time.
//
// Arithmetic (the reference's promotions): xs = f32((f64(f32(x)) - shift) / range); the network in f32, per neuron an fmaf chain
// from the bias; y = f64(ys) * (ubu - lbu) + lbu; max(., lbu), min(., ubu) in f64.
//
// The Jacobian kernel (dompc_ampc_jac_kernel, the same code object): u as above, bit for bit, and du/dx, du/du_prev of the network
// for the same 32 samples per wavefront - forward mode, one input direction k after the other (the outermost loop, not unrolled).
// Per direction the primal and ONE tangent go through the layers together, a layer's primal pass first and its tangent pass behind it:
// the primal's input is dead when the tangent pass begins, so at most three sets of tiles are live (widest shape: 3 x 64 accumulator
// registers) where one pass over shared weight operands would hold four - and spill, as the compiler reported for 128 neurons.  The
// price is that a weight operand is read twice, from the cache.  The cost is about 2 n_in forward passes.
//
// Arithmetic of a tangent, f32 in the network's scaled coordinates: the first layer sees the unit vector e_k; a layer maps
// t_out[i] = d_i * chain, chain = the fmaf chain fmaf(W[i][j], t_in[j], acc) over j in the order of the primal pass from acc = 0 (no
// bias), d_i = the activation's derivative formed from its OUTPUT a_i as torch's backward forms it, the value at the kink included:
// relu a > 0 ? 1 : 0, tanh 1 - a a, leaky_relu a > 0 ? 1 : 0.01, sigmoid a (1 - a), linear 1 (products and differences rounded one
// by one).  A padded neuron's d_i may be non-zero (sigmoid: 0.25); its chain is zero and its column in the next layer is zero.
// J[i][k] = (f64(t_i) * (ubu - lbu)[i]) / range[k] in f64, product and quotient rounded separately (without scaling J = f64(t));
// with clip != 0 the row of an output with u < lbu or u > ubu before clipping is zero.  The f32 rounding of the input has no derivative.
//
// Build flavours as dompc_lqr.hip: hipcc --genco (product) or g++ -DDOMPC_HOST_EMU (tests).
#ifndef DOMPC_AMPC_HEADER
#error "DOMPC_AMPC_HEADER must name the generated network header"
#endif
#include DOMPC_AMPC_HEADER
#include "dompc_ampc_args.h"
#include "dompc_ampc_wave.h"

namespace dompc_ampck {

constexpr int NI = AMPC_N_IN, NO = AMPC_N_OUT, NH = AMPC_N_HIDDEN, NN = AMPC_N_NEURONS;
constexpr int TI = (NI + 31) / 32, TN = (NN + 31) / 32;
static_assert(NI >= 1 && NI <= 64 && NO >= 1 && NO <= 32 && NN >= 1 && NN <= 128 && NH >= 0 && NH <= 8, "network beyond the kernel's limits");
static_assert(NH > 0 || NN == NO, "without a hidden layer the one layer's neurons are the outputs");
// packed floats of a layer with TK input tiles and TO output tiles
constexpr int64_t layer_floats(int tk, int to) { return (int64_t)to * tk * 1024 + 32 * to; }
constexpr int64_t PACKED = NH == 0 ? layer_floats(TI, TN) : layer_floats(TI, TN) + (NH - 1) * layer_floats(TN, TN) + layer_floats(TN, 1);

// activation selectors of the generated header: 0 relu, 1 tanh, 2 leaky_relu (slope 0.01), 3 sigmoid, 4 linear
template <int ACT>
AMPC_DEV float activation(float x) {
  if (ACT == 0) return x > 0.0f ? x : 0.0f;
  if (ACT == 1) return ampc_tanh(x);
  if (ACT == 2) return x > 0.0f ? x : 0.01f * x;
  if (ACT == 3) return 1.0f / (1.0f + ampc_exp(-x));
  return x;
}

// out <- act(W in + b) for a layer of KIN inputs in TK tiles and TO output tiles
template <int TK, int TO, int KIN, int ACT>
AMPC_DEV void layer(const float* __restrict__ W, const Tile (&in)[TK], Tile (&out)[TO]) {
  const float* bias = W + (int64_t)TO * TK * 1024;
#pragma unroll
  for (int to = 0; to < TO; ++to) {
#pragma unroll
    for (int g = 0; g < 16; ++g) lanes([&](int l) { tset(out[to], g, l, bias[32 * to + AMPC_ROW(g, l >> 5)]); });
#pragma unroll
    for (int tk = 0; tk < TK; ++tk) {
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        if (32 * tk + AMPC_ROW(g, 0) < KIN) {          // (lane half 0 holds the lower of the step's two rows)
          wf a;
          lanes([&](int l) { wset(a, l, W[((to * TK + tk) * 16 + g) * 64 + l]); });
          mfma_32x32x2(a, tcol(in[tk], g), out[to]);
        }
      }
    }
#pragma unroll
    for (int g = 0; g < 16; ++g) lanes([&](int l) { tset(out[to], g, l, activation<ACT>(tget(out[to], g, l))); });
  }
}

// d act / d(pre-activation) from the activation's OUTPUT a (torch's backward formulas)
template <int ACT>
AMPC_DEV float activation_slope(float a) {
#pragma clang fp contract(off)
  if (ACT == 0) return a > 0.0f ? 1.0f : 0.0f;
  if (ACT == 1) return 1.0f - a * a;
  if (ACT == 2) return a > 0.0f ? 1.0f : 0.01f;
  if (ACT == 3) return a * (1.0f - a);
  return 1.0f;
}

// the tangent of layer(): tout <- diag(act'(out)) W tin, `out` being what layer() left (the activations)
template <int TK, int TO, int KIN, int ACT>
AMPC_DEV void layer_tangent(const float* __restrict__ W, const Tile (&tin)[TK], const Tile (&out)[TO], Tile (&tout)[TO]) {
#pragma unroll
  for (int to = 0; to < TO; ++to) {
#pragma unroll
    for (int g = 0; g < 16; ++g) lanes([&](int l) { tset(tout[to], g, l, 0.0f); });
#pragma unroll
    for (int tk = 0; tk < TK; ++tk) {
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        if (32 * tk + AMPC_ROW(g, 0) < KIN) {
          wf a;
          lanes([&](int l) { wset(a, l, W[((to * TK + tk) * 16 + g) * 64 + l]); });
          mfma_32x32x2(a, tcol(tin[tk], g), tout[to]);
        }
      }
    }
#pragma unroll
    for (int g = 0; g < 16; ++g) lanes([&](int l) { tset(tout[to], g, l, activation_slope<ACT>(tget(out[to], g, l)) * tget(tout[to], g, l)); });
  }
}

// the scaled network input of the 32 samples from `first` on
AMPC_DEV void scaled_input(const Args& A, int64_t first, Tile (&x)[TI]) {
  const double *shift = A.par, *range = A.par + NI;
#pragma unroll
  for (int t = 0; t < TI; ++t) {
#pragma unroll
    for (int g = 0; g < 16; ++g)
      lanes([&](int l) {
        const int f = 32 * t + AMPC_ROW(g, l >> 5);
        const int64_t s = first + (l & 31);
        float xs = 0.0f;
        if (f < NI && s < A.batch) {
          const int nup = NI - A.nx;
          const float x32 = (float)(f < A.nx ? A.x[s * A.nx + f] : A.u_prev[s * nup + (f - A.nx)]);
          xs = AMPC_SCALING ? (float)(((double)x32 - shift[f]) / range[f]) : x32;
        }
        tset(x[t], g, l, xs);
      });
  }
}

// output i of the network -> the input u_i, rescaled and (A.clip) clipped; *outside: u_i lay beyond a bound before clipping
AMPC_DEV double rescaled_output(const Args& A, int i, float ys, bool* outside) {
  const double *lbu = A.par + 2 * NI, *ubu = lbu + NO, *yrange = ubu + NO;
  double u = (double)ys;
  if (AMPC_SCALING) {
    // product and sum rounded separately, like the reference's two operations: no contraction into one fma here
#pragma clang fp contract(off)
    const double m = u * yrange[i];
    u = m + lbu[i];
  }
  *outside = u < lbu[i] || u > ubu[i];
  if (A.clip) {
    u = u > lbu[i] ? u : lbu[i];
    u = u < ubu[i] ? u : ubu[i];
  }
  return u;
}

// the 32 samples from `first` on
AMPC_DEV void step32(const Args& A, int64_t first) {
  Tile x[TI];
  scaled_input(A, first, x);
  Tile y[1];
  if constexpr (NH == 0) {
    layer<TI, 1, NI, AMPC_ACT>(A.w, x, y);
  } else {
    Tile h[TN], n[TN];
    layer<TI, TN, NI, AMPC_ACT>(A.w, x, h);
    const float* W = A.w + layer_floats(TI, TN);
#pragma unroll 1
    for (int k = 1; k < NH; ++k) {
      layer<TN, TN, NN, AMPC_ACT>(W, h, n);
#pragma unroll
      for (int t = 0; t < TN; ++t) h[t] = n[t];
      W += layer_floats(TN, TN);
    }
    layer<TN, 1, NN, AMPC_OUT_ACT>(W, h, y);
  }
#pragma unroll
  for (int g = 0; g < 16; ++g)
    lanes([&](int l) {
      const int i = AMPC_ROW(g, l >> 5);
      const int64_t s = first + (l & 31);
      if (i < NO && s < A.batch) {
        bool outside;
        A.u[s * NO + i] = rescaled_output(A, i, tget(y[0], g, l), &outside);
      }
    });
}

// u and the Jacobian of the 32 samples from `first` on
AMPC_DEV void jac32(const JacArgs& J, int64_t first) {
  Args A = J.step;
  const int nup = NI - A.nx;
  Tile x[TI];
  scaled_input(A, first, x);
#pragma unroll 1
  for (int k = 0; k < NI; ++k) {
    // weights, biases and bounds are the same in every direction: read again per direction they cost a cache hit, hoisted out of this
    // loop they would sit in more than a hundred registers through all of it
    A.w = reloaded(A.w);
    A.par = reloaded(A.par);
    const double *range = A.par + NI, *yrange = A.par + 2 * NI + 2 * NO;
    Tile e[TI];                                                // the unit vector e_k, for every sample
#pragma unroll
    for (int t = 0; t < TI; ++t) {
#pragma unroll
      for (int g = 0; g < 16; ++g) lanes([&](int l) { tset(e[t], g, l, 32 * t + AMPC_ROW(g, l >> 5) == k ? 1.0f : 0.0f); });
    }
    Tile y[1], ty[1];
    if constexpr (NH == 0) {
      layer<TI, 1, NI, AMPC_ACT>(A.w, x, y);
      layer_tangent<TI, 1, NI, AMPC_ACT>(A.w, e, y, ty);
    } else {
      Tile h[TN], th[TN], n[TN], tn[TN];
      layer<TI, TN, NI, AMPC_ACT>(A.w, x, h);
      layer_tangent<TI, TN, NI, AMPC_ACT>(A.w, e, h, th);
      const float* W = A.w + layer_floats(TI, TN);
#pragma unroll 1
      for (int q = 1; q < NH; ++q) {
        layer<TN, TN, NN, AMPC_ACT>(W, h, n);
        layer_tangent<TN, TN, NN, AMPC_ACT>(W, th, n, tn);
#pragma unroll
        for (int t = 0; t < TN; ++t) { h[t] = n[t]; th[t] = tn[t]; }
        W += layer_floats(TN, TN);
      }
      layer<TN, 1, NN, AMPC_OUT_ACT>(W, h, y);
      layer_tangent<TN, 1, NN, AMPC_OUT_ACT>(W, th, y, ty);
    }
#pragma unroll
    for (int g = 0; g < 16; ++g)
      lanes([&](int l) {
        const int i = AMPC_ROW(g, l >> 5);
        const int64_t s = first + (l & 31);
        if (i < NO && s < A.batch) {
          bool outside;
          const double u = rescaled_output(A, i, tget(y[0], g, l), &outside);
          if (k == 0) A.u[s * NO + i] = u;
          double d = (double)tget(ty[0], g, l);
          if (AMPC_SCALING) {
            // product and quotient rounded separately
#pragma clang fp contract(off)
            const double m = d * yrange[i];
            d = m / range[k];
          }
          if (A.clip && outside) d = 0.0;
          if (k < A.nx) J.du_dx[(s * NO + i) * A.nx + k] = d;
          else J.du_du_prev[(s * NO + i) * nup + (k - A.nx)] = d;
        }
      });
  }
}

}  // namespace dompc_ampck

#define AMPC_INFO(out, hash)                                                                                                  \
  do {                                                                                                                        \
    using namespace dompc_ampck;                                                                                              \
    out[0] = NI; out[1] = NO; out[2] = NH; out[3] = NN; out[4] = AMPC_ACT; out[5] = AMPC_OUT_ACT; out[6] = AMPC_SCALING;      \
    out[7] = (int64_t)sizeof(Args); out[8] = PACKED; out[9] = (int64_t)sizeof(JacArgs);                                   \
    const char h_[] = AMPC_MODEL_HASH;                                                                                        \
    for (int i = 0; i < (int)sizeof(h_); ++i) hash[i] = h_[i];                                                                \
  } while (0)

#ifdef DOMPC_AMPC_NO_ENTRY
// (included by dompc_ampc_loop.hip for step32: the entry points belong to the network's own code object)
#elif !defined(DOMPC_HOST_EMU)
extern "C" __global__ void __launch_bounds__(64) dompc_ampc_kernel(dompc_ampck::Args A) {
  dompc_ampck::step32(A, (int64_t)blockIdx.x * 32);
}
extern "C" __global__ void __launch_bounds__(64) dompc_ampc_jac_kernel(dompc_ampck::JacArgs J) {
  dompc_ampck::jac32(J, (int64_t)blockIdx.x * 32);
}
extern "C" __global__ void dompc_ampc_info_kernel(int64_t* out, char* hash) {
  if (threadIdx.x == 0 && blockIdx.x == 0) AMPC_INFO(out, hash);
}
#else
// The host twins take what the runtime passes to dompc_host::Context::run: the kernel's argument block behind a const void*.
extern "C" void dompc_ampc_hostemu_info(const void* args) { void* const* a = (void* const*)args; AMPC_INFO(((int64_t*)a[0]), ((char*)a[1])); }
extern "C" void dompc_ampc_hostemu_run(const void* args) {
  const dompc_ampck::Args* A = (const dompc_ampck::Args*)args;
  for (int64_t first = 0; first < A->batch; first += 32) dompc_ampck::step32(*A, first);
}
extern "C" void dompc_ampc_hostemu_jac(const void* args) {
  const dompc_ampck::JacArgs* J = (const dompc_ampck::JacArgs*)args;
  for (int64_t first = 0; first < J->step.batch; first += 32) dompc_ampck::jac32(*J, first);
}
#endif
