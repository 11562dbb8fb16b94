// dompc_dopri.h - the explicit Dormand-Prince 5(4) pair (FSAL) and the step-size rules every adaptive integrator here shares: the plant
// (dompc_plant.hip: scalars, one sample per thread; its SDIRK 4(3) branch takes the two rules with its own exponent) and the filter
// (dompc_ekf.hip: [x; P] in lane values).  The stage loops stay with their state types; tableau and rules live here alone.
// The nodes c2 .. c5 are not listed: the right-hand sides are autonomous within a control interval (u, tvp, p are held).
#pragma once
#include <math.h>

#ifndef DOMPC_HOST_EMU
#define DOMPC_DOPRI_FN __device__ inline
#else
#define DOMPC_DOPRI_FN inline
#endif

namespace dompc_dopri {

constexpr double a21 = 1.0 / 5;
constexpr double a31 = 3.0 / 40, a32 = 9.0 / 40;
constexpr double a41 = 44.0 / 45, a42 = -56.0 / 15, a43 = 32.0 / 9;
constexpr double a51 = 19372.0 / 6561, a52 = -25360.0 / 2187, a53 = 64448.0 / 6561, a54 = -212.0 / 729;
constexpr double a61 = 9017.0 / 3168, a62 = -355.0 / 33, a63 = 46732.0 / 5247, a64 = 49.0 / 176, a65 = -5103.0 / 18656;
constexpr double b1 = 35.0 / 384, b3 = 500.0 / 1113, b4 = 125.0 / 192, b5 = -2187.0 / 6784, b6 = 11.0 / 84;
constexpr double e1 = 71.0 / 57600, e3 = -71.0 / 16695, e4 = 71.0 / 1920, e5 = -17253.0 / 339200, e6 = 22.0 / 525, e7 = -1.0 / 40;

// the local error is controlled at this fraction of the requested (abstol, reltol): the global error over a control interval then
// stays at the level CVODES delivers for the same settings (dompc_plant.hip)
constexpr double TOL_SAFETY = 0.01;

// initial step from the scaled norms d0 of the state and d1 of its derivative (Hairer, Norsett, Wanner II.4), at most t_step
DOMPC_DOPRI_FN double first_step(double d0, double d1, double t_step) {
  const double h = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
  return h > t_step ? t_step : h;
}
// factor of the next step from the scaled error of this one; exponent = -1 / (order of the embedded method + 1): -0.2 for the pair,
// -0.25 for SDIRK 4(3)
DOMPC_DOPRI_FN double step_factor(double err, double exponent) { return fmin(5.0, fmax(0.2, 0.9 * pow(fmax(err, 1e-10), exponent))); }

}  // namespace dompc_dopri
