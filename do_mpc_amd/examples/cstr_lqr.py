"""Continuous stirred tank reactor steered to an operating point by a linear quadratic regulator: the reference's
examples/lqr_examples/CSTR_lqr (/root/reference/examples/lqr_examples/CSTR_lqr/template_model.py, template_lqr.py,
template_simulator.py, main.py).

The nonlinear reactor (temperatures in Kelvin, no uncertain parameters - not the model of examples/cstr.py) is linearised at the
operating point (XSS, USS), discretised by zero-order hold over 0.5 min and regulated by a finite-horizon design (10 passes, P = Q)
in inputRatePenalization mode; the plant of the closed loop is the nonlinear model, 200 steps from X0.  The expressions keep the
template's association of operations, so the un-edited template lowers to the same text."""
import warnings

import numpy as np

from ..lqr import LQR
from ..model import LinearModel, Model, linearize
from ..simulator import Simulator
from ..sym import exp, vertcat

X0 = np.array([0.0, 0.0, 387.05, 387.05])
XSS = np.array([[1.6329], [1.1101], [398.6581], [397.3736]])      # C_a, C_b [kmol/m^3], T_R, T_J [K]
USS = np.array([[0.002365], [18.5583]])                           # F [m^3/min], Q_J [kJ/min]
N_STEPS = 200
T_STEP = 0.5
N_HORIZON = 10
Q = 10 * np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0.01, 0], [0, 0, 0, 0.01]])
R = np.array([[1e-1, 0], [0, 1e-5]])
R_DELTA = np.array([[1e8, 0], [0, 1]])


# plant data: two first-order reactions A -> B -> C with the same Arrhenius law, a cooling jacket
K0 = 2.145e10                       # frequency factor of both reactions [1/min]
E_OVER_R = 9758.3                   # activation temperature of both reactions [K]
DH_AB, DH_BC = -4200, -11000        # reaction enthalpies [kJ/kmol]
T_FEED = 387.05                     # [K]
CA_FEED = 5.1                       # [kmol/m^3]
VOLUME = 0.01                       # [m^3]
RHO_CP = 934.2 * 3.01               # density times heat capacity of the reactor content
JACKET_CAPACITY = 5 * 2             # mass times heat capacity of the jacket
K_A = 14.448                        # heat transfer to the jacket [kJ/(min K)]


def build_model(process_noise: bool = False) -> Model:
    """the nonlinear plant: mass balances of A and B, energy balances of reactor and jacket; process_noise: additive noise on every
    right-hand side (Monte-Carlo studies of the closed loop)"""
    mdl = Model("continuous")
    ca, cb, t_r, t_j = (mdl.set_variable("_x", name, (1, 1)) for name in ("C_a", "C_b", "T_R", "T_J"))
    feed = mdl.set_variable("_u", "F")
    cooling = mdl.set_variable("_u", "Q_J")
    arrhenius = lambda c: K0 * exp(-E_OVER_R / t_r) * c      # noqa: E731
    rate_ab, rate_bc = arrhenius(ca), arrhenius(cb)
    mdl.set_expression("r", vertcat(rate_ab, rate_bc))
    dilution = lambda: feed / VOLUME      # noqa: E731  (one node per use, like the template: the lowered text is compared)
    to_jacket = lambda: t_r - t_j      # noqa: E731
    reaction_heat = DH_AB * (-rate_ab) + DH_BC * (-rate_bc)
    mdl.set_rhs("C_a", dilution() * (CA_FEED - ca) - rate_ab, process_noise=process_noise)
    mdl.set_rhs("C_b", -dilution() * cb + rate_ab - rate_bc, process_noise=process_noise)
    mdl.set_rhs("T_R", dilution() * (T_FEED - t_r) - (K_A / (RHO_CP * VOLUME)) * to_jacket() + (1 / RHO_CP) * reaction_heat, process_noise=process_noise)
    mdl.set_rhs("T_J", (1 / JACKET_CAPACITY) * (-cooling + K_A * to_jacket()), process_noise=process_noise)
    mdl.setup()
    return mdl


def build_linear_model(model: Model) -> LinearModel:
    """the plant linearised at the operating point (continuous)"""
    return linearize(model, XSS, USS)


def build_lqr(linear_model: LinearModel, setup: bool = True, n_horizon=N_HORIZON, rate: bool = True, **setup_kw) -> LQR:
    lqr = LQR(linear_model.discretize(T_STEP))
    lqr.set_param(n_horizon=n_horizon, t_step=T_STEP)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)      # (P defaults to Q on the finite horizon, as in the template)
        lqr.set_objective(Q=Q, R=R)
    if rate:
        lqr.set_rterm(delR=R_DELTA)
    if setup:
        lqr.setup(**setup_kw)
    return lqr


def build_simulator(model: Model, setup: bool = True, **setup_kw) -> Simulator:
    sim = Simulator(model)
    sim.set_param(integration_tool="cvodes", abstol=1e-10, reltol=1e-10, t_step=T_STEP)
    if setup:
        sim.setup(**setup_kw)
    return sim
