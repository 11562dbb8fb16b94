"""Batch reactor with an algebraic state regulated by a linear quadratic regulator: the reference's
examples/lqr_examples/batch_reactor_lqr_dae (/root/reference/examples/lqr_examples/batch_reactor_lqr_dae/template_model.py,
template_lqr.py, template_simulator.py, main.py).

Three concentrations Ca, Cb, Ad as states, the feed Cain as input and Cc as algebraic state of the linear balance
0 = 1 + Ad - Ca - Cb - Cc.  The reference's route: the index-1 DAE model becomes an ODE model with the states [Ca, Cb, Ad, Cain, Cc]
and the input rate q (dae2odeconversion), which is linear, is linearised without an operating point, discretised by zero-order hold
over 0.5 s and regulated by a finite-horizon design (10 passes, P = Q); the plant of the closed loop is the continuous linear model,
50 steps from X0 to the set-point XSS.  The expressions keep the template's association of operations, so the un-edited template
lowers to the same text.  `build_dae_model()` alone is the plant for the batched route, LQR.gains_at on the model with its algebraic
state (three states, one input)."""
import warnings

import numpy as np

from ..lqr import LQR
from ..model import LinearModel, Model, dae2odeconversion, linearize
from ..simulator import Simulator

X0 = np.array([1.0, 0.0, 0.0, 0.0, 0.0])                   # Ca, Cb, Ad, Cain, Cc
XSS = np.array([[0.0], [2.0], [3.0], [0.0], [2.0]])
N_STEPS = 50
t_step = T_STEP = 0.5
N_HORIZON = 10
Q = 10 * np.identity(5)
R = 5 * np.identity(1)

K1, K2, K3 = 25, 1, 1               # rate constants [1/s]


def build_dae_model(symvar_type="SX") -> Model:
    """the index-1 DAE plant: x = (Ca, Cb, Ad), u = Cain, z = Cc"""
    mdl = Model("continuous", symvar_type)
    ca = mdl.set_variable("_x", "Ca")
    cb = mdl.set_variable("_x", "Cb")
    ad = mdl.set_variable("_x", "Ad")
    cain = mdl.set_variable("_u", "Cain")
    cc = mdl.set_variable("_z", "Cc")
    mdl.set_rhs("Ca", -K1 * ca + cain)
    mdl.set_rhs("Cb", K1 * ca - K2 * cb + K3 * cc)
    mdl.set_rhs("Ad", cain)
    mdl.set_alg("exp", 1 + ad - ca - cb - cc)
    mdl.setup()
    return mdl


def build_model(symvar_type="SX") -> LinearModel:
    """the continuous linear model of the converted ODE system (five states, the input rate q)"""
    return linearize(dae2odeconversion(build_dae_model(symvar_type)))


def build_lqr(linear_model: LinearModel, setup: bool = True, n_horizon=N_HORIZON, rate: bool = False, **setup_kw) -> LQR:
    assert not rate, "the example runs in standard mode"
    lqr = LQR(linear_model.discretize(T_STEP))
    lqr.set_param(n_horizon=n_horizon, t_step=T_STEP)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)      # (P defaults to Q on the finite horizon, as in the template)
        lqr.set_objective(Q=Q, R=R)
    if setup:
        lqr.setup(**setup_kw)
    return lqr


def build_simulator(model: LinearModel, setup: bool = True, **setup_kw) -> Simulator:
    sim = Simulator(model)
    sim.set_param(integration_tool="cvodes", t_step=T_STEP)
    if setup:
        sim.setup(**setup_kw)
    return sim
