"""Two oscillating masses under a linear quadratic regulator: the reference's examples/lqr_examples/oscillating_masses_discrete_lqr
(/root/reference/examples/lqr_examples/oscillating_masses_discrete_lqr/template_model.py, template_lqr.py, template_simulator.py,
main.py).

A discrete LinearModel given by its matrices (four states in one vector variable, one input), an infinite-horizon design in
inputRatePenalization mode with unit weights, 50 closed-loop steps from X0 with the linear model itself as the plant."""
import numpy as np

from ..lqr import LQR
from ..model import LinearModel
from ..simulator import Simulator

X0 = np.array([2.0, 1.0, 3.0, 1.0])
N_STEPS = 50
T_STEP = 0.5
A = np.array([[0.763, 0.460, 0.115, 0.020],
              [-0.899, 0.763, 0.420, 0.115],
              [0.115, 0.020, 0.763, 0.460],
              [0.420, 0.115, -0.899, 0.763]])
B = np.array([[0.014], [0.063], [0.221], [0.367]])


def build_model() -> LinearModel:
    model = LinearModel("discrete")
    model.set_variable("_x", "x", (4, 1))
    model.set_variable("_u", "u", (1, 1))
    model.setup(A, B)
    return model


def build_lqr(model: LinearModel, setup: bool = True, n_horizon=None, rate: bool = True, **setup_kw) -> LQR:
    lqr = LQR(model)
    lqr.settings.t_step = T_STEP
    lqr.settings.n_horizon = n_horizon
    lqr.set_objective(Q=np.identity(4), R=np.identity(1))
    if rate:
        lqr.set_rterm(delR=np.identity(1))
    if setup:
        lqr.setup(**setup_kw)
    return lqr


def build_simulator(model: LinearModel, setup: bool = True, **setup_kw) -> Simulator:
    sim = Simulator(model)
    sim.set_param(t_step=T_STEP)
    if setup:
        sim.setup(**setup_kw)
    return sim
