"""Three coupled tanks observed by an extended Kalman filter: the reference's examples/triple_tank_ekf
(/root/reference/examples/triple_tank_ekf/template_model.py, template_simulator.py, template_ekf.py, main.py).

Discrete-time model: the levels of three tanks in a row, two pumps, Torricelli flows between the tanks (sign / sqrt / fabs of the
level differences) and out of the middle one; only the level of the third tank is measured.  One parameter and one time-varying
parameter scale the outflow - the time-varying one steps from 0.5 to 1 at t = 50.  The expressions associate their operations
like the template, so the un-edited template lowers to the same text (tests/test_ekf_reference_templates.py)."""
import numpy as np

from ..ekf import EKF
from ..model import Model
from ..simulator import Simulator
from ..sym import fabs, sign, sqrt

X0_TRUE = np.array([2.0, 2.8, 2.7])
X0_EST = np.array([1.2, 1.4, 1.8])
U_CONST = np.array([1e-4, 1e-4])


def build_model() -> Model:
    model = Model("discrete")
    x1 = model.set_variable("_x", "x1")
    x2 = model.set_variable("_x", "x2")
    x3 = model.set_variable("_x", "x3")
    u1 = model.set_variable("_u", "u1")
    u2 = model.set_variable("_u", "u2")
    model.set_meas("x3_meas", x3)
    p1 = model.set_variable("_p", "p1")
    tvp1 = model.set_variable("_tvp", "tvp1")
    area, grav, dt = 0.00154, 9.81, 1
    r1, r2, r3 = 1, 0.8, 1
    pipe = 5 * 1e-5
    q13 = r1 * pipe * sign(x1 - x3) * sqrt(2 * grav * fabs(x1 - x3))
    q32 = r3 * pipe * sign(x3 - x2) * sqrt(2 * grav * fabs(x3 - x2))
    q20 = r2 * pipe * sqrt(2 * grav * x2) * tvp1 * p1
    model.set_rhs("x1", x1 + (dt / area) * (-q13 + u1))
    model.set_rhs("x2", x2 + (dt / area) * (q32 - q20 + u2))
    model.set_rhs("x3", x3 + (dt / area) * (q13 - q32))
    model.setup()
    return model


def _outflow_schedule(obj):
    p_num = obj.get_p_template()
    tvp_num = obj.get_tvp_template()

    def p_fun(t_now):
        p_num["p1"] = 2
        return p_num

    def tvp_fun(t_now):
        tvp_num["tvp1"] = 0.5 if t_now < 50 else 1
        return tvp_num
    obj.set_p_fun(p_fun)
    obj.set_tvp_fun(tvp_fun)


def build_simulator(model: Model, setup: bool = True, **setup_kw) -> Simulator:
    sim = Simulator(model)
    sim.set_param(t_step=1)
    _outflow_schedule(sim)
    if setup:
        sim.setup(**setup_kw)
    return sim


def build_ekf(model: Model, setup: bool = True, **setup_kw) -> EKF:
    ekf = EKF(model)
    ekf.settings.t_step = 1
    _outflow_schedule(ekf)
    if setup:
        ekf.setup(**setup_kw)
    return ekf
