"""Continuous stirred tank reactor steered by an approximate MPC: the reference's examples/CSTR_approximate_mpc
(/root/reference/examples/CSTR_approximate_mpc/main.py, template_mpc.py, template_simulator.py).

A nominal controller (n_robust = 0) is sampled on the box of its bounds, a network with ONE hidden layer of 50 neurons is trained on
the samples and then replaces the solve in the loop.  The controller is the class ("CSTR", {"n_robust": 0, "collocation_deg": 3})
of examples/cstr.py, whose batch code object is prebuilt; the box is the one of the reference's template_mpc.py, which bounds T_R
from above by a hard bound at 140 where examples/cstr.py has a soft constraint: the network's box takes that bound."""
import numpy as np

from ..sampling import AMPCSampler
from ..simulator import Simulator
from . import cstr

X0 = cstr.X0
U0 = np.array([5.0, 0.0])                # main.py:69
T_STEP = 0.005
N_STEPS = 100
N_HIDDEN_LAYERS, N_NEURONS = 1, 50
T_R_UPPER = 140.0                        # template_mpc.py: mpc.bounds["upper", "_x", "T_R"]
MPC_CLASS = {"n_robust": 0, "collocation_deg": 3}
# the reference's box (template_mpc.py): C_a, C_b, T_R, T_K and F, Q_dot
BOX = dict(lbx=[0.1, 0.1, 50.0, 50.0], ubx=[2.0, 2.0, T_R_UPPER, 140.0], lbu=[5.0, -8500.0], ubu=[100.0, 0.0])


def build_model():
    return cstr.build_model()


def build_mpc(model, **overrides):
    mpc = cstr.build_mpc(model, **{**MPC_CLASS, **overrides})
    mpc.x0 = X0
    mpc.u0 = U0
    mpc.set_initial_guess()
    return mpc


def build_simulator(model, setup: bool = True, **setup_kw) -> Simulator:
    """template_simulator.py; the plant's parameters are the nominal ones"""
    sim = Simulator(model)
    sim.set_param(integration_tool="cvodes", abstol=1e-10, reltol=1e-10, t_step=T_STEP)
    p_num = sim.get_p_template()
    p_num["alpha"], p_num["beta"] = 1.0, 1.0
    sim.set_p_fun(lambda t_now: p_num)
    if setup:
        sim.setup(**setup_kw)
        sim.x0 = X0
    return sim


def box(settings) -> None:
    """the reference's bounds box on the settings of an ApproxMPC or an AMPCSampler"""
    settings.ubx = np.array(settings.ubx, dtype=float).reshape(-1, 1)
    settings.ubx[2, 0] = T_R_UPPER


def build_ampc(mpc, setup: bool = True, n_hidden_layers=N_HIDDEN_LAYERS, n_neurons=N_NEURONS, **setup_kw):
    from ..ampc import ApproxMPC      # (torch is imported only when a network is built)
    ampc = ApproxMPC(mpc)
    ampc.settings.n_hidden_layers = n_hidden_layers
    ampc.settings.n_neurons = n_neurons
    box(ampc.settings)
    if setup:
        ampc.setup(**setup_kw)
    return ampc


def build_sampler(mpc, dataset_name: str, n_samples: int, data_dir: str, simulator=None, closed_loop: bool = False,
                  sensitivities: bool = False) -> AMPCSampler:
    """sensitivities=True: the data file also carries du0dx0 and du0du_prev of every row (the labels of Sobolev training)"""
    sampler = AMPCSampler(mpc, simulator)
    st = sampler.settings
    st.dataset_name, st.n_samples, st.data_dir = dataset_name, n_samples, data_dir
    st.closed_loop_flag, st.trajectory_length = closed_loop, 1
    st.store_sensitivities = sensitivities
    box(st)
    sampler.setup()
    return sampler


def build_trainer(ampc, dataset_name: str, n_epochs: int, data_dir: str, results_dir: str, sobolev_weight: float = 0.0):
    """sobolev_weight > 0: the loss also fits the network's Jacobian to the stored sensitivities (build_sampler(sensitivities=True))"""
    from ..ampc import Trainer
    trainer = Trainer(ampc)
    st = trainer.settings
    st.dataset_name, st.n_epochs, st.data_dir, st.results_dir = dataset_name, n_epochs, data_dir, results_dir
    st.sobolev_weight = sobolev_weight
    st.save_history = True
    st.scheduler_flag = True
    trainer.scheduler_settings.cooldown = 0
    trainer.scheduler_settings.patience = 50
    trainer.setup()
    return trainer
