"""Tracking a set-point transition of the stirred tank reactor of examples/cstr_lqr.py with the time-varying LQR.

The reference has no counterpart: its `linearize` refuses models that vary along a trajectory ("LTV models are not yet implemented").
The transition is RECORDED, not designed: the nonlinear plant is simulated open loop from X0 (an empty, cold reactor) with an input
sequence that starts with a doubled feed and settles on USS (`Simulator.simulate_batch`), which takes it towards XSS.  B perturbed
starts are then tracked along that record by `closed_loop.BatchClosedLoopTVLQR`: the pairs (A_k, B_k) are the zero-order hold of the
Jacobians frozen at the knots of the record, the gains K_k come from one backward Riccati recursion over them (`LQR.gains_along`),
and the law is u_k = u*_k + K_k (x_k - x*_k).  Weights: Q, R of examples/cstr_lqr.py in standard mode, P_f = Q."""
import numpy as np

from ..closed_loop import BatchClosedLoopTVLQR
from . import cstr_lqr
from .cstr_lqr import Q, R, T_STEP, USS, X0, XSS, build_linear_model, build_model, build_simulator  # noqa: F401

N_STEPS = 20                         # steps of the recorded transition (10 min: 2.4 residence times at the final feed)
FEED_BOOST, FEED_DECAY = 1.0, 4.0    # F_k = F_ss (1 + FEED_BOOST exp(-k / FEED_DECAY)): the reactor is filled faster at first
# relative perturbation of the concentrations' scale and absolute one of the temperatures [K] of the B starts
START_SPREAD = np.array([0.1, 0.1, 2.0, 2.0])


def input_sequence(n_steps: int = N_STEPS) -> np.ndarray:
    """the inputs of the transition [n_steps][nu]"""
    k = np.arange(n_steps)
    U = np.tile(USS.ravel(), (n_steps, 1))
    U[:, 0] *= 1.0 + FEED_BOOST * np.exp(-k / FEED_DECAY)
    return U


def build_lqr(setup: bool = True, **setup_kw):
    """the controller in standard mode (the gains of the loop come from gains_along; setup() designs the constant gain at XSS)"""
    return cstr_lqr.build_lqr(build_linear_model(build_model()), setup=setup, n_horizon=None, rate=False, **setup_kw)


def record(simulator, n_steps: int = N_STEPS):
    """the recorded transition from X0: (X_ref [n_steps + 1][1][nx], U_ref [n_steps][1][nu])"""
    U = input_sequence(n_steps)
    r = simulator.simulate_batch(X0[None, :], U)
    assert not np.any(r["status"] & 1), "the open-loop simulation of the transition failed"
    return r["x"], U[:, None, :]


def starts(B: int, seed: int = 0) -> np.ndarray:
    """B starts around X0 [B][nx]: the first one is X0 itself"""
    rng = np.random.default_rng(seed)
    d = START_SPREAD[None, :] * rng.uniform(-1.0, 1.0, (B, 4))
    d[0] = 0.0
    d[:, :2] = np.abs(d[:, :2])      # (concentrations are not negative)
    return X0[None, :] + d


def build_loop(lqr, simulator, B: int = 9, device=0, n_steps: int = N_STEPS, seed: int = 0) -> BatchClosedLoopTVLQR:
    X_ref, U_ref = record(simulator, n_steps)
    return BatchClosedLoopTVLQR(lqr, simulator, starts(B, seed), X_ref, U_ref, device=device)
