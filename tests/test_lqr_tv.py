"""Time-varying LQR along trajectories, the law record per step of the general plant rollout and BatchClosedLoopTVLQR on the host
emulation of the kernels (the text that ships, compiled by g++): no GPU needed.  The checks are those of tests/test_gpu_lqr_tv.py
(lqr_tv_common.py); the bounds of the comparisons with the numpy twin are established here."""
import numpy as np
import pytest

import lqr_tv_common as tc


@pytest.mark.parametrize("K", [1, 3, 10])
@pytest.mark.parametrize("nx,nu,rate", tc.CONSTANT_DESIGNS, ids=lambda v: str(v))
def test_constant_pair_equals_the_finite_horizon_design(nx, nu, rate, K):
    tc.check_constant_pair(nx, nu, rate, K, hostemu=True)


@pytest.mark.parametrize("rate,K,shared", tc.RANDOM_CASES, ids=lambda v: str(v))
def test_random_pairs_against_the_twin(rate, K, shared):
    """the spread written in lqr_tv_common.SPREAD is the one measured now (x86-64 longdouble), and the host emulation is within the
    bound that follows from it"""
    sp, worst = tc.check_random_pairs(rate, K, shared, hostemu=True, measure=True)
    key = ("rate" if rate else "standard", K, "shared" if shared else "per")
    print(f"{key}: twin spread {sp:.3e} (written {tc.SPREAD[key]:.3e}), host emulation - twin = {worst:.3e}")
    assert abs(sp / tc.SPREAD[key] - 1.0) < 0.01
    tc.check_random_pairs(rate, K, shared, hostemu=True)


@pytest.mark.parametrize("name", tc.ALONG_CASES)
def test_gains_along_against_the_twins(name):
    tc.check_gains_along(name, hostemu=True)


def test_gains_along_item_decomposition():
    tc.check_item_decomposition(hostemu=True)


def test_status_and_neighbours():
    tc.check_status_and_neighbours(hostemu=True)


def test_failed_knot_beside_good_trajectories():
    tc.check_failed_knot(hostemu=True)


def test_device_pointer_entries_equal_the_host_entries():
    tc.check_device_entries(hostemu=True)


def test_refusals_of_the_time_varying_entries():
    tc.check_lqr_refusals(hostemu=True)


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("kind", ["ode", "dae", "discrete"])
def test_rollout_with_a_law_record_per_step(kind, K):
    tc.check_rollout_law_step(kind, K, hostemu=True)


def test_refusals_of_law_step():
    tc.check_rollout_refusals(hostemu=True)


@pytest.mark.parametrize("noise", [False, True], ids=["quiet", "noise"])
def test_loop_fused_equals_stepwise(noise):
    tc.check_loop_paths(hostemu=True, noise=noise)


def test_tracking_beats_replaying_the_inputs():
    """observed on the host emulation (B = 9, 20 steps): see lqr_tv_common.check_tracking_beats_replay"""
    tc.check_tracking_beats_replay(hostemu=True)


def test_a_rate_mode_controller_is_refused():
    import lqr_common as lc
    from do_mpc_amd.closed_loop import BatchClosedLoopTVLQR
    lqr = lc.model_free_lqr(3, 1, True, rate=True)
    with pytest.raises(NotImplementedError, match="inputRatePenalization"):
        BatchClosedLoopTVLQR(lqr, None, np.zeros((1, 3)), np.zeros((2, 1, 3)), np.zeros((1, 1, 1)))
