"""Time-varying LQR along trajectories, the law record per step of the general plant rollout and BatchClosedLoopTVLQR on the MI355X
(HIP path through the C ABI): the checks of tests/test_lqr_tv.py on the device, with the bounds established there on the host
emulation.  Reads only the prebuilt code objects."""
import pytest

import lqr_tv_common as tc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K", [1, 3, 10])
@pytest.mark.parametrize("nx,nu,rate", tc.CONSTANT_DESIGNS, ids=lambda v: str(v))
def test_constant_pair_equals_the_finite_horizon_design(nx, nu, rate, K):
    tc.check_constant_pair(nx, nu, rate, K, hostemu=False)


@pytest.mark.parametrize("rate,K,shared", tc.RANDOM_CASES, ids=lambda v: str(v))
def test_random_pairs_against_the_twin(rate, K, shared):
    tc.check_random_pairs(rate, K, shared, hostemu=False)


@pytest.mark.parametrize("name", tc.ALONG_CASES)
def test_gains_along_against_the_twins(name):
    tc.check_gains_along(name, hostemu=False)


def test_gains_along_item_decomposition():
    tc.check_item_decomposition(hostemu=False)


def test_status_and_neighbours():
    tc.check_status_and_neighbours(hostemu=False)


def test_failed_knot_beside_good_trajectories():
    tc.check_failed_knot(hostemu=False)


def test_device_pointer_entries_equal_the_host_entries():
    tc.check_device_entries(hostemu=False)


def test_refusals_of_the_time_varying_entries():
    tc.check_lqr_refusals(hostemu=False)


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("kind", ["ode", "dae", "discrete"])
def test_rollout_with_a_law_record_per_step(kind, K):
    tc.check_rollout_law_step(kind, K, hostemu=False)


def test_refusals_of_law_step():
    tc.check_rollout_refusals(hostemu=False)


@pytest.mark.parametrize("noise", [False, True], ids=["quiet", "noise"])
def test_loop_fused_equals_stepwise(noise):
    tc.check_loop_paths(hostemu=False, noise=noise)


def test_tracking_beats_replaying_the_inputs():
    tc.check_tracking_beats_replay(hostemu=False)
