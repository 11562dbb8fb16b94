"""The general plant rollout - Simulator.rollout_device, Simulator.simulate_batch, BatchClosedLoopLQR.run(fused=True) - on the MI355X
(dompc_plant_loop_kernel): the checks of tests/test_rollout.py on the HIP path."""
import pytest

import rollout_common as rc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,K", [(67, 4), (1, 1)])
def test_same_bits_as_the_law_rollout(B, K):
    rc.check_same_bits_as_law_rollout(False, B, K)


def test_open_loop_with_noise_equals_stepwise_launches():
    rc.check_open_loop_with_noise(False)


@pytest.mark.parametrize("which", ["family", "oscillating_masses_dae"])
def test_plants_with_algebraic_states(which):
    rc.check_dae_plant(which, False)


def test_previous_input_term():
    rc.check_previous_input_term(False)


@pytest.mark.parametrize("name", rc.LQR_CASES)
def test_lqr_loop_fused_equals_stepwise(name):
    rc.check_lqr_fused(name, False)


def test_lqr_loop_standard_mode_far_from_the_set_point():
    rc.check_lqr_law_far(False)


@pytest.mark.parametrize("name", ["one_term", "oscillating_masses"])
def test_lqr_loop_chunks_and_mixing_with_steps(name):
    rc.check_lqr_chunks_and_mixing(name, False)


@pytest.mark.parametrize("kind", ["ode", "dae"])
def test_simulate_batch_equals_make_step_batch(kind):
    rc.check_simulate_batch(kind, False)


def test_refusals():
    rc.check_refusals(False)
