"""Sensitivity-based MPC (do_mpc_amd/asmpc.py, csrc/dompc_asmpc.hip, the plant rollout of csrc/dompc_plant.hip) on the TEST-ONLY host
emulation of the kernels (the -m gpu twin: test_gpu_asmpc.py)."""
import pytest

import asmpc_common as ac
import hostemu
from test_hostemu_parity import make_mpc


@pytest.mark.parametrize("B", ac.BATCHES)
@pytest.mark.parametrize("shape", ac.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_law_and_step_match_the_reference_formula(shape, B):
    ac.check_shape(*shape, B, hostemu=True)


def test_zero_leading_entry_is_solved_by_pivoting():
    ac.check_pivoting(hostemu=True)


@pytest.mark.parametrize("shape", [(3, 16), (17, 3), (64, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_law_preparation_with_pivot_orders_that_are_not_the_identity(shape):
    """I - G = a signed permutation + noise, another permutation in every member of the wavefront.  Measured on the host emulation,
    relative to the largest entry: 8.3e-16 (3 x 16), 3.3e-16 (17 x 3), 8.5e-16 (64 x 16) at the bound 1e-12 of `close`; cond(I - G) <= 2"""
    ac.check_pivot_orders(*shape, hostemu=True)


def test_singular_failed_and_nan_members_fall_back_and_stay_local():
    ac.check_fallbacks(hostemu=True)


def test_clip_infinite_bounds_nan_state_and_max_dx():
    ac.check_clip_nan_and_max_dx(hostemu=True)


def test_refusals_by_name():
    ac.check_refusals(make_mpc, hostemu.patched)


@pytest.mark.parametrize("name", ["batch_reactor", "CSTR"])
def test_solve_and_step_equal_the_example_class(name):
    ac.check_solve_equals_example(make_mpc, name, hostemu=True)


@pytest.mark.parametrize("name", ["batch_reactor", "CSTR"])
def test_make_step_equals_row_0_of_the_batched_loop(name):
    ac.check_make_step_equals_row0(make_mpc, name, hostemu=True)


@pytest.mark.parametrize("name", ["batch_reactor", "CSTR"])
def test_fused_run_equals_stepwise_run(name):
    ac.check_fused_equals_stepwise(make_mpc, name, hostemu=True)


def test_fused_run_equals_stepwise_run_with_plant_parameters_that_change_with_time():
    ac.check_fused_equals_stepwise(make_mpc, "CSTR", hostemu=True, varying=True)


def test_rollout_with_a_law_from_set_law_equals_the_stepwise_launches():
    ac.check_rollout_with_synthetic_law(hostemu=True)


def test_rollout_refuses_a_plant_with_algebraic_states():
    ac.check_dae_plant_is_refused(make_mpc, hostemu=True)
