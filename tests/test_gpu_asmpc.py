"""Sensitivity-based MPC (do_mpc_amd/asmpc.py, csrc/dompc_asmpc.hip, the plant rollout of csrc/dompc_plant.hip) on the HIP path (twin
of test_asmpc.py)."""
import contextlib

import numpy as np
import pytest

import asmpc_common as ac
import differentiator_batch_common as bc
from test_gpu_parity import make_mpc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B", ac.BATCHES)
@pytest.mark.parametrize("shape", ac.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_law_and_step_match_the_reference_formula(shape, B):
    ac.check_shape(*shape, B, hostemu=False)


def test_zero_leading_entry_is_solved_by_pivoting():
    ac.check_pivoting(hostemu=False)


@pytest.mark.parametrize("shape", [(3, 16), (17, 3), (64, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_law_preparation_with_pivot_orders_that_are_not_the_identity(shape):
    ac.check_pivot_orders(*shape, hostemu=False)


def test_singular_failed_and_nan_members_fall_back_and_stay_local():
    ac.check_fallbacks(hostemu=False)


def test_clip_infinite_bounds_nan_state_and_max_dx():
    ac.check_clip_nan_and_max_dx(hostemu=False)


def test_refusals_by_name():
    ac.check_refusals(make_mpc, contextlib.nullcontext)


@pytest.mark.parametrize("name", ["batch_reactor", "CSTR"])
def test_solve_and_step_equal_the_example_class(name):
    ac.check_solve_equals_example(make_mpc, name, hostemu=False)


@pytest.mark.parametrize("name", ["batch_reactor", "CSTR"])
def test_make_step_equals_row_0_of_the_batched_loop(name):
    ac.check_make_step_equals_row0(make_mpc, name, hostemu=False)


@pytest.mark.parametrize("name", ["batch_reactor", "CSTR"])
def test_fused_run_equals_stepwise_run(name):
    ac.check_fused_equals_stepwise(make_mpc, name, hostemu=False)


def test_fused_run_equals_stepwise_run_with_plant_parameters_that_change_with_time():
    ac.check_fused_equals_stepwise(make_mpc, "CSTR", hostemu=False, varying=True)


def test_rollout_with_a_law_from_set_law_equals_the_stepwise_launches():
    ac.check_rollout_with_synthetic_law(hostemu=False)


def test_rollout_refuses_a_plant_with_algebraic_states():
    ac.check_dae_plant_is_refused(make_mpc, hostemu=False)


@pytest.mark.parametrize("name", ["batch_reactor", "CSTR"])
def test_resolve_every_1_is_the_mpc_loop(name):
    """resolve_every = 1 over 3 steps against BatchClosedLoop from the same start: equal u0 and x, bit for bit - the law at x = x_ref
    adds an exact zero to the solver's u0, and the solve calls are the same"""
    from do_mpc_amd.closed_loop import BatchClosedLoop
    X0 = bc.batch_states(name)
    loop = ac.make_loop(make_mpc, name, False, 1)
    ref = BatchClosedLoop(make_mpc(name, max_batch=5), ac.make_plant(name, False), X0)
    for k in range(3):
        r, q = loop.step(), ref.step()
        assert r["solved"] and r["stats"]["success"].all() and q["stats"]["success"].all()
        du, dx = float(np.max(np.abs(r["u0"] - q["u0"]))), float(np.max(np.abs(r["x"] - q["x"])))
        print(f"{name} step {k}: max |u - u_mpc| = {du:.3e}, max |x - x_mpc| = {dx:.3e}, law status {r['law_status']}")
        assert np.array_equal(r["u0"], q["u0"]) and np.array_equal(r["x"], q["x"]), (k, du, dx)


def test_solve_device_equals_solve():
    """the device-resident chain solve -> sensitivities -> law against ASMPC.solve on host arrays: the same law"""
    import torch
    name = "batch_reactor"
    mpc, a, r = ac.solved(make_mpc, name, hostemu=False)
    host = a.law
    loop = ac.make_loop(make_mpc, name, False, 3)
    loop._solve()
    torch.cuda.synchronize()
    dev = loop.asmpc.law
    assert np.array_equal(dev["flags"], host["flags"]) and np.array_equal(dev["x_ref"], host["x_ref"])
    assert np.array_equal(dev["u_ref"], host["u_ref"]) and np.array_equal(dev["M"], host["M"])
