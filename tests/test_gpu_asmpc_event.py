"""Event-triggered re-solves of sensitivity-based MPC (do_mpc_amd/asmpc.py, closed_loop.BatchClosedLoopASMPC, the selection and the
scatter of csrc/dompc_asmpc.hip) on the HIP path (twin of test_asmpc_event.py)."""
import pytest

import asmpc_event_common as ec
from test_gpu_parity import make_mpc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B", ec.SELECT_BATCHES)
def test_select_lists_the_flagged_members_in_order(B):
    ec.check_select(B, hostemu=False)


@pytest.mark.parametrize("B", ec.LARGE_SELECT_BATCHES)
def test_select_across_more_than_select_threads_workgroups(B):
    """B = 257 SPAN + 1: workgroup 257 (counted from 0) takes a second round in the strided sum over the counts of the workgroups before it"""
    ec.check_select_large(B, hostemu=False)


@pytest.mark.parametrize("shape", [(4, 2), (17, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_set_law_members_writes_the_named_columns_only(shape):
    ec.check_scatter(*shape, hostemu=False)


def test_fallbacks_through_set_law_members_flag_their_own_column():
    ec.check_scatter_fallbacks(hostemu=False)


def test_duplicate_and_out_of_range_members_are_refused_on_the_host():
    ec.check_member_refusals(hostemu=False)


@pytest.mark.parametrize("name", ["batch_reactor", "CSTR"])
def test_event_mode_that_selects_every_member_is_the_mpc_loop(name):
    ec.check_all_selected_is_the_mpc_loop(make_mpc, name)


@pytest.mark.parametrize("name", ["batch_reactor", "CSTR"])
def test_event_mode_that_selects_nothing_is_the_periodic_loop(name):
    ec.check_nothing_selected_is_todays_loop(make_mpc, name, hostemu=False)


@pytest.mark.parametrize("name", ["batch_reactor", "CSTR"])
def test_selected_members_equal_a_solve_of_those_members_and_the_rest_is_untouched(name):
    ec.check_some_members_selected(make_mpc, name, hostemu=False)


@pytest.mark.parametrize("name", ["batch_reactor", "CSTR"])
def test_make_step_with_events_on_every_call_equals_resolve_every_1(name):
    ec.check_make_step_event(make_mpc, name, hostemu=False)


def test_fused_run_is_refused_with_event_triggered():
    ec.check_fused_is_refused(make_mpc, hostemu=False)
