"""Event-triggered re-solves of sensitivity-based MPC (do_mpc_amd/asmpc.py, closed_loop.BatchClosedLoopASMPC, the selection and the
scatter of csrc/dompc_asmpc.hip) on the TEST-ONLY host emulation of the kernels (the -m gpu twin: test_gpu_asmpc_event.py, which also
holds the comparison with BatchClosedLoop - that loop has no host flavour)."""
import pytest

import asmpc_event_common as ec
from test_hostemu_parity import make_mpc


def test_select_span_is_the_kernels():
    ec.check_span_constant()


@pytest.mark.parametrize("B", ec.SELECT_BATCHES)
def test_select_lists_the_flagged_members_in_order(B):
    ec.check_select(B, hostemu=True)


@pytest.mark.parametrize("B", ec.LARGE_SELECT_BATCHES)
def test_select_across_more_than_select_threads_workgroups(B):
    """(a serial loop on the host emulation: the strided sum over more than SELECT_THREADS workgroups exists on the device only)"""
    ec.check_select_large(B, hostemu=True)


@pytest.mark.parametrize("shape", [(4, 2), (17, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_set_law_members_writes_the_named_columns_only(shape):
    ec.check_scatter(*shape, hostemu=True)


def test_fallbacks_through_set_law_members_flag_their_own_column():
    ec.check_scatter_fallbacks(hostemu=True)


def test_duplicate_and_out_of_range_members_are_refused_on_the_host():
    ec.check_member_refusals(hostemu=True)


@pytest.mark.parametrize("name", ["batch_reactor", "CSTR"])
def test_event_mode_that_selects_nothing_is_the_periodic_loop(name):
    ec.check_nothing_selected_is_todays_loop(make_mpc, name, hostemu=True)


@pytest.mark.parametrize("name", ["batch_reactor", "CSTR"])
def test_selected_members_equal_a_solve_of_those_members_and_the_rest_is_untouched(name):
    ec.check_some_members_selected(make_mpc, name, hostemu=True)


@pytest.mark.parametrize("name", ["batch_reactor", "CSTR"])
def test_make_step_with_events_on_every_call_equals_resolve_every_1(name):
    ec.check_make_step_event(make_mpc, name, hostemu=True)


def test_fused_run_is_refused_with_event_triggered():
    ec.check_fused_is_refused(make_mpc, hostemu=True)
