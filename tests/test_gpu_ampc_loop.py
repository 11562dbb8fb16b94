"""The fused approximate-MPC loop on the GPU (tests/ampc_loop_common.py; dompc_ampc_loop_kernel of the prebuilt pairs,
__graft_entry__.PREBUILT_AMPC_LOOP): one launch of K control steps against K pairs of step-wise launches, bit for bit."""
import pytest

import ampc_loop_common as lc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B", lc.LANE_B)
def test_lane_layout(B):
    lc.check_lane_layout(False, B)


def test_previous_inputs():
    lc.check_previous_inputs(False)


@pytest.mark.parametrize("n", (2, 3))
def test_shapes(n):
    lc.check_shape(False, n)


@pytest.mark.parametrize("n", (4, 5))
def test_unequal_work_noise_parameters(n):
    lc.check_family(False, n)


@pytest.mark.parametrize("n", (1, 4))
def test_loop(n):
    lc.check_loop(False, n)


def test_closed_loop_copies():
    lc.check_closed_loop_copies(False)


def test_weights_are_data():
    lc.check_weights_are_data(False)


def test_refusals():
    lc.check_refusals(False)
