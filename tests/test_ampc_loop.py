"""The fused approximate-MPC loop on the host emulation (tests/ampc_loop_common.py; csrc/dompc_ampc_loop.hip compiled by g++): one
launch of K control steps against K pairs of step-wise launches, bit for bit.  The GPU suite runs the same checks on the prebuilt pairs
(tests/test_gpu_ampc_loop.py)."""
import pytest

import ampc_common as amc
import ampc_loop_common as lc


@pytest.mark.parametrize("B", lc.LANE_B)
def test_lane_layout(B):
    lc.check_lane_layout(True, B)


def test_previous_inputs():
    lc.check_previous_inputs(True)


@pytest.mark.parametrize("n", (2, 3))
def test_shapes(n):
    lc.check_shape(True, n)


# shapes beyond the prebuilt pairs: two live tiles with padded sigmoid neurons, eight hidden layers without scaling
@pytest.mark.parametrize("case", [amc.FAMILY[4], amc.FAMILY[7]], ids=amc.family_id)
def test_family_shapes(case):
    lc.check_shape(True, 1, B=35, K=2, family=case)


@pytest.mark.parametrize("n", (4, 5))
def test_unequal_work_noise_parameters(n):
    lc.check_family(True, n)


@pytest.mark.parametrize("n", (1, 4))
def test_loop(n):
    lc.check_loop(True, n)


def test_closed_loop_copies():
    lc.check_closed_loop_copies(True)


def test_weights_are_data():
    lc.check_weights_are_data(True)


def test_refusals():
    lc.check_refusals(True)
