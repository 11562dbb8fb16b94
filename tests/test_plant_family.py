"""Batched plant integrator (csrc/dompc_plant.hip) on lanes that do unequal work, on the host emulation of its kernel: the probe
family of tests/plant_family_common.py against its closed form and against a numpy twin of the explicit pair, and the references
themselves."""
import numpy as np
import pytest

import plant_family_common as pf


# ---------------------------------------------------------------------------------------------------- the references
def test_twin_tableau_satisfies_the_order_conditions_in_rationals():
    assert all(r == 0 for r in pf.order_condition_residuals(pf.DP_B, 5))
    assert all(r == 0 for r in pf.order_condition_residuals([b - e for b, e in zip(pf.DP_B, pf.DP_E)], 4))
    assert any(r != 0 for r in pf.order_condition_residuals(pf.DP_BHAT, 5))          # (the embedded weights are of order 4 only)
    assert all(sum(row) == c for row, c in zip(pf.DP_A[1:], pf.DP_C[1:]))              # row sums
    assert sum(pf.DP_E) == 0 and pf.DP_E[1] == 0


def test_closed_form_matches_the_matrix_exponential():
    """(expm of a matrix of norm 1e4 t_step: scaling and squaring loses a few digits)"""
    assert pf.closed_form_against_expm(pf.reference()["inp"], range(130)) < 1e-12


def test_twin_converges_to_the_closed_form_and_conditions_on_the_batch_hold():
    for tol in (1e-10, 1e-6):
        ref = pf.reference(tol)                            # (asserts the margins and the mix of lanes per wavefront)
        expl = ref["explicit"]
        assert pf.relerr(ref["twin"]["x"], ref["x"])[expl].max() < tol


def test_first_pivot_of_the_algebraic_jacobian_is_zero():
    assert np.array_equal(pf.alg_jacobian(pf.build_model("dae")), [[0.0, 1.0], [1.0, 0.0]])


# ---------------------------------------------------------------------------------------------------- the kernel's host emulation
@pytest.mark.parametrize("B", pf.SIZES)
@pytest.mark.parametrize("kind", ["ode", "dae"])
def test_values_status_and_step_counts(kind, B):
    pf.check_values(kind, hostemu=True, B=B)


def test_explicit_pair_alone_reports_the_step_limit():
    pf.check_explicit_only(hostemu=True)


@pytest.mark.parametrize("kind", ["ode", "dae"])
def test_implicit_method_alone(kind):
    pf.check_implicit_only(kind, hostemu=True)


def test_looser_tolerance_takes_fewer_steps():
    pf.check_looser_tolerance(hostemu=True)


def test_failures_stay_local():
    pf.check_failures_stay_local(hostemu=True)


@pytest.mark.parametrize("kind", ["ode", "dae"])
def test_rows_do_not_depend_on_their_position(kind):
    pf.check_position(kind, hostemu=True)


@pytest.mark.parametrize("kind", ["ode", "dae"])
def test_shared_rows_equal_tiled_rows(kind):
    pf.check_shared_rows(kind, hostemu=True)


def test_discrete_member_equals_numpy():
    pf.check_discrete(hostemu=True)


def test_dip_newton_starts_survive_a_growing_batch():
    pf.check_dip_growing_z_buffer(hostemu=True)


def test_dip_permutation_across_the_wavefront_boundary():
    pf.check_dip_permutation(hostemu=True)
