"""The synthetic shape family (tests/riccati_shape_common.py) on the test-only host emulation: the family, its lowering, the oracle case and
the sparse Newton reference with nl_cons rows are validated here before tests/test_gpu_riccati_shapes.py runs them on the device.  The host
emulation runs the generic Riccati recursion for every member."""
import pytest

import hostemu
import parity_common as pc
import riccati_shape_common as rs
from do_mpc_amd.examples import CASES


def make_mpc(name, **kw):
    ex = CASES[name]
    with hostemu.patched():
        return ex.build_mpc(ex.build_model(), **kw)


@pytest.mark.parametrize("mid", rs.IDS)
def test_oracle_solution_has_the_active_set_the_family_is_built_for(mid):
    rs.check_oracle_active_set(mid)


@pytest.mark.parametrize("delta", rs.DELTAS)
@pytest.mark.parametrize("mid", rs.IDS)
def test_newton_direction_matches_sparse_kkt_solve(mid, delta):
    """(the host emulation's own deviation is what the GPU bound is derived from: it must itself lie inside that bound)"""
    rep = rs.check_newton_direction(make_mpc, mid, delta, pc.STEP_TOL)
    assert rep["dx"] <= rs.gpu_dx_bound(mid, delta), (rep["dx"], rs.HOST_DX[(mid, delta)])


@pytest.mark.parametrize("mid", rs.IDS)
def test_cold_solve_takes_the_oracles_iterates(mid):
    mpc = rs.check_cold_solve(make_mpc, mid)
    assert mpc.S.riccati_kind == 0          # (host emulation: always the generic recursion)


@pytest.mark.parametrize("mid", ["s4", "s7"])
def test_members_of_a_batch_equal_single_solves(mid):
    rs.check_batch_members(make_mpc, mid)


def test_sensitivities_with_several_nl_cons_rows_match_the_oracles_sparse_kkt_solve():
    rs.check_sensitivities(make_mpc)
