"""The synthetic shape family (tests/riccati_shape_common.py) on the device: the matrix-core Riccati recursion at the shapes no shipped
model reaches, and the generic device recursion one past its limits."""
import pytest

import riccati_shape_common as rs
from do_mpc_amd.examples import CASES

pytestmark = pytest.mark.gpu


def make_mpc(name, **kw):
    ex = CASES[name]
    return ex.build_mpc(ex.build_model(), **kw)


@pytest.mark.parametrize("mid", rs.IDS)
def test_device_runs_the_recursion_the_shape_selects(mid):
    mpc = make_mpc(rs.name_of(mid))
    rs.check_shape(mpc, mid)
    assert mpc.S.riccati_kind == rs.MEMBERS[mid][8]
    print("riccati_shapes kind %s riccati_kind=%d edges_per_wavefront=%d" % (mid, mpc.S.riccati_kind, mpc.S.edges_per_wavefront))
    if mid == "s7":
        assert mpc.S.edges_per_wavefront == 1          # (NX + NU + 2 > 16: no four-edge sweep, csrc/dompc_edge.h QUAD_EDGE)


@pytest.mark.parametrize("name", ["industrial_poly", "CSTR"])
def test_shipped_models_run_the_matrix_core_recursion(name):
    assert make_mpc(name).S.riccati_kind == 1


@pytest.mark.parametrize("delta", rs.DELTAS)
@pytest.mark.parametrize("mid", rs.IDS)
def test_newton_direction_matches_sparse_kkt_solve(mid, delta):
    """dx within 100 x the host emulation's own deviation from the sparse reference (riccati_shape_common.HOST_DX), at most STEP_TOL"""
    rs.check_newton_direction(make_mpc, mid, delta, rs.gpu_dx_bound(mid, delta))


@pytest.mark.parametrize("mid", rs.IDS)
def test_cold_solve_takes_the_oracles_iterates(mid):
    rs.check_cold_solve(make_mpc, mid)


@pytest.mark.parametrize("mid", ["s4", "s7"])
def test_members_of_a_batch_equal_single_solves(mid):
    rs.check_batch_members(make_mpc, mid)


def test_sensitivities_with_several_nl_cons_rows_match_the_oracles_sparse_kkt_solve():
    rs.check_sensitivities(make_mpc)
