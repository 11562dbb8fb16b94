"""LQR for models with algebraic states on the host emulation of csrc/dompc_lqr.hip (the text that ships, compiled by g++ with
-DDOMPC_HOST_EMU): the reference's route dae2odeconversion -> linearize -> LQR with its stored run, and the batched route, the
index-1 reduction inside the design kernel (LQR.gains_at on the DAE model), against a numpy twin.  The GPU runs the same checks in
tests/test_gpu_lqr_dae.py.  Bounds of the twin comparisons: those of lqr_common.check_family_b (tests/lqr_dae_common.py)."""
import numpy as np
import pytest

import lqr_dae_common as dc
from do_mpc_amd import casadi_compat, lowering, sym
from do_mpc_amd.examples import CASES
from do_mpc_amd.model import LinearModel, Model, dae2odeconversion, linearize


# ---------------------------------------------------------------------------------------------- the reference's route
def test_batch_reactor_dae_loop_reproduces_the_stored_run():
    """50 steps of examples/lqr_examples/batch_reactor_lqr_dae/main.py against the stored run; bound: the reference's own 1e-8,
    absolute (testing/test_batch_reactor_lqr_dae.py).  Measured on the host emulation: _x 1.68e-9, _u 7.5e-10, _time 0 - the stored
    run was integrated by CVODES at its default tolerances, the batched Dormand-Prince plant reaches the bound as it stands.  _z: the
    converted model has no algebraic state, the record is empty on both sides."""
    (dx, du, dt), z_shape, z_stored = dc.replay(hostemu=True)
    assert dx < 1e-8 and du < 1e-8 and dt < 1e-8
    assert z_shape == z_stored == (50, 0)


def test_dae2odeconversion_carries_names_input_rate_and_noise_flags():
    m = Model("continuous")
    a = m.set_variable("_x", "a")
    b = m.set_variable("_x", "b", (2, 1))
    u = m.set_variable("_u", "u", (2, 1))
    z = m.set_variable("_z", "z", (2, 1))
    p = m.set_variable("_p", "p")
    tv = m.set_variable("_tvp", "tv")
    m.set_rhs("a", -p * a + u[0] + z[0], process_noise=True)
    m.set_rhs("b", sym.vertcat(a - b[0] * tv, z[1] - b[1] + u[1]))
    m.set_alg("g", sym.vertcat(2 * z[0] + z[1] - a * b[0], z[1] * (1 + a * a) - u[0] - b[1]))
    with pytest.raises(AssertionError, match="Run this function after original model is setup"):
        dae2odeconversion(m)
    m.setup()
    ode = dae2odeconversion(m)
    assert ode.model_type == "continuous" and ode._x.names == ["a", "b", "u", "z"] and ode.n_x == 7 and ode.n_z == 0
    assert [n for n in ode._u.names if n != "default"] == ["q"] and ode._u.vars["q"].shape == (2, 1)
    assert [n for n in ode._p.names if n != "default"] == ["p"] and [n for n in ode._tvp.names if n != "default"] == ["tv"]
    assert [n for n in ode._w.names if n != "default"] == ["a_noise"]          # the flag of `a` alone
    # z' = -g_z^-1 (g_x f + g_u q) at a consistent point, against numpy
    rng = np.random.default_rng(1)
    x, uu, q, pp, tt = rng.uniform(0.5, 1.5, 3), rng.uniform(-1, 1, 2), rng.uniform(-1, 1, 2), np.array([0.7]), np.array([1.3])
    z1 = (uu[0] + x[2]) / (1 + x[0] ** 2)
    zz = np.array([(x[0] * x[1] - z1) / 2, z1])
    f = m._rhs_fun.eval(x, uu, zz, tt, pp, np.zeros(1))[0]
    gz = np.array([[2.0, 1.0], [0.0, 1 + x[0] ** 2]])
    gx = np.array([[-x[1], -x[0], 0.0], [2 * x[0] * zz[1], 0.0, -1.0]])
    gu = np.array([[0.0, 0.0], [-1.0, 0.0]])
    want = np.concatenate([f, q, -np.linalg.solve(gz, gx @ f + gu @ q)])
    have = ode._rhs_fun.eval(np.concatenate([x, uu, zz]), q, np.zeros(0), tt, pp, np.zeros(1))[0]
    assert dc.relerr(have, want) < 1e-14
    # the converted batch reactor is linear: linearize needs no operating point
    lin = linearize(dae2odeconversion(CASES["batch_reactor_lqr_dae"].build_dae_model()))
    assert isinstance(lin, LinearModel) and lin.sys_A.shape == (5, 5) and lin.sys_B.shape == (5, 1)
    assert np.array_equal(lin.sys_A[4], [0.0, 1.0, 0.0, 0.0, -1.0]) and np.array_equal(lin.sys_B.ravel(), [0, 0, 0, 1, 0])
    with pytest.raises(NotImplementedError, match="LTV models are not yet implemented."):
        linearize(ode)
    with pytest.raises(ValueError, match="class LinearModel can be initialized only with SX variable."):
        CASES["batch_reactor_lqr_dae"].build_model("MX")


def test_symbolic_inverse_against_numpy():
    """sym.inv on random 1 x 1 to 4 x 4 matrices of symbols, substituted, against np.linalg.inv (condition number <= 1e3 by
    construction: bound 1e-11 = 1e3 * 1e-14), one of them with a structural zero on the diagonal; constants fold to constants and a
    structurally singular matrix is refused by name"""
    rng = np.random.default_rng(0)
    for n in (1, 2, 3, 4, 4):
        S = sym.SX.sym("m", n, n)
        val = dc._conditioned(rng, n)
        assert dc.relerr(sym.Function("inv", [S], [sym.inv(S)]).eval(val.reshape(-1, order="F"))[0].reshape((n, n), order="F"), np.linalg.inv(val)) < 1e-11
    S = sym.SX.sym("m", 3, 3)
    M = sym.SX(S)
    M[0, 0] = 0.0                                          # structural zero on the diagonal: the pivot is taken below it
    val = dc._conditioned(rng, 3, zero00=True)
    have = sym.Function("inv", [S], [sym.inv(M)]).eval(val.reshape(-1, order="F"))[0].reshape((3, 3), order="F")
    assert dc.relerr(have, np.linalg.inv(val)) < 1e-11
    C = np.array([[0.0, 2.0], [4.0, 1.0]])
    assert sym.inv(sym.SX(C)).is_constant() and dc.relerr(sym.inv(sym.SX(C)).to_numpy(), np.linalg.inv(C)) < 1e-15
    assert "inv" in casadi_compat._CASADI_NAMES
    with pytest.raises(RuntimeError, match="structurally singular"):
        sym.inv(sym.SX(np.array([[1.0, 0.0], [2.0, 0.0]])))
    with pytest.raises(ValueError, match="square"):
        sym.inv(sym.SX.sym("r", 2, 3))


# ---------------------------------------------------------------------------------------------- the reduction against the twin
def test_batch_reactor_designs_against_the_twin():
    """(a) measured on the host emulation: K 4.6e-16, discrete pair 7.8e-16, Z 0"""
    dc.check_batch_reactor(hostemu=True)


def test_elimination_pivots_over_the_lanes():
    """(b) measured: K 5.6e-16, pair 1.1e-16, Z 2.2e-16"""
    dc.check_pivoting(hostemu=True)


def test_newton_converges_member_by_member_inside_one_wavefront():
    """(c) Newton updates [2 12 5 4 3 10 7]; measured: K 6.3e-14, pair 8.2e-16, Z 0"""
    dc.check_newton_in_one_wavefront(hostemu=True)


@pytest.mark.parametrize("name", ["nz16", "nx15_rate"])
def test_size_limits(name):
    """(d) measured: n_z = 16: K 1.0e-15, pair 6.7e-16, Z 6.6e-15; n_x = 15 in rate mode: K 8.6e-16, pair 2.0e-15"""
    dc.check_size_limits(True, name)


def test_lowering_refuses_by_name_what_lies_beyond_the_limits():
    big = dc.linear_g_model(33, 2, 1, 17, discrete=True)
    kw = lambda m: dict(x_sym=m._x.cat.nodes(), u_sym=m._u.cat.nodes(), z_sym=m._z.cat.nodes(), rhs=m._rhs.nodes(), alg=m._alg.nodes())      # noqa: E731
    with pytest.raises(NotImplementedError, match="more than 16 algebraic states"):
        lowering.lower_lqr(nx=2, nu=1, rate=False, **kw(big))
    wide = dc.linear_g_model(34, 15, 2, 1, discrete=False)
    with pytest.raises(NotImplementedError, match="N > 16"):
        lowering.lower_lqr(nx=15, nu=2, rate=True, discrete=False, **kw(wide))
    with pytest.raises(NotImplementedError, match="n_x \\+ n_u > 16"):
        lowering.lower_lqr(nx=15, nu=2, rate=False, discrete=False, **kw(wide))
    hdr = lowering.lower_lqr(nx=15, nu=2, rate=False, discrete=True, **kw(wide))
    assert "#define LQR_NZ 1" in hdr and "LQR_GZ_NZ" in hdr
    assert "LQR_NZ" not in lowering.lower_lqr(nx=3, nu=1, rate=False)          # designs without algebraic states: the text they had


def test_batch_sizes_with_and_without_z_out():
    dc.check_batch_sizes_and_z_out(hostemu=True)


def test_the_oscillating_masses_dae_model_designs():
    """(f) measured: K 1.0e-14, pair 0, Z 0"""
    dc.check_oscillating_masses_dae(hostemu=True)


def test_status_bit_2_and_neighbours():
    dc.check_status(hostemu=True)


def test_linearize_dae_is_the_host_statement_of_the_reduction():
    dc.check_linearize_dae(hostemu=True)


def test_batch_closed_loop_on_the_dae_plant():
    dc.check_closed_loop(hostemu=True)
