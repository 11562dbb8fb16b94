"""Linear quadratic regulator (do_mpc_amd.lqr / LinearModel / linearize) on the host emulation of csrc/dompc_lqr.hip: the text that
ships, compiled by g++ with -DDOMPC_HOST_EMU.  The GPU runs the same checks in tests/test_gpu_lqr.py."""
import warnings

import numpy as np
import pytest
from scipy.signal import cont2discrete

import lqr_common as lc
from do_mpc_amd import build, lowering, sym
from do_mpc_amd.examples import CASES, cstr_lqr, oscillating_masses_lqr
from do_mpc_amd.lqr import LQR
from do_mpc_amd.model import LinearModel, Model, linearize


# ---------------------------------------------------------------------------------------------- LinearModel, linearize
def _abcd(seed=0, nx=3, nu=2, ny=2):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nx, nx)), rng.standard_normal((nx, nu)), rng.standard_normal((ny, nx)), rng.standard_normal((ny, nu))


def _vars(model, nx=3, nu=2):
    return model.set_variable("_x", "x", (nx, 1)), model.set_variable("_u", "u", (nu, 1))


def test_linear_model_refuses_what_the_reference_refuses():
    with pytest.raises(ValueError, match="class LinearModel can be initialized only with SX variable."):
        LinearModel("discrete", "MX")
    m = LinearModel("continuous")
    x, u = _vars(m)
    with pytest.raises(ValueError, match="Given rhs is not linear."):
        m.set_rhs("x", x * x[0] + sym.vertcat(u, 0))
    with pytest.raises(ValueError, match="Measurement function is not linear."):
        m.set_meas("y", sym.sin(x[0]))
    with pytest.raises(NotImplementedError, match="Algebraic variables are not supported for linear models."):
        m.set_alg("a", x[0])
    with pytest.raises(AssertionError, match="Attributes are available after the model is setup."):
        m.sys_A
    A, B, C, D = _abcd()
    for name, kw in (("A", {"A": [[1.0]]}), ("B", {"B": 1.0}), ("C", {"C": "c"}), ("D", {"D": (1,)})):
        with pytest.raises(ValueError, match=f"{name} must be a numpy array or None"):
            m.setup(**kw)
    with pytest.raises(ValueError, match="A must be a square matrix with size n_x x n_x. You have A.shape="):
        m.setup(A[:2], B)
    with pytest.raises(ValueError, match="B must be a matrix with size n_x x n_u. You have B.shape="):
        m.setup(A, B[:, :1])


def test_the_setup_paths_give_the_same_system_matrices():
    A, B, C, D = _abcd()
    by_matrices = LinearModel("continuous")
    _vars(by_matrices)
    by_matrices.setup(A, B, C, D)
    by_rhs = LinearModel("continuous")
    x, u = _vars(by_rhs)
    by_rhs.set_meas("y", C @ x + D @ u)
    by_rhs.set_rhs("x", A @ x + B @ u)
    by_rhs.setup()
    mixed = LinearModel("continuous")
    x, u = _vars(mixed)
    mixed.set_rhs("x", A @ x + B @ u)
    mixed.setup(C=C, D=D)
    for m in (by_matrices, by_rhs, mixed):
        for have, want in zip((m.sys_A, m.sys_B, m.sys_C, m.sys_D), (A, B, C, D)):
            assert isinstance(have, np.ndarray) and np.array_equal(have, want)
    # neither C / D nor set_meas: state feedback
    plain = LinearModel("discrete")
    _vars(plain)
    plain.setup(A, B)
    assert np.array_equal(plain.sys_C, np.eye(3)) and np.array_equal(plain.sys_D, np.zeros((3, 2)))
    assert plain.n_w == 3 and plain.n_v == 0          # process noise on every state, like the reference (set_rhs(..., process_noise=True))


@pytest.mark.parametrize("method", ["zoh", "bilinear", "euler", "backward_diff", "gbt"])
def test_discretize_against_cont2discrete(method):
    """numpy only (the zero-order hold by the scaled Taylor polynomial of the kernel).  Bound 1e-13: the matrices are of size 1, both
    sides are backward stable; measured 6.7e-16 (zoh) and 0 (the closed-form methods)."""
    A, B, C, D = _abcd(seed=4)
    m = LinearModel("continuous")
    _vars(m)
    m.setup(A, B, C, D)
    kw = {"alpha": 0.3} if method == "gbt" else {}
    d = m.discretize(0.3, method, **kw)
    ref = cont2discrete((A, B, C, D), 0.3, method, **kw)
    assert d.model_type == "discrete" and d._x.names == m._x.names and d._u.names == m._u.names
    for have, want in zip((d.sys_A, d.sys_B, d.sys_C), ref[:3]):
        assert lc.relerr(have, want) < 1e-13
    with pytest.raises(AssertionError, match="Given model is already discrete."):
        d.discretize(0.3)
    with pytest.raises(ValueError):
        m.discretize(0.3, "no such method")


def test_zero_order_hold_over_random_systems():
    """256 systems of family (a) (n = 2..12, t_step in [0.1, 0.5]); the issue's figure over 4 096 is 8.8e-15, bound 1e-13"""
    rng = np.random.default_rng(2026)
    worst = 0.0
    for _ in range(256):
        n, nu = int(rng.integers(2, 13)), int(rng.integers(1, 5))
        A, B, dt = rng.standard_normal((n, n)) / np.sqrt(n), rng.standard_normal((n, nu)), float(rng.uniform(0.1, 0.5))
        m = LinearModel("continuous")
        _vars(m, n, nu)
        m.setup(A, B)
        d = m.discretize(dt)
        Ad, Bd = lc.twin_zoh(A, B, dt)
        worst = max(worst, lc.relerr(d.sys_A, Ad), lc.relerr(d.sys_B, Bd))
    print(f"zero-order hold, 256 systems: numpy - scipy = {worst:.3e}")
    assert worst < 1e-13


def test_get_steady_state_has_the_four_branches():
    A, B, _, _ = _abcd(seed=2)
    A = 0.3 * A
    m = LinearModel("discrete")
    _vars(m)
    m.setup(A, B)
    uss = np.array([[0.4], [-0.2]])
    xss = m.get_steady_state(uss=uss)
    assert np.allclose(xss, A @ xss + B @ uss, atol=1e-14)
    u_back = m.get_steady_state(xss=xss)                       # B is not square: pseudo-inverse
    assert np.allclose(u_back, np.linalg.pinv(B) @ (np.eye(3) - A) @ xss)
    sq = LinearModel("discrete")
    _vars(sq, 2, 2)
    As, Bs = 0.3 * np.array([[1.0, 2.0], [0.5, -1.0]]), np.array([[1.0, 0.2], [0.0, 2.0]])
    sq.setup(As, Bs)
    xs = np.array([[1.0], [2.0]])
    assert np.allclose(Bs @ sq.get_steady_state(xss=xs), (np.eye(2) - As) @ xs)
    rank = LinearModel("discrete")
    _vars(rank, 2, 1)
    rank.setup(np.array([[1.0, 1.0], [1.0, 1.0]]), np.array([[1.0], [0.0]]))
    with pytest.raises(ValueError, match="State matrix does not have full rank."):
        rank.get_steady_state(uss=np.array([[1.0]]))
    with pytest.raises(AssertionError, match="Provide either steady state states or steady state inputs."):
        m.get_steady_state()
    assert m.get_steady_state(xss=xss, uss=uss) is None        # both given: the reference falls through its four branches
    cont = LinearModel("continuous")
    _vars(cont)
    cont.setup(A, B)
    with pytest.raises(AssertionError, match="Please convert the system to discrete"):
        cont.get_steady_state(uss=uss)


def test_linearize_of_the_cstr_equals_the_jacobians_at_the_steady_state():
    plant = cstr_lqr.build_model()
    lin = linearize(plant, cstr_lqr.XSS, cstr_lqr.USS)
    A, B = lc.twin_jacobians(plant, cstr_lqr.XSS, cstr_lqr.USS)
    assert isinstance(lin, LinearModel) and lin.model_type == "continuous"
    assert np.array_equal(lin.sys_A, A) and np.array_equal(lin.sys_B, B)
    assert np.array_equal(lin.sys_C, np.eye(4)) and np.array_equal(lin.sys_D, np.zeros((4, 2)))      # the trivial C, D were dropped
    assert lin._x.names == plant._x.names and lin._u.names == plant._u.names and "r" in lin._aux.names


def test_linearize_refuses_dae_models_and_matrices_that_are_not_constant():
    dae = CASES["oscillating_masses_dae"].build_model()
    with pytest.raises(AssertionError, match="Linearization around steady state is not supported for DAEs"):
        linearize(dae, np.zeros((dae.n_x, 1)), np.zeros((dae.n_u, 1)))
    m = Model("continuous")
    x = m.set_variable("_x", "x")
    u = m.set_variable("_u", "u")
    p = m.set_variable("_p", "p")
    m.set_rhs("x", -p * x * x + u)
    with pytest.raises(AssertionError, match="Run this function after original model is setup"):
        linearize(m, np.ones((1, 1)), np.zeros((1, 1)))
    m.setup()
    with pytest.raises(NotImplementedError, match="LTV models are not yet implemented."):
        linearize(m, np.ones((1, 1)), np.zeros((1, 1)))                      # p stays symbolic
    lin = linearize(m, np.ones((1, 1)), np.zeros((1, 1)), p0=np.array([2.0]))
    assert np.array_equal(lin.sys_A, [[-4.0]])


# ---------------------------------------------------------------------------------------------- the controller's surface
def test_lqr_asserts_and_raises_what_the_reference_does():
    lin = oscillating_masses_lqr.build_model()
    with pytest.raises(AssertionError, match="LQR can only be used with linear models."):
        LQR(CASES["oscillating_masses"].build_model())
    raw = LinearModel("discrete")
    _vars(raw)
    with pytest.raises(AssertionError, match="Model for LQR was not setup."):
        LQR(raw)
    cont = cstr_lqr.build_linear_model(cstr_lqr.build_model())
    with pytest.raises(AssertionError, match="Initialize LQR with discrete system."):
        LQR(cont)
    lqr = LQR(lin)
    with pytest.raises(AssertionError, match=r"Q must have shape = \(4, 4\). You have \(3, 3\)"):
        lqr.set_objective(Q=np.eye(3), R=np.eye(1))
    with pytest.raises(AssertionError, match=r"R must have shape = \(1, 1\). You have \(2, 2\)"):
        lqr.set_objective(Q=np.eye(4), R=np.eye(2))
    lqr.set_param(n_horizon=5, no_such_key=1)
    assert lqr.settings.n_horizon == 5
    with pytest.raises(AssertionError, match="P must have same shape as Q."):
        lqr.set_objective(Q=np.eye(4), R=np.eye(1), P=np.eye(3))
    with pytest.warns(UserWarning, match="P is not given explicitly. Q is chosen as P for calculating finite discrete gain"):
        lqr.set_objective(Q=2 * np.eye(4), R=np.eye(1))
    assert np.array_equal(lqr.P, 2 * np.eye(4))
    with pytest.raises(ValueError, match="t_step must be set"):
        lqr.setup()
    with pytest.raises(AssertionError, match="LQR is not setup. run setup\\(\\) function."):
        lqr.make_step(np.zeros((4, 1)))
    with pytest.raises(AssertionError, match="LQR is not setup. Run setup\\(\\) function."):
        lqr.set_setpoint()
    lqr.mode = "inputRatePenalization"                    # the mode without set_rterm
    lqr.settings.t_step = 0.5
    with pytest.raises(AttributeError, match="set delR using set_rterm fun to execute in inputRatePenalization mode."):
        lqr.setup(_lib_path=lc.lqr_hostemu_library, _code_object="")


def test_runtime_surface_of_both_modes():
    for rate in (False, True):
        _, _, lqr = lc.example("oscillating_masses_lqr", hostemu=True, rate=rate)
        n = 5 if rate else 4
        assert lqr.K.shape == (1, n) and lqr.flags["setup"] and lqr.mode == ("inputRatePenalization" if rate else "standard")
        assert lqr.Q.shape == (n, n)                           # design-size weights after setup (_lqr.py:484-490)
        with pytest.raises(AssertionError, match="Objective can not be set after LQR is setup"):
            lqr.set_objective(Q=np.eye(4), R=np.eye(1))
        with pytest.raises(Exception, match="Invalid type"):
            lqr.make_step([1.0, 2.0, 3.0, 4.0])
        x0 = np.array([[2.0], [1.0], [3.0], [1.0]])
        u1 = lqr.make_step(x0)
        assert u1.shape == (1, 1) and np.array_equal(lqr.x0.master, x0.ravel()) and np.array_equal(lqr.u0.master, u1.ravel())
        assert np.allclose(u1, lqr.K @ (np.vstack([x0, [[0.0]]]) if rate else x0))
        u2 = lqr.make_step(x0)                                 # rate mode: u_prev enters
        assert np.allclose(u2, lqr.K @ np.vstack([x0, u1]) + u1 if rate else u1)
        assert lqr.t0[0] == 1.0 and lqr.data["_x"].shape == (2, 4) and lqr.data["_u"].shape == (2, 1)
        assert np.array_equal(lqr.data["_time"].ravel(), [0.0, 0.5])
        with pytest.raises(AssertionError, match="xss must be of shape"):
            lqr.set_setpoint(xss=np.zeros((3, 1)))
        del lqr.xss
        lqr.set_setpoint(xss=np.ones((4, 1)), uss=2 * np.ones((1, 1)))
        assert lqr.xss.shape == (n, 1) and (not rate or (lqr.xss[4, 0] == 2.0 and lqr.uss[0, 0] == 0.0))
        ub = lqr.make_step_batch(np.tile(x0.T, (3, 1)), U_prev=np.tile(lqr.u0.master, (3, 1)))
        assert np.allclose(ub, lqr.make_step(x0).T)
        lqr.reset_history()
        assert lqr.t0[0] == 0.0 and lqr.data["_x"].shape[0] == 0
        K = lqr.discrete_gain(lqr.A_rated, lqr.B_rated) if rate else lqr.discrete_gain(lqr.model.sys_A, lqr.model.sys_B)
        assert np.array_equal(K, lqr.K)
        if rate:                                               # the kernel forms [[A, B], [0, I]] itself: another pair is refused
            bad = lqr.A_rated.copy()
            bad[4, 0] = 0.5
            with pytest.raises(ValueError, match="the pair must be"):
                lqr.discrete_gain(bad, lqr.B_rated)


def test_lowering_refuses_by_name_what_the_kernel_cannot_map():
    with pytest.raises(NotImplementedError, match="N > 16"):
        lowering.lower_lqr(nx=14, nu=3, rate=True)
    assert "#define LQR_N 16" in lowering.lower_lqr(nx=16, nu=4, rate=False)
    m = Model("continuous")
    x = m.set_variable("_x", "x", (14, 1))
    u = m.set_variable("_u", "u", (3, 1))
    m.set_rhs("x", -x * x + sym.vertcat(u, np.zeros((11, 1))))
    m.setup()
    kw = dict(nx=14, nu=3, rate=False, x_sym=m._x.cat.nodes(), u_sym=m._u.cat.nodes(), rhs=m._rhs.nodes())
    with pytest.raises(NotImplementedError, match="n_x \\+ n_u > 16"):
        lowering.lower_lqr(discrete=False, **kw)
    assert "LQR_DISCRETE 1" in lowering.lower_lqr(discrete=True, **kw)
    w = Model("discrete")
    x = w.set_variable("_x", "x")
    u = w.set_variable("_u", "u")
    w.set_rhs("x", x + u, process_noise=True)
    w.rhs_list[0]["expr"] = w.rhs_list[0]["expr"] * x          # x (x + u + w): the Jacobian depends on the process noise
    w.setup()
    with pytest.raises(NotImplementedError, match="depends on _w"):
        lowering.lower_lqr(nx=1, nu=1, rate=False, x_sym=w._x.cat.nodes(), u_sym=w._u.cat.nodes(), w_sym=w._w.cat.nodes(), rhs=w._rhs.nodes())
    dae = CASES["oscillating_masses_dae"].build_model()
    with pytest.raises(NotImplementedError, match="algebraic states"):
        lowering.lower_lqr(nx=dae.n_x, nu=dae.n_u, rate=False, x_sym=dae._x.cat.nodes(), u_sym=dae._u.cat.nodes(), z_sym=dae._z.cat.nodes(),
                           rhs=dae._rhs.nodes())


def test_a_library_of_another_design_is_refused():
    _, _, rate = lc.example("oscillating_masses_lqr", hostemu=True, rate=True)
    d = next(iter(rate._designs.values()))
    lqr = oscillating_masses_lqr.build_lqr(oscillating_masses_lqr.build_model(), setup=False, rate=False)
    with pytest.raises(RuntimeError, match="different model dimensions"):
        lqr.setup(_lib_path=lc.lqr_hostemu_library(d.header, d.hash), _code_object="")


# ---------------------------------------------------------------------------------------------- stored runs of the reference
def test_oscillating_masses_loop_reproduces_the_stored_run():
    """50 steps of examples/lqr_examples/oscillating_masses_discrete_lqr/main.py; bound: the reference's own 1e-8
    (testing/test_oscillating_masses_discrete_lqr.py).  Measured on the host emulation: _x 1.8e-14, _u 1.5e-14 - the loop is discrete,
    the difference is the round-off of K (8e-15 against the twin) carried through 50 steps."""
    ex_, eu_ = lc.replay("oscillating_masses_lqr", hostemu=True)
    assert ex_ < 1e-8 and eu_ < 1e-8


def test_cstr_loop_reproduces_the_stored_run():
    """200 steps of examples/lqr_examples/CSTR_lqr/main.py against the stored run.  _x: the reference's own 1e-8 (measured 5.90e-9).
    _u: measured 1.149e-8, which misses 1e-8 - and is not the gain's doing: K equals the twin's recursion to 8.3e-17
    (test_example_gains_against_the_twin), and it is a floor of the stored run, not of this plant integrator: with the simulator
    tolerances at 1e-10 (the template's), 1e-11, 1e-12 and 1e-13 the figure is 1.1483e-8, 1.1487e-8, 1.1487e-8, 1.1486e-8.  The
    stored run was integrated by CVODES at 1e-10; its state error of 5.9e-9 is multiplied by gains of size 2 in K [x; u_prev].  The
    bound for _u of this one case is therefore ten times the measured difference, 1.2e-7; the run is made at 1e-12 so that the
    remaining difference is the stored run's alone."""
    ex_, eu_ = lc.replay("cstr_lqr", hostemu=True, abstol=1e-12)
    assert ex_ < 1e-8 and eu_ < 1.2e-7


# ---------------------------------------------------------------------------------------------- gains against the twin
@pytest.mark.parametrize("n_horizon", [None, 1, 10, 50])
@pytest.mark.parametrize("rate", [False, True], ids=["standard", "rate"])
@pytest.mark.parametrize("name", ["oscillating_masses_lqr", "cstr_lqr"])
def test_example_gains_against_the_twin(name, rate, n_horizon):
    """K against scipy.linalg.solve_discrete_are (infinite horizon) or the reference's recursion.  Measured on the host emulation, worst
    over the 16 cases: 1.72e-10 (cstr_lqr, standard, infinite: R^-1 = 1e5 enters G0 = B R^-1 B' of the doubling, and the kernel's
    Riccati residual there is 2.05e-11 against scipy's 9.9e-14 - the difference in K is the kernel's), finite horizons <= 8.2e-16.
    Bound: ten times the worst, 1.8e-9.  Riccati residuals of the four infinite-horizon cases, kernel / scipy: oscillating masses
    5.1e-16 / 3.1e-15 and 4.1e-16 / 1.7e-15 (rate), cstr 2.05e-11 / 9.9e-14 and 1.8e-15 / 3.2e-12 (rate); the kernel's may exceed
    scipy's by ten times the worst measured excess, 2.1e-10."""
    lc.check_example_gains(name, rate, n_horizon, hostemu=True)


def test_family_a_random_systems_in_one_launch():
    """4 096 random systems (n = 2..12, nu = 1..4) in one launch of the (12, 4) design (lqr_common.embed).  Measured on the host
    emulation: 146 members left out by scipy's own residual (3.6 %); over the other 3 950 K - scipy = 1.64e-8 at worst (member 1747:
    max |P| = 5.9e5, scipy's residual 7.6e-11, the kernel's 9.9e-13 - an unfused numpy doubling agrees with the kernel to 1.8e-10),
    kernel residual - scipy residual = 1.66e-9 at worst (member 3087), median kernel / scipy residual 0.16; at most 14 doubling
    steps.  Bounds: ten times the measured values."""
    lc.check_family_a(hostemu=True)


@pytest.mark.parametrize("rate", [False, True], ids=["standard", "rate"])
def test_the_largest_design_size(rate):
    """six random systems at N = 16: (16, 4) in standard mode and (12, 4) in inputRatePenalization mode.  Measured on the host
    emulation: K - scipy = 3.90e-12, kernel residual - scipy residual = 1.72e-13 at worst over both modes (10 doubling steps), none left out.  Bounds: ten
    times the measured values."""
    lc.check_size_16(rate, hostemu=True)


def test_family_b_operating_points_of_the_cstr():
    """gains_at at 1 024 operating points (+-2 % around the example's), rate mode, infinite horizon.  Measured on the host emulation:
    none left out, K - twin = 4.82e-10, discrete pair - cont2discrete = 3.51e-13, kernel residual - scipy residual = 6.65e-15 at
    worst (median ratio 0.002).  Bounds: ten times the measured values."""
    lc.check_family_b(hostemu=True)


def test_status_bits_and_neighbours():
    lc.check_status(hostemu=True)


def test_per_member_terminal_weight_and_horizon_change():
    """finite horizon with one terminal weight per member; changing n_horizon afterwards designs with the new horizon"""
    lqr = lc.model_free_lqr(3, 1, hostemu=True, n_horizon=4)
    rng = np.random.default_rng(5)
    A, Bm = 0.7 * rng.standard_normal((5, 3, 3)), rng.standard_normal((5, 3, 1))
    Pt = np.stack([(1.0 + b) * np.eye(3) for b in range(5)])
    r = lqr.gains_batch(A, Bm, P=Pt)
    for b in range(5):
        Kt, Ptw = lc.twin_design(A[b], Bm[b], np.eye(3), np.eye(1), n_horizon=4, P=Pt[b])
        assert lc.relerr(r["K"][b], Kt) < 1e-12 and lc.relerr(r["P"][b], Ptw) < 1e-12 and r["iters"][b] == 4
    lqr.settings.n_horizon = None
    r = lqr.gains_batch(A, Bm)
    for b in range(5):
        assert lc.relerr(r["K"][b], lc.twin_design(A[b], Bm[b], np.eye(3), np.eye(1))[0]) < lc.K_BOUND_A


# ---------------------------------------------------------------------------------------------- zero-order hold: unequal designs in one wavefront
@pytest.mark.parametrize("members", [None, [4, 5, 6, 7, 8, 9, 15]], ids=["B16", "B7-slowest-last"])
def test_zero_order_hold_with_mixed_squarings_in_a_wavefront(members):
    """gains_at at 16 operating points of the CSTR (T_R 340 .. 440 K, F x 0.5 .. 8) whose exponentials need 13 13 12 12 | 12 11 11 9 |
    11 11 12 12 | 12 13 13 13 squarings; B = 7: 12 11 11 9 | 11 11 13.  Measured on the host emulation against scipy: discrete pair -
    cont2discrete = 5.97e-13 with |B_d| up to 2.1e3 (bound: ten times that, lqr_common.AB_BOUND_MIXED), K - twin = 1.30e-10 and
    residual excess 5.6e-16 (bounds of family (b)), none left out.  Bit for bit against single-member calls is trivially true here and
    is the point of the GPU twin."""
    lc.check_mixed_squarings(hostemu=True, members=members)


def test_failed_exponentials_beside_good_designs():
    """status [0 3 0 3 0 0 3], doubling steps [9 50 10 50 10 11 50] on the host emulation"""
    lc.check_failed_exponential(hostemu=True)


# ---------------------------------------------------------------------------------------------- closed loop
@pytest.mark.parametrize("name", ["oscillating_masses_lqr", "cstr_lqr"])
def test_batch_closed_loop_of_copies_is_the_single_loop(name):
    lc.check_closed_loop_copies(name, hostemu=True)


def test_batch_closed_loop_with_a_gain_schedule():
    lc.check_closed_loop_schedule(hostemu=True)


# ---------------------------------------------------------------------------------------------- compiler evidence
def _prebuilt():
    import __graft_entry__ as ge
    return ge.PREBUILT_LQR


@pytest.mark.parametrize("entry", _prebuilt(), ids=lambda e: "-".join(str(v) for v in e))
def test_prebuilt_designs_use_no_scratch(entry, tmp_path):
    """every register array of the kernel is indexed at compile time: no scratch memory and no spilled VGPR, N = 16 included"""
    import __graft_entry__ as ge
    try:
        build._hipcc()
    except build.BuildError:
        pytest.skip("hipcc not available")
    (label, hdr, h), = ge.lowered_lqr([entry])
    meta = lc.kernel_metadata(build.lqr_code_object(hdr, h), tmp_path)
    if meta is None:
        pytest.skip("llvm-readelf not found next to hipcc")
    assert meta == (0, 0), label
