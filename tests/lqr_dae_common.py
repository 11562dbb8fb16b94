"""TEST-ONLY helpers of the LQR tests for models with algebraic states (tests/test_lqr_dae.py on the host emulation of
csrc/dompc_lqr.hip, tests/test_gpu_lqr_dae.py on the device): the numpy twin of the index-1 reduction inside the design kernel
(Newton and the reduction with np.linalg.solve, then lqr_common.twin_zoh / twin_design), the DAE models of the cases and the shared
checks.  Comparison rule and bounds are those of lqr_common.check_family_b (K_BOUND_B, AB_BOUND_B, RES_MARGIN_B, SCIPY_RESIDUAL)."""
import os

import numpy as np

import lqr_common as lc
from do_mpc_amd import sym
from do_mpc_amd.examples import CASES
from do_mpc_amd.model import Model, _dae_functions
from lqr_common import relerr

Z_TOL, Z_MAX_ITER = 1e-10, 40
T_STEP = 0.5


# ---------------------------------------------------------------------------------------------- the twin
def twin_reduce(model, x, u, z0, tol=Z_TOL, max_iter=Z_MAX_ITER, explicit_inverse=False):
    """-> (A, B, z, Newton updates, ok) of the reduced system at (x, u): Newton on g = 0 from z0, g_z [Z_x Z_u] = [g_x g_u],
    A = f_x - f_z Z_x, B = f_u - f_z Z_u (undiscretised)"""
    f_alg, f_lin = _dae_functions(model)
    nx, nu, nz = model.n_x, model.n_u, model.n_z
    solve = (lambda M, r: np.linalg.inv(M) @ r) if explicit_inverse else np.linalg.solve
    args = [np.asarray(x, float).ravel(), np.asarray(u, float).ravel(), np.asarray(z0, float).ravel().copy(), np.zeros(0), np.zeros(0)]
    passes, ok = 0, True
    while True:
        g, gz = f_alg.eval(*args)
        gz = gz.reshape((nz, nz), order="F")
        if np.max(np.abs(g)) <= tol:
            break
        if passes >= max_iter or not np.all(np.isfinite(gz)) or np.linalg.matrix_rank(gz) < nz:
            ok = False
            break
        args[2] = args[2] - solve(gz, g)
        passes += 1
    fx, fu, fz, gx, gu, gz = (M.reshape(s, order="F") for M, s in zip(f_lin.eval(*args), ((nx, nx), (nx, nu), (nx, nz), (nz, nx), (nz, nu), (nz, nz))))
    if not ok or np.linalg.matrix_rank(gz) < nz:
        return np.zeros((nx, nx)), np.zeros((nx, nu)), args[2], passes, False
    Z = solve(gz, np.hstack([gx, gu]))
    return fx - fz @ Z[:, :nx], fu - fz @ Z[:, nx:], args[2], passes, True


# ---------------------------------------------------------------------------------------------- the models of the cases
def _conditioned(rng, n, cond=1e3, zero00=False):
    """random n x n matrix with condition number <= cond (singular values drawn in [1, cond^(1/2)] / ...); zero00: entry (0, 0) is a
    structural zero (a permutation of a matrix whose first column starts with it)"""
    while True:
        U, _ = np.linalg.qr(rng.standard_normal((n, n)))
        V, _ = np.linalg.qr(rng.standard_normal((n, n)))
        M = U @ np.diag(10.0 ** rng.uniform(-1.0, 1.0, n)) @ V.T
        if zero00:
            M[0, 0] = 0.0
        if np.linalg.cond(M) <= cond:
            return M


def linear_g_model(seed, nx, nu, nz, discrete, zero00=False, stable=0.6, shift=0.0):
    """f = F x + G u + H z + 0.1 sin(x_0) e_0, g = M z - C x - D u (linear in z: one Newton pass); M with condition number <= 1e3.
    shift: F - shift I, a damped system (the Riccati solution of a large design stays well conditioned: scipy's own residual left two
    of five undamped systems of 15 states out)"""
    rng = np.random.default_rng(seed)
    F = stable * rng.standard_normal((nx, nx)) / np.sqrt(nx) - shift * np.eye(nx)
    Gm, H = rng.standard_normal((nx, nu)), 0.3 * rng.standard_normal((nx, nz)) / np.sqrt(nz)
    M, Cm, D = _conditioned(rng, nz, zero00=zero00), rng.standard_normal((nz, nx)) / np.sqrt(nx), rng.standard_normal((nz, nu))
    mdl = Model("discrete" if discrete else "continuous")
    x = mdl.set_variable("_x", "x", (nx, 1))
    u = mdl.set_variable("_u", "u", (nu, 1))
    z = mdl.set_variable("_z", "z", (nz, 1))
    nl = sym.vertcat(0.1 * sym.sin(x[0]), np.zeros((nx - 1, 1))) if nx > 1 else 0.1 * sym.sin(x[0])
    mdl.set_rhs("x", F @ x + Gm @ u + H @ z + nl)
    mdl.set_alg("g", M @ z - Cm @ x - D @ u)
    mdl.setup()
    return mdl


def cubic_g_model(seed=11, nx=4, nu=2, nz=2, singular_when_u0_zero=False):
    """continuous; g_i = z_i^3 + z_i - (C x)_i: Newton from z = 0 needs the more passes the larger |C x|.  singular_when_u0_zero:
    g_i = u_0 (z_i^3 + z_i) - (C x)_i instead, whose g_z = u_0 (3 z^2 + 1) is singular at EVERY iterate of a design with u_0 = 0"""
    rng = np.random.default_rng(seed)
    F = 0.6 * rng.standard_normal((nx, nx)) / np.sqrt(nx)
    Gm, H, Cm = rng.standard_normal((nx, nu)), 0.3 * rng.standard_normal((nx, nz)), rng.standard_normal((nz, nx)) / np.sqrt(nx)
    mdl = Model("continuous")
    x = mdl.set_variable("_x", "x", (nx, 1))
    u = mdl.set_variable("_u", "u", (nu, 1))
    z = mdl.set_variable("_z", "z", (nz, 1))
    mdl.set_rhs("x", F @ x + Gm @ u + H @ z)
    cub = z * z * z + z
    mdl.set_alg("g", (u[0] * cub if singular_when_u0_zero else cub) - Cm @ x)
    mdl.setup()
    return mdl


# the designs of the cases: name -> (model, inputRatePenalization mode).  __graft_entry__.PREBUILT_LQR lists them as ("dae", name, mode),
# so their code objects are built with the others.
DESIGNS = {
    "batch_reactor": (lambda: CASES["batch_reactor_lqr_dae"].build_dae_model(), False),
    "pivoting": (lambda: linear_g_model(21, 2, 1, 3, discrete=True, zero00=True), False),
    "newton": (lambda: cubic_g_model(), False),
    "nz16": (lambda: linear_g_model(31, 2, 1, 16, discrete=False), False),
    "nx15_rate": (lambda: linear_g_model(32, 15, 1, 1, discrete=False, shift=1.0), True),
    "oscillating_masses_dae": (lambda: CASES["oscillating_masses_dae"].build_model(), False),
    "status": (lambda: cubic_g_model(seed=12, singular_when_u0_zero=True), False),
}


def controller(model, hostemu, rate=False, setup=False):
    """controller of the model's size on a placeholder LinearModel, unit weights (delR = I in rate mode): gains_at takes the model
    itself and needs no gain of the placeholder, so setup() - one more design - is made only where a closed loop asks for it"""
    import warnings
    from do_mpc_amd.lqr import LQR
    from do_mpc_amd.model import LinearModel
    nx, nu = model.n_x, model.n_u
    m = LinearModel("discrete")
    m.set_variable("_x", "x", (nx, 1))
    m.set_variable("_u", "u", (nu, 1))
    m.setup(0.5 * np.eye(nx), np.eye(nx, nu))
    lqr = LQR(m)
    lqr.set_param(t_step=T_STEP, z_tol=Z_TOL, z_max_iter=Z_MAX_ITER)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        lqr.set_objective(Q=np.eye(nx), R=np.eye(nu))
    if rate:
        lqr.set_rterm(delR=np.eye(nu))
    if setup:
        lc.setup_lqr(lqr, hostemu)
    elif hostemu:
        lqr._emu = lc.lqr_hostemu_library
    return lqr


def design(name, hostemu, **kw):
    build, rate = DESIGNS[name]
    model = build()
    return model, controller(model, hostemu, rate=rate, **kw)


def points(model, B, seed=3, scale=1.0):
    rng = np.random.default_rng(seed)
    return scale * rng.uniform(-1, 1, (B, model.n_x)), scale * rng.uniform(-1, 1, (B, model.n_u))


# ---------------------------------------------------------------------------------------------- shared checks
def compare_with_twin(model, lqr, r, X, U, Z0, rate=False, what=""):
    """every design of `r` (a gains_at result) against the twin with the rule and the bounds of lqr_common.check_family_b; also the
    twin against itself with an explicit inverse instead of solve (the conditioning is carried by the inputs, not by the bound)"""
    nx, nu = model.n_x, model.n_u
    Q, R, dR = np.eye(nx), np.eye(nu), np.eye(nu)
    Qt = np.block([[Q, np.zeros((nx, nu))], [np.zeros((nu, nx)), R]]) if rate else Q
    Rt = dR if rate else R
    cont = model.model_type == "continuous"
    left, wk, wab, wz, wex, wself = 0, 0.0, 0.0, 0.0, 0.0, 0.0
    assert np.all(r["status"] == 0), r["status"]
    for b in range(len(X)):
        Ac, Bc, z, passes, ok = twin_reduce(model, X[b], U[b], Z0[b])
        Ai, Bi, zi, _, _ = twin_reduce(model, X[b], U[b], Z0[b], explicit_inverse=True)
        assert ok
        Ad, Bd = lc.twin_zoh(Ac, Bc, T_STEP) if cont else (Ac, Bc)
        Adi, Bdi = lc.twin_zoh(Ai, Bi, T_STEP) if cont else (Ai, Bi)
        wself = max(wself, relerr(Adi, Ad), relerr(Bdi, Bd), relerr(zi, z))
        wab = max(wab, relerr(r["A"][b], Ad), relerr(r["B"][b], Bd))
        if "Z" in r:
            wz = max(wz, relerr(r["Z"][b], z))
        assert r["newton"][b] == passes, (b, r["newton"][b], passes)
        Kt, Pt = lc.twin_design(Ad, Bd, Q, R, rate=rate, delR=dR)
        At, Bt = lc.design_pair(Ad, Bd, rate)
        rs = lc.riccati_residual(At, Bt, Qt, Rt, Pt)
        if not rs <= lc.SCIPY_RESIDUAL:
            left += 1
            continue
        wk = max(wk, relerr(r["K"][b], Kt))
        wex = max(wex, lc.riccati_residual(At, Bt, Qt, Rt, r["P"][b]) - rs)
    print(f"{what}: {len(X)} designs, {left} left out, K - twin = {wk:.3e} (bound {lc.K_BOUND_B:.1e}), pair - twin = {wab:.3e}, Z - twin = "
          f"{wz:.3e} (bound {lc.AB_BOUND_B:.1e}), residual kernel - scipy = {wex:.3e} (margin {lc.RES_MARGIN_B:.1e}), twin solve - twin inverse = "
          f"{wself:.3e}, Newton updates {r['newton']}")
    assert left <= max(1, lc.LEFT_OUT * len(X))
    assert wself < lc.AB_BOUND_B
    assert wk < lc.K_BOUND_B and wab < lc.AB_BOUND_B and wz < lc.AB_BOUND_B and wex <= lc.RES_MARGIN_B


def check_batch_reactor(hostemu):
    """(a) n_x = 3, n_u = 1, n_z = 1, linear g, continuous: one Newton pass from Z0 = 0"""
    model, lqr = design("batch_reactor", hostemu)
    X, U = points(model, 5, scale=2.0)
    r = lqr.gains_at(model, X, U)
    assert np.all(r["newton"] == 1)
    assert relerr(r["Z"][:, 0], 1 + X[:, 2] - X[:, 0] - X[:, 1]) < 1e-14
    compare_with_twin(model, lqr, r, X, U, np.zeros((5, 1)), what="(a) batch reactor")


def check_pivoting(hostemu):
    """(b) n_x = 2, n_u = 1, n_z = 3, discrete, g_z with a zero in position (0, 0): the elimination pivots off the diagonal"""
    model, lqr = design("pivoting", hostemu)
    gz = _dae_functions(model)[0].eval(np.zeros(2), np.zeros(1), np.zeros(3), np.zeros(0), np.zeros(0))[1].reshape((3, 3), order="F")
    assert gz[0, 0] == 0.0 and np.linalg.cond(gz) <= 1e3
    X, U = points(model, 5)
    Z0 = np.zeros((5, 3))
    r = lqr.gains_at(model, X, U, Z0=Z0)
    compare_with_twin(model, lqr, r, X, U, Z0, what="(b) pivoting over the lanes")
    return model, lqr, X, U, r


def newton_points():
    rng = np.random.default_rng(5)
    scale = np.array([1e-3, 1e2, 1.0, 10.0, 0.1, 30.0, 3.0])          # spread: the members of the first wavefront differ in their passes
    X = scale[:, None] * rng.uniform(0.5, 1.0, (7, 4)) * rng.choice([-1.0, 1.0], (7, 4))
    U = rng.uniform(-1, 1, (7, 2))
    return X, U


def check_newton_in_one_wavefront(hostemu):
    """(c) n_x = 4, n_u = 2, n_z = 2, continuous, cubic g, B = 7: different pass counts inside a wavefront, every member bit for bit
    its single-design result"""
    model, lqr = design("newton", hostemu)
    X, U = newton_points()
    Z0 = np.zeros((7, 2))
    r = lqr.gains_at(model, X, U, Z0=Z0)
    assert len(set(r["newton"][:4].tolist())) > 1 and len(set(r["newton"][4:].tolist())) > 1, r["newton"]
    for b in range(7):
        one = lqr.gains_at(model, X[b:b + 1], U[b:b + 1], Z0=Z0[b:b + 1])
        for k in ("K", "P", "A", "B", "Z", "newton", "status", "iters"):
            assert np.array_equal(one[k][0], r[k][b]), (b, k)
    compare_with_twin(model, lqr, r, X, U, Z0, what="(c) Newton inside one wavefront")


def check_size_limits(hostemu, name):
    """(d) n_z = 16 with n_x = 2, n_u = 1 ("nz16"), and n_x = 15, n_u = 1, n_z = 1 in rate mode (N = 16), the largest reduced design
    ("nx15_rate")"""
    for rate, what in {"nz16": [(False, "(d) n_z = 16")], "nx15_rate": [(True, "(d) n_x = 15, rate mode")]}[name]:
        model, lqr = design(name, hostemu)
        assert lqr.n_design == (16 if rate else 2)
        X, U = points(model, 5)
        Z0 = np.zeros((5, model.n_z))
        r = lqr.gains_at(model, X, U, Z0=Z0)
        compare_with_twin(model, lqr, r, X, U, Z0, rate=rate, what=what)


def check_batch_sizes_and_z_out(hostemu):
    """(e) B = 1 and B = 5, with and without z_out: the same designs"""
    model, lqr = design("pivoting", hostemu)
    X, U = points(model, 5)
    five = lqr.gains_at(model, X, U)
    without = lqr.gains_at(model, X, U, z_out=False)
    assert "Z" in five and "Z" not in without
    one = lqr.gains_at(model, X[:1], U[:1])
    for k in ("K", "P", "A", "B", "status", "newton"):
        assert np.array_equal(five[k], without[k]) and np.array_equal(one[k][0], five[k][0]), k
    assert np.array_equal(one["Z"][0], five["Z"][0])


def check_oscillating_masses_dae(hostemu):
    """(f) the discrete oscillating_masses_dae example model (x+ = z, 0 = z - A x - B u): the reduced pair is (A_D, B_D)"""
    ex = CASES["oscillating_masses_dae"]
    model, lqr = design("oscillating_masses_dae", hostemu)
    X, U = points(model, 5)
    Z0 = np.zeros((5, 4))
    r = lqr.gains_at(model, X, U, Z0=Z0)
    assert relerr(r["A"], np.tile(ex.A_D, (5, 1, 1))) < 1e-15 and relerr(r["B"], np.tile(ex.B_D, (5, 1, 1))) < 1e-15
    compare_with_twin(model, lqr, r, X, U, Z0, what="(f) oscillating_masses_dae")


def check_status(hostemu):
    """B = 6 designs on the cubic g with z_max_iter = 1: design 1 has a g_z that is singular at every iterate (u_0 = 0), design 4
    starts at Z0 = 0, where one update is not enough; both report bit 2 with K = 0, P = Q.  The four others start at their
    consistent algebraic states and equal their single-design results bit for bit."""
    model, lqr = design("status", hostemu)
    lqr.set_param(z_max_iter=1)
    rng = np.random.default_rng(9)
    X = 3.0 * rng.uniform(0.5, 1.0, (6, 4))
    U = rng.uniform(0.5, 1.0, (6, 2))
    U[1, 0] = 0.0
    good = [0, 2, 3, 5]
    Z0 = np.zeros((6, 2))
    for b in good:
        Z0[b] = twin_reduce(model, X[b], U[b], np.zeros(2), tol=1e-14)[2]
    r = lqr.gains_at(model, X, U, Z0=Z0)
    print("status:", r["status"], "Newton updates:", r["newton"], "iterations:", r["iters"])
    assert r["status"][1] & 4 and r["status"][4] & 4 and r["newton"][4] == 1 and r["newton"][1] == 0
    for k in ("K", "P", "A", "B", "Z"):
        assert np.all(np.isfinite(r[k])), k
    for b in (1, 4):
        assert np.array_equal(r["K"][b], np.zeros((2, 4))) and np.array_equal(r["P"][b], np.eye(4))
    assert np.all(r["status"][good] == 0) and np.all(r["newton"][good] == 0), (r["status"], r["newton"])
    for b in good:
        one = lqr.gains_at(model, X[b:b + 1], U[b:b + 1], Z0=Z0[b:b + 1])
        for k in ("K", "P", "A", "B", "Z", "status", "newton"):
            assert np.array_equal(one[k][0], r[k][b]), (b, k)
        Ac, Bc, z, passes, ok = twin_reduce(model, X[b], U[b], Z0[b], max_iter=1)
        assert ok and passes == 0
        Ad, Bd = lc.twin_zoh(Ac, Bc, T_STEP)
        assert relerr(r["A"][b], Ad) < lc.AB_BOUND_B and relerr(r["K"][b], lc.twin_design(Ad, Bd, np.eye(4), np.eye(2))[0]) < lc.K_BOUND_B


def check_linearize_dae(hostemu):
    """linearize_dae = the kernel's undiscretised pair and Z: the discrete case (b) read directly, the continuous case (a) through
    the zero-order hold of the twin; the three-argument linearize still refuses the model"""
    import pytest
    from do_mpc_amd.model import LinearModel, linearize, linearize_dae
    model, lqr, X, U, r = check_pivoting(hostemu)
    for b in range(len(X)):
        lin = linearize_dae(model, X[b], U[b], tol=Z_TOL, max_iter=Z_MAX_ITER)
        assert isinstance(lin, LinearModel) and lin.model_type == "discrete" and (lin.n_x, lin.n_u, lin.n_z) == (2, 1, 0)
        assert relerr(r["A"][b], lin.sys_A) < lc.AB_BOUND_B and relerr(r["B"][b], lin.sys_B) < lc.AB_BOUND_B
        assert relerr(r["Z"][b], lin.zss.ravel()) < lc.AB_BOUND_B and lin.newton_passes == r["newton"][b]
    reactor, lq = design("batch_reactor", hostemu)
    Xr, Ur = points(reactor, 3, scale=2.0)
    rr = lq.gains_at(reactor, Xr, Ur)
    for b in range(3):
        lin = linearize_dae(reactor, Xr[b].reshape(-1, 1), Ur[b].reshape(-1, 1))
        Ad, Bd = lc.twin_zoh(lin.sys_A, lin.sys_B, T_STEP)
        assert relerr(rr["A"][b], Ad) < lc.AB_BOUND_B and relerr(rr["B"][b], Bd) < lc.AB_BOUND_B
        assert relerr(rr["Z"][b], lin.zss.ravel()) < lc.AB_BOUND_B and lin._x.names == reactor._x.names
    with pytest.raises(AssertionError, match="Linearization around steady state is not supported for DAEs"):
        linearize(reactor, Xr[0].reshape(-1, 1), Ur[0].reshape(-1, 1))


# ---------------------------------------------------------------------------------------------- the stored run
def replay(hostemu):
    """the closed loop of the reference's main.py: LQR on the discretised converted model, the simulator on the continuous linear
    model -> (largest ABSOLUTE difference of simulator._x, ._u, ._time against the stored run, shape of ._z, stored shape of ._z)"""
    ex = CASES["batch_reactor_lqr_dae"]
    linear = ex.build_model()
    lqr = lc.setup_lqr(ex.build_lqr(linear, setup=False), hostemu)
    sim = lc.plant_on(ex.build_simulator(linear, setup=False), hostemu)
    x0 = ex.X0.reshape(-1, 1)
    sim.x0 = x0
    lqr.set_setpoint(xss=ex.XSS, uss=lqr.model.get_steady_state(xss=ex.XSS))
    for _ in range(ex.N_STEPS):
        x0 = sim.make_step(lqr.make_step(x0))
    g = np.load(os.path.join(lc.GOLDEN, "batch_reactor_lqr_dae.npz"))
    d = [float(np.max(np.abs(sim.data[k] - g["simulator." + k]))) for k in ("_x", "_u", "_time")]
    print(f"batch_reactor_lqr_dae: {ex.N_STEPS} steps, max |difference| _x = {d[0]:.3e}, _u = {d[1]:.3e}, _time = {d[2]:.3e}")
    return d, sim.data["_z"].shape, g["simulator._z"].shape


# ---------------------------------------------------------------------------------------------- closed loop on the DAE plant
def steady_states(B=6):
    """B steady states of the batch reactor: with Ca = 0 and Cain = 0 the state is at rest where Cb = Cc, i.e. Cb = (1 + Ad) / 2"""
    ad = np.linspace(1.0, 3.5, B)
    X = np.stack([np.zeros(B), (1 + ad) / 2, ad], axis=1)
    return X, np.zeros((B, 1))


def check_closed_loop(hostemu, B=6, n=20):
    """BatchClosedLoopLQR on the continuous batch-reactor DAE plant with per-loop gains of gains_at at B steady states: every loop ends
    nearer to its set-point than it started, and the batch equals B single loops"""
    from do_mpc_amd.closed_loop import BatchClosedLoopLQR
    from do_mpc_amd.simulator import Simulator
    model, lqr = design("batch_reactor", hostemu, setup=True)
    XSS, USS = steady_states(B)
    g = lqr.gains_at(model, XSS, USS)
    assert np.all(g["status"] == 0) and relerr(g["Z"][:, 0], XSS[:, 1]) < 1e-14          # (at rest Cc = Cb)
    sim = Simulator(model)
    sim.set_param(t_step=T_STEP)
    lc.plant_on(sim, hostemu)
    X0 = XSS + 0.2 * np.random.default_rng(4).uniform(-1, 1, XSS.shape)
    dev = "cpu" if hostemu else 0
    rec = BatchClosedLoopLQR(lqr, sim, X0, K=g["K"], XSS=XSS, USS=USS, device=dev).run(n)
    assert np.all(rec["plant_status"] == 0)
    d0, dn = np.linalg.norm(rec["x"][0] - XSS, axis=1), np.linalg.norm(rec["x"][n] - XSS, axis=1)
    print(f"closed loop on the DAE plant: distance to the set-point at step 0 {d0}, after {n} steps {dn}")
    assert np.all(dn < d0)
    worst = 0.0
    for b in range(B):
        one = BatchClosedLoopLQR(lqr, sim, X0[b:b + 1], K=g["K"][b:b + 1], XSS=XSS[b:b + 1], USS=USS[b:b + 1], device=dev).run(n)
        worst = max(worst, relerr(one["x"][:, 0], rec["x"][:, b]), relerr(one["u"][:, 0], rec["u"][:, b]))
    print(f"batch of {B} - single loops = {worst:.3e}")
    assert worst < 1e-12
