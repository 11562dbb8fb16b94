"""TEST-ONLY helpers of the extended Kalman filter tests for models with algebraic states (tests/test_ekf_dae.py on the host emulation
of csrc/dompc_ekf.hip, tests/test_gpu_ekf_dae.py on the device): the models of the cases, a numpy / scipy twin of the filter on the
reduced system, and the shared checks.

NO REFERENCE FIXTURE CAN EXIST for any of this: the reference's EKF asserts n_alg == 0 ('EKF with algebraic equations not ready for
use!').  Every check here is therefore either an EQUIVALENCE (the filter of a model with algebraic states against the existing ODE
filter of the same model with z eliminated by hand) or an ORACLE comparison (against `TwinDAE`, the recursion of ekf_common.Twin -
itself checked against the reference's stored run - carried over to the reduced system z = zeta(x, u))."""
import numpy as np

import ekf_common as ec
from do_mpc_amd import sym
from do_mpc_amd.ekf import EKF
from do_mpc_amd.examples import CASES
from do_mpc_amd.model import Model, _dae_functions
from ekf_common import relerr

NAN_BITS = 0x7FF8DEADBEEF0123


# ---------------------------------------------------------------------------------------------- the twin
class TwinDAE:
    """ekf_common.Twin on the reduced system of x' = f(x, u, z), 0 = g(x, u, z), y = h(x, u, z) (x+ = f for a discrete model), built
    from the model's own sym.Functions: zeta(x, u) by Newton to 1e-14 (model._dae_functions: g and g_z), A = f_x - f_z g_z^-1 g_x and
    C = h_x - h_z g_z^-1 g_x at the PRIOR estimate (`c_at_apriori=True`: C at the a-priori state instead), continuous models by
    scipy's DOP853 on [x; P] with zeta solved inside every right-hand side."""

    def __init__(self, model, t_step=None, rtol=1e-12, atol=1e-12, c_at_apriori=False):
        m = self.m = model
        self.t_step, self.rtol, self.atol, self.c_at_apriori = t_step, rtol, atol, c_at_apriori
        zero = {s.idx: sym.ZERO for s in m._w.cat.nodes() + m._v.cat.nodes()}
        col = lambda nodes: sym.SX(list(nodes), (len(nodes), 1))      # noqa: E731
        f, h = col(sym.substitute_nodes(m._rhs.nodes(), zero)), col(sym.substitute_nodes(m._y.cat.nodes(), zero))
        ins = [m._x.cat, m._u.cat, m._z.cat, m._tvp.cat, m._p.cat]
        self._alg = _dae_functions(m)[0]
        self._lin = _dae_functions(m)[1]
        self._fh = sym.Function("fh", ins, [f, h])
        self._hjac = sym.Function("hjac", ins, [sym.jacobian(h, m._x.cat), sym.jacobian(h, m._z.cat)])

    def zeta(self, x, u, z0, tvp, p, tol=1e-14, max_iter=100):
        """-> (z with max |g| <= tol, Newton updates); an iterate that round-off keeps above tol is accepted below 1e-12 once the
        updates no longer reduce it"""
        nz = self.m.n_z
        z, n, last = np.asarray(z0, float).ravel().copy(), 0, np.inf
        while True:
            g, gz = self._alg.eval(x, u, z, tvp, p)
            g, gz = np.asarray(g, float).ravel(), np.asarray(gz, float).reshape((nz, nz), order="F")
            r = float(np.max(np.abs(g)))
            if r <= tol or (r < 1e-12 and r >= last):
                return z, n
            assert n < max_iter and np.isfinite(r), f"twin: Newton did not converge (max |g| = {r:.3e})"
            z, n, last = z - np.linalg.solve(gz, g), n + 1, r

    def reduced(self, x, u, z, tvp, p):
        m = self.m
        nx, nu, nz, ny = m.n_x, m.n_u, m.n_z, m.n_y
        fx, _, fz, gx, _, gz = (np.asarray(M, float).reshape(s, order="F") for M, s in zip(
            self._lin.eval(x, u, z, tvp, p), ((nx, nx), (nx, nu), (nx, nz), (nz, nx), (nz, nu), (nz, nz))))
        hx, hz = (np.asarray(M, float).reshape(s, order="F") for M, s in zip(self._hjac.eval(x, u, z, tvp, p), ((ny, nx), (ny, nz))))
        Zx = np.linalg.solve(gz, gx)
        return fx - fz @ Zx, hx - hz @ Zx

    def _fh_at(self, x, u, z, tvp, p):
        f, h = self._fh.eval(x, u, z, tvp, p)
        return np.asarray(f, float).ravel(), np.asarray(h, float).ravel()

    def step(self, x, P, y, u, Q, R, z0, p=(), tvp=()):
        """-> (posterior x, P, algebraic states consistent with the a-priori state)"""
        m = self.m
        nx = m.n_x
        x, P, u, p, tvp = (np.asarray(a, float) for a in (x, P, u, p, tvp))
        u, p, tvp = u.ravel(), p.ravel(), tvp.ravel()
        z, _ = self.zeta(x, u, z0, tvp, p)
        A, C = self.reduced(x, u, z, tvp, p)
        if m.model_type == "discrete":
            xa = self._fh_at(x, u, z, tvp, p)[0]
            Pa = A @ P @ A.T + Q
        else:
            from scipy.integrate import solve_ivp
            warm = [z]

            def ode(t, s):
                xs, Ps = s[:nx], s[nx:].reshape(nx, nx)
                warm[0], _ = self.zeta(xs, u, warm[0], tvp, p)
                Ax, _ = self.reduced(xs, u, warm[0], tvp, p)
                return np.concatenate([self._fh_at(xs, u, warm[0], tvp, p)[0], (Ax @ Ps + Ps @ Ax.T + Q).ravel()])
            sol = solve_ivp(ode, (0.0, float(self.t_step)), np.concatenate([x, P.ravel()]), method="DOP853", rtol=self.rtol, atol=self.atol)
            assert sol.success
            xa, Pa = sol.y[:nx, -1], sol.y[nx:, -1].reshape(nx, nx)
        za, _ = self.zeta(xa, u, z, tvp, p)
        if self.c_at_apriori:
            C = self.reduced(xa, u, za, tvp, p)[1]
        L = Pa @ C.T @ np.linalg.inv(C @ Pa @ C.T + R)
        xn = xa + L @ (np.asarray(y, float).ravel() - self._fh_at(xa, u, za, tvp, p)[1])
        return xn, (np.eye(nx) - L @ C) @ Pa, za


# ---------------------------------------------------------------------------------------------- the models of the cases
OM = CASES["oscillating_masses_dae"]


def masses_dae_model():
    """model 1: the equations of oscillating_masses_dae (x+ = z, 0 = z - A_D x - B_D u) measured at x[0], x[2] and z[1]"""
    m = Model("discrete")
    x = m.set_variable("_x", "x", (4, 1))
    u = m.set_variable("_u", "u", (1, 1))
    z = m.set_variable("_z", "x_next", (4, 1))
    m.set_meas("y1", x[0])
    m.set_meas("y2", x[2])
    m.set_meas("y3", z[1])
    m.set_rhs("x", z)
    m.set_alg("x_next", z - OM.A_D @ x - OM.B_D @ u)
    m.setup()
    return m


def masses_eliminated_model():
    """model 1 with z eliminated by hand: x+ = A_D x + B_D u, y3 = (A_D x + B_D u)[1]"""
    m = Model("discrete")
    x = m.set_variable("_x", "x", (4, 1))
    u = m.set_variable("_u", "u", (1, 1))
    xn = OM.A_D @ x + OM.B_D @ u
    m.set_meas("y1", x[0])
    m.set_meas("y2", x[2])
    m.set_meas("y3", xn[1])
    m.set_rhs("x", xn)
    m.setup()
    return m


def nonlinear_discrete_model():
    """model 2: discrete, g nonlinear in z, the measurement y = x1 z1 depends on z: C depends on where it is evaluated"""
    m = Model("discrete")
    x1, x2 = m.set_variable("_x", "x1"), m.set_variable("_x", "x2")
    u = m.set_variable("_u", "u")
    z1, z2 = m.set_variable("_z", "z1"), m.set_variable("_z", "z2")
    m.set_meas("prod", x1 * z1)
    m.set_rhs("x1", x1 + 0.3 * x2 + 0.1 * z2)
    m.set_rhs("x2", 0.9 * x2 + 0.2 * sym.sin(x1) + u + 0.1 * z1)
    m.set_alg("g1", z1 + 0.2 * z1 * z1 * z1 - x1 * x2 - 0.1 * z2)
    m.set_alg("g2", z2 + 0.1 * z2 * z2 * z2 - sym.sin(x1))
    m.setup()
    return m


def continuous_model():
    """model 3: continuous, n_x = n_z = n_y = 2; g_1 does not depend on z_1 - g_z has a structural zero in position (0, 0), so the
    elimination pivots over the lanes; y = [x1 + z1, x2 z2]"""
    m = Model("continuous")
    x1, x2 = m.set_variable("_x", "x1"), m.set_variable("_x", "x2")
    u = m.set_variable("_u", "u")
    z1, z2 = m.set_variable("_z", "z1"), m.set_variable("_z", "z2")
    m.set_meas("y1", x1 + z1)
    m.set_meas("y2", x2 * z2)
    m.set_rhs("x1", -x1 + z1 + u)
    m.set_rhs("x2", -0.5 * x2 + 0.3 * z2 * sym.sin(x1))
    m.set_alg("g1", z2 + 0.1 * z2 * z2 * z2 - x1)
    m.set_alg("g2", z1 + 0.2 * z2 + 0.1 * z1 * z1 * z1 - x2)
    m.setup()
    return m


def reactor_eliminated_model():
    """model 5 with Cc = 1 + Ad - Ca - Cb eliminated by hand"""
    ex = CASES["batch_reactor_lqr_dae"]
    m = Model("continuous")
    ca, cb, ad = m.set_variable("_x", "Ca"), m.set_variable("_x", "Cb"), m.set_variable("_x", "Ad")
    cain = m.set_variable("_u", "Cain")
    m.set_rhs("Ca", -ex.K1 * ca + cain)
    m.set_rhs("Cb", ex.K1 * ca - ex.K2 * cb + ex.K3 * (1 + ad - ca - cb))
    m.set_rhs("Ad", cain)
    m.setup()
    return m


def limit_model(nz=16, noise_in_jacobian=False):
    """discrete, n_x = n_y = 16 and n_z = `nz`: f = F x + G u + H z + 0.1 sin(x_0) e_0, g = M z + 0.05 z^3 - C x - D u (M diagonally
    dominant), y = Cy x + Dy z.  noise_in_jacobian: f_z gets the factor (1 + w_0)"""
    rng = np.random.default_rng(41)
    nx = ny = 16
    F = 0.6 * rng.standard_normal((nx, nx)) / np.sqrt(nx)
    Gm, H = rng.standard_normal((nx, 1)), 0.3 * rng.standard_normal((nx, nz)) / np.sqrt(nz)
    M = 2.0 * np.eye(nz) + 0.5 * rng.standard_normal((nz, nz)) / np.sqrt(nz)
    Cm, D = rng.standard_normal((nz, nx)) / np.sqrt(nx), rng.standard_normal((nz, 1))
    Cy, Dy = np.eye(ny, nx) + 0.1 * rng.standard_normal((ny, nx)), 0.3 * rng.standard_normal((ny, nz)) / np.sqrt(nz)
    m = Model("discrete")
    x = m.set_variable("_x", "x", (nx, 1))
    u = m.set_variable("_u", "u", (1, 1))
    z = m.set_variable("_z", "z", (nz, 1))
    m.set_meas("y", Cy @ x + Dy @ z)
    nl = sym.vertcat(0.1 * sym.sin(x[0]), np.zeros((nx - 1, 1)))
    if noise_in_jacobian:
        w = m.set_variable("_w", "w", (nx, 1))
        m.set_rhs("x", F @ x + Gm @ u + (H @ z) * (1.0 + w[0]) + nl)
    else:
        m.set_rhs("x", F @ x + Gm @ u + H @ z + nl)
    m.set_alg("g", M @ z + 0.05 * z * z * z - Cm @ x - D @ u)
    m.setup()
    return m


def status_model():
    """discrete, n_x = n_z = 2; the inputs select the algebraic equations of a member:
      g_i = u_0 (z_i^3 + z_i) + u_1 (z_i^2 + 1 + x_i^2) + u_2 z_i + u_3 sqrt((z_i + 1)^2) - (C x)_i
    u = (0, 0, 1, 0): linear in z (one update per solve); (1, 0, 0, 0): cubic; (0, 1, 0, 0): no root; (0, 0, 0, 0): g_z = 0, singular
    everywhere; (0, 0, 1, 1): g is finite at z = -1 but g_z = 1 + (z + 1) / sqrt((z + 1)^2) is 0 / 0 there - and finite everywhere else"""
    Cm = np.array([[0.8, -0.3], [0.2, 0.9]])
    m = Model("discrete")
    x = m.set_variable("_x", "x", (2, 1))
    u = m.set_variable("_u", "u", (4, 1))
    z = m.set_variable("_z", "z", (2, 1))
    m.set_meas("y1", x[0] + z[0])
    m.set_meas("y2", x[1])
    m.set_rhs("x", np.array([[0.9, 0.2], [-0.1, 0.8]]) @ x + 0.1 * z)
    m.set_alg("g", u[0] * (z * z * z + z) + u[1] * (z * z + 1 + x * x) + u[2] * z + u[3] * sym.sqrt((z + 1) * (z + 1)) - Cm @ x)
    m.setup()
    return m


# name -> (builder, t_step).  __graft_entry__.PREBUILT_EKF_DAE lists these names, so their code objects are built with the others.
MODELS = {
    "masses": (masses_dae_model, 0.5),
    "nonlinear_discrete": (nonlinear_discrete_model, 1.0),
    "continuous": (continuous_model, 0.5),
    "dip": (lambda: CASES["dip"].build_model(), 0.04),
    "batch_reactor": (lambda: CASES["batch_reactor_lqr_dae"].build_dae_model(), 0.5),
    "limit": (limit_model, 1.0),
    "status": (status_model, 1.0),
    "oscillating_masses_dae": (lambda: OM.build_model(), 0.5),
    # models 1 and 5 with z eliminated by hand: ODE models for the existing filter (the opt-in changes nothing for them)
    "masses_eliminated": (masses_eliminated_model, 0.5),
    "batch_reactor_eliminated": (reactor_eliminated_model, 0.5),
}
P_VALUES = {"dip": {"m1": 0.2, "m2": 0.2}}
TVP_VALUES = {"dip": {"pos_set": 0.8}}


def make_filter(name, hostemu=None, **settings):
    """the filter of MODELS[name] with dae_reduction on, constant parameters, abstol = reltol = 1e-10 (hostemu=None: not set up)"""
    build, t_step = MODELS[name]
    m = build()
    ekf = EKF(m)
    ekf.settings.t_step = t_step
    ekf.settings.dae_reduction = True
    for k, v in settings.items():
        setattr(ekf.settings, k, v)
    if m.n_p:
        pt = ekf.get_p_template()
        for k, v in P_VALUES[name].items():
            pt[k] = v
        ekf.set_p_fun(lambda t: pt)
    if m.n_tvp:
        tv = ekf.get_tvp_template()
        for k, v in TVP_VALUES[name].items():
            tv[k] = v
        ekf.set_tvp_fun(lambda t: tv)
    if hostemu is None:
        ekf._check_validity()                      # (p_fun / tvp_fun of a model without parameters)
        return ekf
    ec.setup_on_hostemu(ekf) if hostemu else ekf.setup()
    ekf.set_initial_guess()
    return ekf


def spd(rng, n):
    G = rng.uniform(-1, 1, (n, n))
    return 0.1 * np.eye(n) + 0.02 * G @ G.T


# ---------------------------------------------------------------------------------------------- shared checks
def check_masses_equivalence(hostemu):
    """1 (EQUIVALENCE): model 1 against the existing ODE filter on the hand-eliminated model, three steps.  g_z = I: one Newton update
    is exact up to round-off, so the bound is check_evaluation_point's 1e-12 for round-off-only comparisons; two solves per step (prior
    estimate, a-priori state), one update each"""
    ekf = make_filter("masses", hostemu)
    ode = make_filter("masses_eliminated", hostemu)
    rng = np.random.default_rng(7)
    B = 5
    X, Pc = 0.5 * rng.uniform(-1, 1, (B, 4)), np.stack([spd(rng, 4) for _ in range(B)])
    U = 0.3 * rng.uniform(-1, 1, (B, 1))
    Q, R = 1e-3 * np.eye(4), 1e-2 * np.eye(3)
    Xo, Po, Z, worst = X.copy(), Pc.copy(), np.zeros((B, 4)), 0.0
    for k in range(3):
        Y = 0.3 * rng.uniform(-1, 1, (B, 3))
        r = ekf.step_batch(X, Pc, Y, U, Q, R, Z0=Z)
        o = ode.step_batch(Xo, Po, Y, U, Q, R)
        assert np.all(r["status"] == 0) and np.all(o["status"] == 0)
        assert np.all(r["newton"] == 2), r["newton"]
        worst = max(worst, relerr(r["x"], o["x"]), relerr(r["P"], o["P"]))
        X, Pc, Z, Xo, Po = r["x"], r["P"], r["Z"], o["x"], o["P"]
    print(f"discrete elimination equivalence: filter with z - filter of the eliminated model = {worst:.3e}")
    assert worst < 1e-12


def check_evaluation_points(hostemu):
    """2 (ORACLE): A_k, C_k at the prior estimate (x0, zeta(x0, u)): the kernel equals the twin, a twin with C at the a-priori state
    differs - ekf_common.check_evaluation_point on the reduced system, with its bounds"""
    ekf = make_filter("nonlinear_discrete", hostemu, z_tol=1e-13)
    m = ekf.model
    x, P = np.array([0.7, -1.3]), np.array([[0.5, 0.1], [0.1, 0.8]])
    Q, R, u, y, z0 = 1e-2 * np.eye(2), 1e-1 * np.eye(1), np.array([0.4]), np.array([-0.2]), np.zeros(2)
    r = ekf.step_batch(x[None], P[None], y[None], u, Q, R, Z0=z0)
    xt, Pt, zt = TwinDAE(m).step(x, P, y, u, Q, R, z0)
    xw, Pw, _ = TwinDAE(m, c_at_apriori=True).step(x, P, y, u, Q, R, z0)
    e = max(relerr(r["x"][0], xt), relerr(r["P"][0], Pt), relerr(r["Z"][0], zt))
    d = max(relerr(xw, xt), relerr(Pw, Pt))
    print(f"evaluation points: kernel - twin = {e:.3e}, (C at x-) - twin = {d:.3e}, Newton updates {r['newton'][0]}")
    assert r["status"][0] == 0 and r["newton"][0] >= 2
    assert e < 1e-12                   # (Newton to 1e-13 / 1e-14 on both sides, then a dozen multiply-adds on numbers of size 1)
    assert d > 1e-3


def continuous_case(name, seed=3):
    """start values, input and five measurements: deterministic, of the size of the model's own states"""
    m = MODELS[name][0]()
    rng = np.random.default_rng(seed)
    nx, ny = m.n_x, m.n_y
    if name == "dip":
        x = np.array([0.1, 0.3, -0.2, 0.05, -0.1, 0.1]) + 0.02 * rng.uniform(-1, 1, nx)
        u = np.array([0.5])
    elif name == "batch_reactor":
        x = np.array([1.0, 0.5, 0.2]) + 0.1 * rng.uniform(-1, 1, nx)
        u = np.array([0.3])
    else:
        x = np.array([0.8, -0.5]) + 0.1 * rng.uniform(-1, 1, nx)
        u = np.array([0.4])
    P = spd(rng, nx)
    Q, R = 1e-3 * np.eye(nx), 1e-2 * np.eye(ny)
    ys = [0.3 * rng.uniform(-1, 1, ny) + (x if ny == nx else 0.0) for _ in range(5)]
    return m, x, P, u, Q, R, ys


_TWIN_RUNS = {}


def continuous_twin_runs(name):
    """five steps of the twin at rtol = atol = 1e-12 and at 1e-13 -> (trajectory at 1e-12, difference between the two runs); computed
    once per process"""
    if name not in _TWIN_RUNS:
        m, x, P, u, Q, R, ys = continuous_case(name)
        p, tvp = ec.p_tvp(make_filter(name, None))
        out = []
        for tol in (1e-12, 1e-13):
            tw = TwinDAE(m, t_step=MODELS[name][1], rtol=tol, atol=tol)
            xs, Ps, zs, traj = x.copy(), P.copy(), np.zeros(m.n_z), []
            for y in ys:
                xs, Ps, zs = tw.step(xs, Ps, y, u, Q, R, zs, p=p, tvp=tvp)
                traj.append((xs.copy(), Ps.copy(), zs.copy()))
            out.append(traj)
        diff = max(max(relerr(a[0], b[0]), relerr(a[1], b[1])) for a, b in zip(*out))
        _TWIN_RUNS[name] = (out[0], diff)
    return _TWIN_RUNS[name]


def check_continuous(name, hostemu):
    """3, 4 (ORACLE): five filter steps (abstol = reltol = 1e-10, z_tol = 1e-13: the Newton residual sits below the integrator bound)
    against TwinDAE integrated at 1e-12; bound of ekf_common.check_continuous: max(1e-9, 10 x |twin(1e-12) - twin(1e-13)|)"""
    m, x, P, u, Q, R, ys = continuous_case(name)
    ekf = make_filter(name, hostemu, z_tol=1e-13)
    ref, twin_diff = continuous_twin_runs(name)
    bound = max(1e-9, 10.0 * twin_diff)
    xs, Ps, zs, worst = x.copy(), P.copy(), np.zeros(m.n_z), 0.0
    for k, y in enumerate(ys):
        r = ekf.step_batch(xs[None], Ps[None], y[None], u, Q, R, Z0=zs)
        assert r["status"][0] == 0 and r["n_steps"][0] >= 1, r
        xs, Ps, zs = r["x"][0], r["P"][0], r["Z"][0]
        worst = max(worst, relerr(xs, ref[k][0]), relerr(Ps, ref[k][1]), relerr(zs, ref[k][2]))
    print(f"{name}: kernel - twin(1e-12) = {worst:.3e}, twin(1e-12) - twin(1e-13) = {twin_diff:.3e}, bound = {bound:.3e}, "
          f"steps of the last interval = {int(r['n_steps'][0])}, Newton updates of the last interval = {int(r['newton'][0])}")
    assert worst < bound


def check_batch_reactor_equivalence(hostemu):
    """5 (EQUIVALENCE): the batch reactor with its algebraic state against the existing continuous ODE filter on the hand-eliminated
    model (Cc = 1 + Ad - Ca - Cb), five steps, z_tol = 1e-13; bound: the project's 1e-9 for two runs of the same integrator"""
    m, x, P, u, Q, R, ys = continuous_case("batch_reactor")
    ekf = make_filter("batch_reactor", hostemu, z_tol=1e-13)
    ode = make_filter("batch_reactor_eliminated", hostemu)
    xs, Ps, zs, xo, Po, worst = x.copy(), P.copy(), np.zeros(1), x.copy(), P.copy(), 0.0
    for y in ys:
        r = ekf.step_batch(xs[None], Ps[None], y[None], u, Q, R, Z0=zs)
        o = ode.step_batch(xo[None], Po[None], y[None], u, Q, R)
        assert r["status"][0] == 0 and o["status"][0] == 0
        xs, Ps, zs, xo, Po = r["x"][0], r["P"][0], r["Z"][0], o["x"][0], o["P"][0]
        worst = max(worst, relerr(xs, xo), relerr(Ps, Po))
    print(f"batch reactor: filter with z - filter of the eliminated model = {worst:.3e}, steps {int(r['n_steps'][0])} / {int(o['n_steps'][0])}")
    assert worst < 1e-9


def raw_step_dae_batch(ekf, B, X, Pc, Y, U, Q, R, Z0, tail=2):
    """ekf_common.raw_step_batch for the entry with algebraic states: `tail` more rows than B, filled with a NaN pattern (inputs and
    outputs, Z and newton too) -> the outputs INCLUDING the tail rows"""
    import ctypes as C
    m = ekf.model
    p, tvp = ec.p_tvp(ekf)

    def padded(a, row_shape):
        out = np.full((B + tail,) + row_shape, ec.NAN_PATTERN)
        out[:B] = np.asarray(a, float).reshape((B,) + row_shape)
        return out
    Xp, Pp, Yp, Up, Zp = padded(X, (m.n_x,)), padded(Pc, (m.n_x, m.n_x)), padded(Y, (m.n_y,)), padded(U, (m.n_u,)), padded(Z0, (m.n_z,))
    Qp, Rp = np.ascontiguousarray(Q, dtype=float), np.ascontiguousarray(R, dtype=float)
    xo, Po, zo = np.full_like(Xp, ec.NAN_PATTERN), np.full_like(Pp, ec.NAN_PATTERN), np.full_like(Zp, ec.NAN_PATTERN)
    st, nw = np.full(B + tail, -7, dtype=np.int32), np.full(B + tail, -7, dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    pa, ta = np.ascontiguousarray(p if p.size else np.zeros(1)), np.ascontiguousarray(tvp if tvp.size else np.zeros(1))
    rc = ekf._lib.dompc_ekf_step_dae_batch(ekf._h, B, ptr(Xp), ptr(Pp), ptr(Yp), ptr(Up), ptr(Zp), ptr(ta), ptr(pa), ptr(Qp), ptr(Rp),
                                           2 | 4 | 8 | 16, ptr(xo), ptr(Po), ptr(zo), ptr(nw), ptr(st))
    assert rc == 0, ekf._lib.dompc_ekf_last_error(ekf._h)
    return xo, Po, zo, nw, st


def unequal_filters(B):
    """B filters of model 3 for one wavefront with unequal work: even members start near the origin with a guess 1e-8 off their
    consistent algebraic states (ONE Newton update in the first solve), odd members far out with the guess 0 (at least 6 updates, and
    other step sizes of the integration)"""
    m = continuous_model()
    rng = np.random.default_rng(23)
    tw = TwinDAE(m)
    X = np.where(np.arange(B)[:, None] % 2 == 0, 0.3, 12.0) * rng.uniform(0.5, 1.0, (B, 2)) * rng.choice([-1.0, 1.0], (B, 2))
    U = 0.3 * rng.uniform(-1, 1, (B, 1))
    Z0, first = np.zeros((B, 2)), []
    for b in range(B):
        if b % 2 == 0:
            Z0[b] = tw.zeta(X[b], U[b], np.zeros(2), np.zeros(0), np.zeros(0))[0] + 1e-8
        first.append(tw.zeta(X[b], U[b], Z0[b], np.zeros(0), np.zeros(0), tol=1e-10)[1])
    Pc = np.stack([spd(rng, 2) for _ in range(B)])
    Y = 0.3 * rng.uniform(-1, 1, (B, 2))
    return m, X, Pc, Y, U, Z0, first


def check_one_wavefront_unequal_work(ekf, B):
    """6: row b of the batch equals the single call of filter b bit for bit (x, P, Z, newton, status word) although neighbours need
    1 and at least 6 Newton updates for their first solve and take different numbers of integration steps; nothing behind row B is
    written"""
    m, X, Pc, Y, U, Z0, first = unequal_filters(B)
    assert all(n == 1 for n in first[0::2]) and all(n >= 6 for n in first[1::2]), first
    Q, R = 1e-3 * np.eye(2), 1e-2 * np.eye(2)
    xo, Po, zo, nw, st = raw_step_dae_batch(ekf, B, X, Pc, Y, U, Q, R, Z0)
    assert np.all(st[:B] & 0xFF == 0), st
    if B > 1:
        assert (st[0] >> 8) != (st[1] >> 8) and nw[0] != nw[1], (st >> 8, nw)
    bits = lambda a: np.ascontiguousarray(a[B:]).view(np.uint64)      # noqa: E731
    assert np.all(bits(xo) == NAN_BITS) and np.all(bits(Po) == NAN_BITS) and np.all(bits(zo) == NAN_BITS)
    assert np.all(st[B:] == -7) and np.all(nw[B:] == -7)
    assert np.all(np.isfinite(xo[:B])) and np.all(np.isfinite(Po[:B])) and np.all(np.isfinite(zo[:B]))
    for b in range(B):
        x1, P1, z1, n1, s1 = raw_step_dae_batch(ekf, 1, X[b:b + 1], Pc[b:b + 1], Y[b:b + 1], U[b:b + 1], Q, R, Z0[b:b + 1])
        assert np.array_equal(x1[0], xo[b]) and np.array_equal(P1[0], Po[b]) and np.array_equal(z1[0], zo[b]), (B, b)
        assert n1[0] == nw[b] and s1[0] == st[b], (B, b, n1[0], nw[b], s1[0], st[b])


def check_status_bit_2(hostemu):
    """7: one member of a wavefront cannot solve its algebraic equations - a g without a root (the default 20 updates run out), a g_z
    that is singular everywhere, a g_z that is not finite at the guess, and, with z_max_iter = 1, a cubic g that needs more than one
    update.  It reports bit 2, hands back its prior x, P and its Z0 bit for bit, without a NaN; the other three members (g linear in
    z) equal their single calls bit for bit.  make_step raises."""
    import pytest
    rng = np.random.default_rng(31)
    Q, R = 1e-3 * np.eye(2), 1e-2 * np.eye(2)
    lin = (0.0, 0.0, 1.0, 0.0)
    cases = (("no root", {}, 1, (0.0, 1.0, 0.0, 0.0), 0.5, 20), ("singular g_z", {}, 2, (0.0, 0.0, 0.0, 0.0), 0.0, 0),
             ("g_z not finite", {}, 3, (0.0, 0.0, 1.0, 1.0), -1.0, 0), ("cubic, z_max_iter = 1", {"z_max_iter": 1}, 0, (1.0, 0.0, 0.0, 0.0), 0.0, 1))
    filters = {}
    for what, settings, slot, sel, z0, updates in cases:
        key = tuple(settings.items())
        if key not in filters:
            filters[key] = make_filter("status", hostemu, **settings)
        ekf = filters[key]
        X = 2.0 * rng.uniform(0.5, 1.0, (4, 2))
        Pc, Y = np.stack([spd(rng, 2) for _ in range(4)]), 0.3 * rng.uniform(-1, 1, (4, 2))
        U = np.tile(lin, (4, 1))
        U[slot] = sel
        Z0 = np.zeros((4, 2))
        Z0[slot] = z0
        r = ekf.step_batch(X, Pc, Y, U, Q, R, Z0=Z0)
        print(f"status bit 2, member {slot} ({what}): status {r['status']}, Newton updates {r['newton']}")
        assert r["status"][slot] & 4 and not r["status"][slot] & 1 and r["newton"][slot] == updates
        assert np.array_equal(r["x"][slot], X[slot]) and np.array_equal(r["P"][slot], Pc[slot]) and np.array_equal(r["Z"][slot], Z0[slot])
        for k in ("x", "P", "Z"):
            assert np.all(np.isfinite(r[k])), k
        for b in range(4):
            if b == slot:
                continue
            one = ekf.step_batch(X[b:b + 1], Pc[b:b + 1], Y[b:b + 1], U[b:b + 1], Q, R, Z0=Z0[b:b + 1])
            assert r["status"][b] == 0 and r["newton"][b] == 2
            for k in ("x", "P", "Z", "newton", "status", "n_steps"):
                assert np.array_equal(one[k][0], r[k][b]), (what, b, k)
    ekf = filters[()]
    ekf.x0 = np.array([1.0, 1.5])
    with pytest.raises(RuntimeError, match="Newton on the algebraic equations"):
        ekf.make_step(np.zeros((2, 1)), np.zeros((4, 1)), Q, R)
    # ... during the integration (model 3, far out, from its consistent algebraic states: the first solve needs no update, a stage of
    # the first step more than the one it may take): bit 0 as well
    cont = make_filter("continuous", hostemu, z_max_iter=1, z_tol=1e-13)
    x, u = np.array([9.0, -7.0]), np.array([0.2])
    z0 = TwinDAE(cont.model).zeta(x, u, np.zeros(2), np.zeros(0), np.zeros(0))[0]
    P = spd(rng, 2)
    r = cont.step_batch(x[None], P[None], np.zeros((1, 2)), u, Q, R, Z0=z0)
    print(f"status bit 2 during the integration: status {r['status']}, Newton updates {r['newton']}, steps {r['n_steps']}")
    assert r["status"][0] == 5
    assert np.array_equal(r["x"][0], x) and np.array_equal(r["P"][0], P) and np.array_equal(r["Z"][0], z0)


def check_limit_sizes(hostemu):
    """8 (ORACLE): the discrete n_x = n_z = n_y = 16 filter against TwinDAE, 1e-9 (cond(S) < 100 as in the large-batch test of the ODE
    filter, Newton to 1e-10 on a g_z with condition number < 10)"""
    ekf = make_filter("limit", hostemu)
    m = ekf.model
    rng = np.random.default_rng(43)
    B = 3
    X, U = 0.5 * rng.uniform(-1, 1, (B, 16)), 0.3 * rng.uniform(-1, 1, (B, 1))
    Pc, Y = np.stack([spd(rng, 16) for _ in range(B)]), 0.3 * rng.uniform(-1, 1, (B, 16))
    Q, R = 1e-3 * np.eye(16), 1e-2 * np.eye(16)
    r = ekf.step_batch(X, Pc, Y, U, Q, R)
    assert np.all(r["status"] == 0), r["status"]
    tw, worst = TwinDAE(m), 0.0
    for b in range(B):
        xt, Pt, zt = tw.step(X[b], Pc[b], Y[b], U[b], Q, R, np.zeros(16))
        worst = max(worst, relerr(r["x"][b], xt), relerr(r["P"][b], Pt), relerr(r["Z"][b], zt))
    print(f"n_x = n_z = n_y = 16: kernel - twin = {worst:.3e}, Newton updates {r['newton']}")
    assert worst < 1e-9


def check_make_step(hostemu):
    """9: make_step on model 1 carries z0 from step to step, records `_z`, and ten steps equal the batch path bit for bit"""
    ekf = make_filter("masses", hostemu)
    bat = make_filter("masses", hostemu)
    rng = np.random.default_rng(13)
    x0, P0 = 0.5 * rng.uniform(-1, 1, 4), spd(rng, 4)
    Q, R = 1e-3 * np.eye(4), 1e-2 * np.eye(3)
    ekf.x0, ekf.P0 = x0, P0.copy()
    assert np.array_equal(ekf.z0.master, np.zeros(4))
    x, P, z = x0[None].copy(), P0[None].copy(), np.zeros((1, 4))
    for k in range(10):
        y, u = 0.3 * rng.uniform(-1, 1, (3, 1)), 0.3 * rng.uniform(-1, 1, (1, 1))
        got = ekf.make_step(y, u, Q, R)
        r = bat.step_batch(x, P, y.T, u.T, Q, R, Z0=z)
        x, P, z = r["x"], r["P"], r["Z"]
        assert got.shape == (4, 1) and np.array_equal(got.ravel(), x[0]) and np.array_equal(ekf.P0, P[0])
        assert np.array_equal(ekf.z0.master, z[0]) and np.any(z[0] != 0.0)
    assert ekf.data["_z"].shape == (10, 4) and np.array_equal(ekf.data["_z"][-1], z[0]) and ekf.data["_x"].shape == (10, 4)
