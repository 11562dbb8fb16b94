"""TEST-ONLY helpers of the extended Kalman filter tests: setup on the host emulation (hostemu_build.ekf_hostemu_library:
csrc/dompc_ekf.hip compiled by g++ with -DDOMPC_HOST_EMU, the text that ships) and a numpy / scipy twin of the reference's recursion
on the model's own sym.Functions."""
import os

import numpy as np

from do_mpc_amd import sym
from hostemu_build import OUT, ekf_hostemu_library  # noqa: F401  (callers name both through this module)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def setup_on_hostemu(ekf):
    """ekf.setup() on the host-emulated kernel"""
    hdr = ekf._lower()
    h = hdr.rsplit('EKF_MODEL_HASH "', 1)[1].split('"')[0]
    ekf.setup(_lib_path=ekf_hostemu_library(hdr, h), _code_object="")
    return ekf


class Twin:
    """The reference's filter recursion (/root/reference/do_mpc/estimator/_ekf.py:281-311) in numpy on the model's own functions:
    A = d rhs / d x and C = d y / d x by sym.jacobian, evaluated at the PRIOR estimate (`c_at_apriori=True`: C at the a-priori state
    instead - the variant the evaluation-point test must tell apart); discrete models x- = rhs(x0), P- = A P A' + Q; continuous
    models scipy.integrate.solve_ivp (DOP853) on [x; P] with dP/dt = A(x) P + P A(x)' + Q."""

    def __init__(self, model, t_step=None, rtol=1e-12, atol=1e-12, c_at_apriori=False):
        m = self.m = model
        self.t_step, self.rtol, self.atol, self.c_at_apriori = t_step, rtol, atol, c_at_apriori
        ins = [m._x.cat, m._u.cat, m._tvp.cat, m._p.cat, m._w.cat, m._v.cat]
        self._A = sym.Function("A", ins, [sym.jacobian(m._rhs, m._x.cat)])
        self._C = sym.Function("C", ins, [sym.jacobian(m._y.cat, m._x.cat)])
        self._f = sym.Function("f", ins, [m._rhs])
        self._h = sym.Function("h", ins, [m._y.cat])

    def _ev(self, fn, x, u, tvp, p, shape=None):
        m = self.m
        r = np.asarray(fn.eval(x, u, tvp, p, np.zeros(m.n_w), np.zeros(m.n_v))[0], float)
        return r.reshape(shape, order="F") if shape else r.ravel()

    def step(self, x, P, y, u, Q, R, p=(), tvp=()):
        m = self.m
        nx, ny = m.n_x, m.n_y
        x, P, u, p, tvp = (np.asarray(a, float) for a in (x, P, u, p, tvp))
        u, p, tvp = u.ravel(), p.ravel(), tvp.ravel()
        A = self._ev(self._A, x, u, tvp, p, (nx, nx))
        C = self._ev(self._C, x, u, tvp, p, (ny, nx))
        if m.model_type == "discrete":
            xa = self._ev(self._f, x, u, tvp, p)
            Pa = A @ P @ A.T + Q
        else:
            from scipy.integrate import solve_ivp

            def ode(t, s):
                xs, Ps = s[:nx], s[nx:].reshape(nx, nx)
                Ax = self._ev(self._A, xs, u, tvp, p, (nx, nx))
                return np.concatenate([self._ev(self._f, xs, u, tvp, p), (Ax @ Ps + Ps @ Ax.T + Q).ravel()])
            sol = solve_ivp(ode, (0.0, float(self.t_step)), np.concatenate([x, P.ravel()]), method="DOP853", rtol=self.rtol, atol=self.atol)
            assert sol.success
            xa, Pa = sol.y[:nx, -1], sol.y[nx:, -1].reshape(nx, nx)
        if self.c_at_apriori:
            C = self._ev(self._C, xa, u, tvp, p, (ny, nx))
        L = Pa @ C.T @ np.linalg.inv(C @ Pa @ C.T + R)
        xn = xa + L @ (np.asarray(y, float).ravel() - self._ev(self._h, xa, u, tvp, p))
        Pn = (np.eye(nx) - L @ C) @ Pa
        return xn, Pn


def relerr(a, b):
    """largest difference relative to max(1, |b|): the measure of simulator_common.check_against_scipy"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


# ---------------------------------------------------------------------------------------------- shared cases (CPU: host emulation, GPU: HIP)
import ctypes as C  # noqa: E402

from do_mpc_amd.ekf import EKF  # noqa: E402
from do_mpc_amd.examples import CASES  # noqa: E402
from do_mpc_amd.model import Model  # noqa: E402

Q_TT, R_TT = 1e-3 * np.eye(3), 1e-2 * np.eye(1)           # examples/triple_tank_ekf/main.py:160-163
T_STEP = {"rotating_masses": 0.1, "CSTR": 0.005, "oscillating_masses": 0.5, "triple_tank": 1.0}
P_VALUES = {"rotating_masses": {"P_p": 1.0, "Theta_1": 2.25e-4, "Theta_2": 2.25e-4, "Theta_3": 2.25e-4}, "CSTR": {"alpha": 1.0, "beta": 1.0},
            "triple_tank": {"p1": 2.0}, "oscillating_masses": {}}
MODEL_KW = {"oscillating_masses": {"estimation": True}}


def make_ekf(name, hostemu, model=None, **settings):
    """filter of a shipped example with constant parameters, abstol = reltol = 1e-10"""
    m = model or CASES[name].build_model(**MODEL_KW.get(name, {}))
    ekf = EKF(m)
    ekf.settings.t_step = T_STEP[name]
    for k, v in settings.items():
        setattr(ekf.settings, k, v)
    if m.n_p:
        pt = ekf.get_p_template()
        for k, v in P_VALUES[name].items():
            pt[k] = v
        ekf.set_p_fun(lambda t: pt)
    if m.n_tvp:
        tv = ekf.get_tvp_template()
        if name == "triple_tank":
            tv["tvp1"] = 0.5
        ekf.set_tvp_fun(lambda t: tv)
    if hostemu:
        setup_on_hostemu(ekf)
    else:
        ekf.setup()
    ekf.set_initial_guess()
    return ekf


def p_tvp(ekf):
    return ekf.p_fun(0.0).master.copy(), ekf.tvp_fun(0.0).master.copy()


def check_golden_triple_tank(ekf):
    """200 steps of examples/triple_tank_ekf/main.py with the measurements of the stored run: `_x` within the reference test's own
    1e-8 (testing/test_triple_tank_EKF.py:141), the other records equal"""
    g = np.load(os.path.join(GOLDEN, "triple_tank.npz"))
    ekf.x0 = np.array([1.2, 1.4, 1.8]).reshape(-1, 1)
    ekf.set_initial_guess()
    u0 = np.array([0.0001, 0.0001]).reshape(-1, 1)
    for k in range(200):
        x = ekf.make_step(y_next=g["simulator._y"][k].reshape(-1, 1), u_next=u0, Q_k=Q_TT, R_k=R_TT)
        assert x.shape == (3, 1)
    err = float(np.max(np.abs(ekf.data["_x"] - g["estimator._x"])))
    print(f"triple tank, 200 steps: max |x - golden| = {err:.3e}")
    assert ekf.data["_x"].shape == g["estimator._x"].shape
    assert err < 1e-8
    for k in ("_u", "_p", "_tvp", "_time"):
        assert np.array_equal(ekf.data[k], g["estimator." + k]), k


def nonlinear_meas_model():
    """discrete model with the nonlinear measurement y = x1 * x2: C = [x2, x1] depends on where it is evaluated"""
    from do_mpc_amd.sym import sin
    m = Model("discrete")
    x1, x2 = m.set_variable("_x", "x1"), m.set_variable("_x", "x2")
    u = m.set_variable("_u", "u")
    m.set_meas("prod", x1 * x2)
    m.set_rhs("x1", x1 + 0.3 * x2)
    m.set_rhs("x2", 0.9 * x2 + 0.2 * sin(x1) + u)
    m.setup()
    return m


def check_evaluation_point(hostemu):
    """C_k is evaluated at the PRIOR estimate (_ekf.py:284): the kernel equals the twin, a twin with C at the a-priori state differs"""
    m = nonlinear_meas_model()
    ekf = EKF(m)
    ekf.settings.t_step = 1.0
    setup_on_hostemu(ekf) if hostemu else ekf.setup()
    x, P = np.array([0.7, -1.3]), np.array([[0.5, 0.1], [0.1, 0.8]])
    Q, R, u, y = 1e-2 * np.eye(2), 1e-1 * np.eye(1), np.array([0.4]), np.array([-0.2])
    r = ekf.step_batch(x[None], P[None], y[None], u, Q, R)
    xt, Pt = Twin(m).step(x, P, y, u, Q, R)
    xw, Pw = Twin(m, c_at_apriori=True).step(x, P, y, u, Q, R)
    e = max(relerr(r["x"][0], xt), relerr(r["P"][0], Pt))
    d = max(relerr(xw, xt), relerr(Pw, Pt))
    print(f"evaluation point: kernel - twin = {e:.3e}, (C at x-) - twin = {d:.3e}")
    assert r["status"][0] == 0
    assert e < 1e-12                   # (a dozen multiply-adds on numbers of size 1: round-off only)
    assert d > 1e-3                    # the other evaluation point is a different filter, not round-off


def continuous_case(name, seed=3):
    """start values, inputs and five measurements of a continuous example: deterministic, of the size of the example's own states"""
    m = CASES[name].build_model()
    rng = np.random.default_rng(seed)
    nx, ny = m.n_x, m.n_y
    if name == "CSTR":
        x = CASES[name].X0 * (1.0 + 0.02 * rng.uniform(-1, 1, nx))
        u = np.array([20.0, -3000.0])
        P = np.diag([1e-2, 1e-2, 1.0, 1.0])
        Q, R = np.diag([1e-4, 1e-4, 1e-2, 1e-2]), np.diag([1e-3, 1e-3, 1e-1, 1e-1])
        ys = [x * (1.0 + 0.01 * rng.uniform(-1, 1, ny)) for _ in range(5)]
    else:
        x = 0.3 * rng.uniform(-1, 1, nx)
        u = np.array([0.5, -0.3])
        Aq = rng.uniform(-1, 1, (nx, nx))
        P = 0.1 * np.eye(nx) + 0.01 * Aq @ Aq.T
        Q, R = 1e-3 * np.eye(nx), 1e-2 * np.eye(ny)
        ys = [np.concatenate([0.3 * rng.uniform(-1, 1, 3), u + 0.01 * rng.uniform(-1, 1, 2)]) for _ in range(5)]
    return m, x, P, u, Q, R, ys


def continuous_twin_runs(name):
    """five steps of the twin at rtol = atol = 1e-12 and at 1e-13 -> (trajectory at 1e-12, difference between the two runs)"""
    m, x, P, u, Q, R, ys = continuous_case(name)
    ekf = make_ekf(name, hostemu=True, model=m)
    p, tvp = p_tvp(ekf)
    out = []
    for tol in (1e-12, 1e-13):
        tw = Twin(m, t_step=T_STEP[name], rtol=tol, atol=tol)
        xs, Ps, traj = x.copy(), P.copy(), []
        for y in ys:
            xs, Ps = tw.step(xs, Ps, y, u, Q, R, p=p, tvp=tvp)
            traj.append((xs.copy(), Ps.copy()))
        out.append(traj)
    diff = max(max(relerr(a[0], b[0]), relerr(a[1], b[1])) for a, b in zip(*out))
    return out[0], diff


def check_continuous(name, hostemu):
    """five filter steps (abstol = reltol = 1e-10) against the twin integrated at 1e-12; bound: the 1e-9 (relative, floor 1) the plant
    integrator meets with the same pair and safety factor (simulator_common.check_against_scipy), or ten times the twin's own
    integration error (its runs at 1e-12 and 1e-13 compared) if that is larger"""
    m, x, P, u, Q, R, ys = continuous_case(name)
    ekf = make_ekf(name, hostemu, model=m)
    p, tvp = p_tvp(ekf)
    ref, twin_diff = continuous_twin_runs(name)
    bound = max(1e-9, 10.0 * twin_diff)
    xs, Ps, worst = x.copy(), P.copy(), 0.0
    for k, y in enumerate(ys):
        r = ekf.step_batch(xs[None], Ps[None], y[None], u, Q, R)
        assert r["status"][0] == 0 and r["n_steps"][0] >= 1
        xs, Ps = r["x"][0], r["P"][0]
        worst = max(worst, relerr(xs, ref[k][0]), relerr(Ps, ref[k][1]))
    print(f"{name}: kernel - twin(1e-12) = {worst:.3e}, twin(1e-12) - twin(1e-13) = {twin_diff:.3e}, bound = {bound:.3e}, steps of the last interval = {int(r['n_steps'][0])}")
    assert worst < bound


def random_filters(model, B, seed=11, scale=0.3, offset=0.0):
    """B filters with distinct x (around `offset`), P (symmetric positive definite), y, u and per-filter Q, R"""
    rng = np.random.default_rng(seed)
    nx, ny, nu = model.n_x, model.n_y, model.n_u
    X = offset + scale * rng.uniform(-1, 1, (B, nx))
    G = rng.uniform(-1, 1, (B, nx, nx))
    Pc = 0.1 * np.eye(nx)[None] + 0.02 * G @ G.transpose(0, 2, 1)
    Y = scale * rng.uniform(-1, 1, (B, ny))
    U = scale * rng.uniform(-1, 1, (B, nu))
    Q = np.eye(nx)[None] * (1e-3 * (1.0 + rng.uniform(0, 1, (B, 1, 1))))
    R = np.eye(ny)[None] * (1e-2 * (1.0 + rng.uniform(0, 1, (B, 1, 1))))
    return X, Pc, Y, U, Q, R


NAN_PATTERN = np.frombuffer(np.uint64(0x7FF8DEADBEEF0123).tobytes(), dtype=np.float64)[0]


def raw_step_batch(ekf, B, X, Pc, Y, U, Q, R, tail=2):
    """the host entry of the C ABI on arrays with `tail` more rows than B, those rows filled with a NaN pattern (inputs and outputs):
    returns the outputs INCLUDING the tail rows"""
    m = ekf.model
    p, tvp = p_tvp(ekf)

    def padded(a, row_shape):
        out = np.full((B + tail,) + row_shape, NAN_PATTERN)
        out[:B] = np.asarray(a, float).reshape((B,) + row_shape)
        return out
    Xp, Pp, Yp, Up = padded(X, (m.n_x,)), padded(Pc, (m.n_x, m.n_x)), padded(Y, (m.n_y,)), padded(U, (m.n_u,))
    shared_q, shared_r = np.asarray(Q).ndim == 2, np.asarray(R).ndim == 2
    Qp = np.ascontiguousarray(Q, dtype=float) if shared_q else padded(Q, (m.n_x, m.n_x))
    Rp = np.ascontiguousarray(R, dtype=float) if shared_r else padded(R, (m.n_y, m.n_y))
    xo, Po = np.full_like(Xp, NAN_PATTERN), np.full_like(Pp, NAN_PATTERN)
    st = np.full(B + tail, -7, dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    pa, ta = np.ascontiguousarray(p if p.size else np.zeros(1)), np.ascontiguousarray(tvp if tvp.size else np.zeros(1))
    rc = ekf._lib.dompc_ekf_step_batch(ekf._h, B, ptr(Xp), ptr(Pp), ptr(Yp), ptr(Up), ptr(ta), ptr(pa), ptr(Qp), ptr(Rp),
                                       2 | 4 | (8 if shared_q else 0) | (16 if shared_r else 0), ptr(xo), ptr(Po), ptr(st))
    assert rc == 0, ekf._lib.dompc_ekf_last_error(ekf._h)
    return xo, Po, st


def check_batch_semantics(ekf, B, shared_qr, offset=0.0):
    """row b of a batch call equals the single call of filter b bit for bit; nothing behind row B is written"""
    X, Pc, Y, U, Q, R = random_filters(ekf.model, B, seed=100 + B, offset=offset)
    if shared_qr:
        Q, R = Q[0], R[0]
    xo, Po, st = raw_step_batch(ekf, B, X, Pc, Y, U, Q, R)
    assert np.all(st[:B] & 0xFF == 0), st
    tail_bits = lambda a: np.ascontiguousarray(a[B:]).view(np.uint64)      # noqa: E731
    assert np.all(tail_bits(xo) == 0x7FF8DEADBEEF0123) and np.all(tail_bits(Po) == 0x7FF8DEADBEEF0123) and np.all(st[B:] == -7)
    assert np.all(np.isfinite(xo[:B])) and np.all(np.isfinite(Po[:B]))
    for b in range(B):
        one = ekf.step_batch(X[b:b + 1], Pc[b:b + 1], Y[b:b + 1], U[b:b + 1], Q if shared_qr else Q[b], R if shared_qr else R[b])
        assert np.array_equal(one["x"][0], xo[b]) and np.array_equal(one["P"][0], Po[b]), (B, b)
    # ... and agrees with the twin
    p, tvp = p_tvp(ekf)
    tw = Twin(ekf.model, t_step=ekf.settings.t_step)
    b = B - 1
    xt, Pt = tw.step(X[b], Pc[b], Y[b], U[b], Q if shared_qr else Q[b], R if shared_qr else R[b], p=p, tvp=tvp)
    assert max(relerr(xo[b], xt), relerr(Po[b], Pt)) < 1e-9
