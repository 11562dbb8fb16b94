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

    def predict(self, x, P, u, Q, p=(), tvp=()):
        """-> (a-priori x, a-priori P, C at the evaluation point of the measurement update)"""
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
        return xa, Pa, C

    def update(self, xa, Pa, C, y, u, R, p=(), tvp=()):
        u, p, tvp = (np.asarray(a, float).ravel() for a in (u, p, tvp))
        L = Pa @ C.T @ np.linalg.inv(C @ Pa @ C.T + R)
        xn = xa + L @ (np.asarray(y, float).ravel() - self._ev(self._h, xa, u, tvp, p))
        Pn = (np.eye(self.m.n_x) - L @ C) @ Pa
        return xn, Pn

    def step(self, x, P, y, u, Q, R, p=(), tvp=()):
        xa, Pa, C = self.predict(x, P, u, Q, p=p, tvp=tvp)
        return self.update(xa, Pa, C, y, u, R, p=p, tvp=tvp)


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


# ---------------------------------------------------------------------------------------------- unequal problems in one wavefront (ODE filters)
# On the device the integration loop runs to the slowest filter of the wavefront (wave_any), a finished filter steps with h = 0 and keeps
# its values by select, idle groups of the last wavefront repeat the last filter.  The host emulation runs one group at a time, so "row b
# equals the single call of filter b" is trivially true there: these checks are made for their GPU twins.
NAN_BITS = 0x7FF8DEADBEEF0123
_ONCE = {}


def unequal_cstr_filters():
    """eight CSTR filters with shared P, Q, R whose integrations take 51 .. 64 steps on the host emulation: the temperatures scaled by
    0.9 .. 1.1, the feed by 0.3 .. 4.0, the measurement 0.5 % off the state"""
    m, x, P, u, Q, R, _ = continuous_case("CSTR")
    X, U = np.tile(x, (8, 1)), np.tile(u, (8, 1))
    X[:, 2:4] *= np.linspace(0.9, 1.1, 8)[:, None]
    U[:, 0] *= np.linspace(0.3, 4.0, 8)
    return m, X, P, 1.005 * X, U, Q, R


def slowest_last(B):
    """members of unequal_cstr_filters for a batch of B: the first B - 1 and the slowest one (member 7) in the last slot, so that the
    idle groups of the partial wavefront repeat the filter that keeps the loop alive"""
    return list(range(8)) if B == 8 else list(range(B - 1)) + [7]


def _tail_untouched(B, xo, Po, st):
    bits = lambda a: np.ascontiguousarray(a[B:]).view(np.uint64)      # noqa: E731
    return bool(np.all(bits(xo) == NAN_BITS) and np.all(bits(Po) == NAN_BITS) and np.all(st[B:] == -7))


def _rows_equal_single_calls(ekf, B, X, Pc, Y, U, Q, R, xo, Po, st, rows=None):
    """row b of the batch = the single call of filter b bit for bit: x, P (NaN = NaN) and the whole status word"""
    per = lambda a, b, nd: a if np.asarray(a).ndim == nd else a[b:b + 1]      # noqa: E731
    for b in (range(B) if rows is None else rows):
        x1, P1, s1 = raw_step_batch(ekf, 1, X[b:b + 1], per(Pc, b, 2), Y[b:b + 1], U[b:b + 1], per(Q, b, 2), per(R, b, 2))
        assert np.array_equal(x1[0], xo[b], equal_nan=True) and np.array_equal(P1[0], Po[b], equal_nan=True), (B, b)
        assert s1[0] == st[b], (B, b, s1[0], st[b])


def check_unequal_steps(ekf, B):
    """B = 8, 7 or 5 of unequal_cstr_filters (slowest_last): neighbours in a wavefront take different numbers of integration steps
    (asserted on the returned counts: max - min >= 3 in every group of four that has more than one member), every row equals its single
    call bit for bit, nothing behind row B is written, and one member agrees with the twin at the bound of check_continuous"""
    m, X, P, Y, U, Q, R = unequal_cstr_filters()
    idx = slowest_last(B)
    X, Y, U = X[idx], Y[idx], U[idx]
    Pc = np.tile(P, (B, 1, 1))
    xo, Po, st = raw_step_batch(ekf, B, X, Pc, Y, U, Q, R)
    steps = st[:B] >> 8
    print(f"B = {B}: members {idx}, status {st[:B] & 0xFF}, steps {steps}")
    assert np.all(st[:B] & 0xFF == 0), st
    for g in range(0, B, 4):
        if len(steps[g:g + 4]) > 1:
            assert steps[g:g + 4].max() - steps[g:g + 4].min() >= 3, steps
    assert steps[B - 1] == steps.max()                      # (the member the idle groups repeat is the slowest)
    assert _tail_untouched(B, xo, Po, st)
    assert np.all(np.isfinite(xo[:B])) and np.all(np.isfinite(Po[:B]))
    _rows_equal_single_calls(ekf, B, X, Pc, Y, U, Q, R, xo, Po, st)
    # ... and member 3 against the twin (computed once per process)
    if "unequal twin" not in _ONCE:
        p, tvp = p_tvp(ekf)
        runs = [Twin(m, t_step=T_STEP["CSTR"], rtol=tol, atol=tol).step(X[3], P, Y[3], U[3], Q, R, p=p, tvp=tvp) for tol in (1e-12, 1e-13)]
        _ONCE["unequal twin"] = (runs[0], max(relerr(runs[0][0], runs[1][0]), relerr(runs[0][1], runs[1][1])))
    (xt, Pt), twin_diff = _ONCE["unequal twin"]
    bound = max(1e-9, 10.0 * twin_diff)
    err = max(relerr(xo[3], xt), relerr(Po[3], Pt))
    print(f"B = {B}: member 3, kernel - twin(1e-12) = {err:.3e}, twin(1e-12) - twin(1e-13) = {twin_diff:.3e}, bound = {bound:.3e}")
    assert err < bound


def check_failures_beside_neighbours(ekf, last=None):
    """unequal_cstr_filters with per-filter P, Q, R: member 1 has a NaN measurement (bit 1), member 2 a NaN in its prior state (bits 0
    and 1, one step), member 3 P = Q = R = 0 (S = 0: bit 1).  The five good members are bit-equal to the run without failures, every
    member to its single call; a member with bit 1 hands out its a-priori x and P (against the twin's prediction at the bound of
    check_continuous; P = 0 stays 0 exactly); P is finite everywhere, x everywhere but in member 2.
    last: B = 7 without member 7 and with that failing member in the last slot - the idle group repeats a filter that fails"""
    m, X, P, Y, U, Q, R = unequal_cstr_filters()
    idx = list(range(8)) if last is None else [b for b in range(7) if b != last] + [last]
    B = len(idx)
    Pc, Qc, Rc = (np.tile(a, (8, 1, 1)) for a in (P, Q, R))
    good = raw_step_batch(ekf, B, X[idx], Pc[idx], Y[idx], U[idx], Qc[idx], Rc[idx])
    assert np.all(good[2][:B] & 0xFF == 0), good[2]
    Xf, Yf = X.copy(), Y.copy()
    Yf[1, 0] = np.nan
    Xf[2, 0] = np.nan
    Pc[3], Qc[3], Rc[3] = 0.0, 0.0, 0.0
    args = (Xf[idx], Pc[idx], Yf[idx], U[idx], Qc[idx], Rc[idx])
    xo, Po, st = raw_step_batch(ekf, B, *args)
    print(f"members {idx}: status {st[:B] & 0xFF}, steps {st[:B] >> 8}")
    expect = np.array([{1: 2, 2: 3, 3: 2}.get(b, 0) for b in idx])
    assert np.array_equal(st[:B] & 0xFF, expect), (st[:B] & 0xFF, expect)
    assert _tail_untouched(B, xo, Po, st)
    slot = {b: i for i, b in enumerate(idx)}
    assert np.all(np.isfinite(Po[:B])) and np.all(np.isfinite(np.delete(xo[:B], slot[2], axis=0))) and not np.all(np.isfinite(xo[slot[2]]))
    for b in idx:
        if b not in (1, 2, 3):
            i = slot[b]
            assert np.array_equal(xo[i], good[0][i]) and np.array_equal(Po[i], good[1][i]) and st[i] == good[2][i], b
    _rows_equal_single_calls(ekf, B, *args, xo, Po, st)
    # the documented return values of bit 1: the a-priori x and P
    if "apriori twin" not in _ONCE:
        p, tvp = p_tvp(ekf)
        out = {}
        for b in (1, 3):
            runs = [Twin(m, t_step=T_STEP["CSTR"], rtol=tol, atol=tol).predict(Xf[b], Pc[b], U[b], Qc[b], p=p, tvp=tvp)[:2] for tol in (1e-12, 1e-13)]
            out[b] = (runs[0], max(relerr(runs[0][0], runs[1][0]), relerr(runs[0][1], runs[1][1])))
        _ONCE["apriori twin"] = out
    for b in (1, 3):
        (xa, Pa), twin_diff = _ONCE["apriori twin"][b]
        bound = max(1e-9, 10.0 * twin_diff)
        err = max(relerr(xo[slot[b]], xa), relerr(Po[slot[b]], Pa))
        print(f"member {b} (bit 1): kernel - twin's a-priori estimate = {err:.3e}, bound = {bound:.3e}")
        assert err < bound
    assert not Po[slot[3]].any()


def check_step_limit_inside_a_wavefront(hostemu):
    """max_steps = the upper median of the step counts the eight filters take without a limit (57 on the host emulation): the filters
    that need more report bit 0 with max_steps steps, the others finish with status 0; every member equals its single call under the
    same limit bit for bit, and everything is finite"""
    m, X, P, Y, U, Q, R = unequal_cstr_filters()
    free = make_ekf("CSTR", hostemu, model=m).step_batch(X, np.tile(P, (8, 1, 1)), Y, U, Q, R)
    limit = int(np.sort(free["n_steps"])[4])
    over = free["n_steps"] > limit
    assert np.all(free["status"] == 0) and over.any() and not over.all() and over[4:].any() and not over[4:].all(), free["n_steps"]
    ekf = make_ekf("CSTR", hostemu, model=m, max_steps=limit)
    Pc = np.tile(P, (8, 1, 1))
    xo, Po, st = raw_step_batch(ekf, 8, X, Pc, Y, U, Q, R)
    print(f"max_steps = {limit}: status {st[:8] & 0xFF}, steps {st[:8] >> 8} (without a limit: {free['n_steps']})")
    assert np.array_equal(st[:8] & 0xFF, over.astype(int))
    assert np.array_equal(st[:8] >> 8, np.minimum(free["n_steps"], limit))
    assert np.all(np.isfinite(xo[:8])) and np.all(np.isfinite(Po[:8])) and _tail_untouched(8, xo, Po, st)
    fin = np.flatnonzero(~over)
    assert np.array_equal(xo[fin], free["x"][fin]) and np.array_equal(Po[fin], free["P"][fin])      # (the limit changes nothing for them)
    _rows_equal_single_calls(ekf, 8, X, Pc, Y, U, Q, R, xo, Po, st)


def check_status_bit_1_beside_neighbours(hostemu, slot, B=5):
    """tests/test_ekf.py::test_singular_s_returns_the_a_priori_estimate_with_status_bit_1 inside a batch of B triple-tank filters: the
    member in `slot` has P = Q = R = 0 (S = 0) and then a NaN measurement; it reports bit 1 and hands out its a-priori estimate, the
    others report 0 and equal their single calls bit for bit"""
    ekf = make_ekf("triple_tank", hostemu)
    m = ekf.model
    X, Pc, Y, U, Q, R = random_filters(m, B, seed=300 + slot, offset=2.0)
    p, tvp = p_tvp(ekf)
    for what in ("S = 0", "NaN measurement"):
        Pb, Qb, Rb, Yb = Pc.copy(), Q.copy(), R.copy(), Y.copy()
        if what == "S = 0":
            Pb[slot], Qb[slot], Rb[slot] = 0.0, 0.0, 0.0
        else:
            Yb[slot, 0] = np.nan
        xo, Po, st = raw_step_batch(ekf, B, X, Pb, Yb, U, Qb, Rb)
        print(f"triple tank, {what} in slot {slot} of {B}: status {st[:B] & 0xFF}")
        expect = np.zeros(B, dtype=int)
        expect[slot] = 2
        assert np.array_equal(st[:B] & 0xFF, expect) and _tail_untouched(B, xo, Po, st)
        assert np.all(np.isfinite(xo[:B])) and np.all(np.isfinite(Po[:B]))
        x_prior = np.asarray(m._rhs_fun.eval(X[slot], U[slot], np.zeros(0), tvp, p, np.zeros(0))[0], float).ravel()
        A = Twin(m)._ev(Twin(m)._A, X[slot], U[slot], tvp, p, (m.n_x, m.n_x))
        assert relerr(xo[slot], x_prior) < 1e-12 and relerr(Po[slot], A @ Pb[slot] @ A.T + Qb[slot]) < 1e-12      # (round-off only)
        if what == "S = 0":
            assert not Po[slot].any()
        _rows_equal_single_calls(ekf, B, X, Pb, Yb, U, Qb, Rb, xo, Po, st)


def check_step_limit(hostemu, B=5):
    """tests/test_ekf.py::test_step_limit_sets_status_bit_0 for B filters: max_steps = 3 is not enough for any of them"""
    ekf = make_ekf("rotating_masses", hostemu, max_steps=3)
    m, x, P, u, Q, R, ys = continuous_case("rotating_masses")
    X = np.tile(x, (B, 1)) * np.linspace(0.5, 1.5, B)[:, None]
    r = ekf.step_batch(X, np.tile(P, (B, 1, 1)), np.tile(ys[0], (B, 1)), u, Q, R)
    print(f"rotating masses, max_steps = 3: status {r['status']}, steps {r['n_steps']}")
    assert np.all(r["status"] == 1) and np.all(r["n_steps"] == 3) and np.all(np.isfinite(r["x"])) and np.all(np.isfinite(r["P"]))


# ---------------------------------------------------------------------------------------------- row swaps in the elimination of S
def _pivot_order(S):
    """row order of partial pivoting on S' (the matrix the filter eliminates: M = S')"""
    from scipy.linalg import lu
    return tuple(int(i) for i in np.argmax(lu(S.T)[0], axis=0))


def swapping_r(C, Pa, B, seed=4):
    """B full, non-symmetric R = (1e-2 I + 0.3 uniform(-1, 1)) with permuted rows, redrawn until partial pivoting on S' = (C P- C' + R)'
    takes a row order that is not the identity and cond(S) <= 100 - decided from the twin's a-priori covariance, without the kernel.
    n_y = 2 has one such order only: there the even members are drawn until they need NO swap, so that neighbours still differ"""
    rng = np.random.default_rng(seed)
    ny = C.shape[0]
    out = []
    for _ in range(1000):
        R = (1e-2 * np.eye(ny) + 0.3 * rng.uniform(-1, 1, (ny, ny)))[rng.permutation(ny)]
        S = C @ Pa @ C.T + R
        swaps = _pivot_order(S) != tuple(range(ny))
        if np.linalg.cond(S) <= 100.0 and swaps == (ny > 2 or len(out) % 2 == 1):
            out.append(R)
            if len(out) == B:
                return np.stack(out)
    raise AssertionError("no such R in 1000 draws")


def check_row_swaps(name, hostemu, B=6):
    """B filters of one state with per-filter R from swapping_r: S needs row swaps in the elimination (asserted on the CPU: no order
    is the identity and at least three different orders occur - n_y = 2: swap and no swap alternate -, cond(S) <= 100), so the four
    filters of a wavefront swap differently.  Posterior against the twin (continuous: bound of check_continuous; discrete: the 1e-10
    of the large-batch test), batch rows equal single calls bit for bit.  Measured on the host emulation:
    tests/test_ekf.py::test_elimination_of_s_with_row_swaps"""
    if name == "oscillating_masses":
        ekf = make_ekf(name, hostemu)
        m = ekf.model
        X, Pc, Y, U, Q, _ = random_filters(m, 1, seed=21)
        x, P, y, u, Q = X[0], Pc[0], Y[0], U[0], Q[0]
    else:
        m, x, P, u, Q, _, ys = continuous_case(name)
        ekf = make_ekf(name, hostemu, model=m)
        y = ys[0]
    p, tvp = p_tvp(ekf)
    if ("swaps", name) not in _ONCE:
        tols = (1e-12, 1e-13) if m.model_type == "continuous" else (1e-12,)
        _ONCE[("swaps", name)] = [Twin(m, t_step=T_STEP[name], rtol=tol, atol=tol).predict(x, P, u, Q, p=p, tvp=tvp) for tol in tols]
    pred = _ONCE[("swaps", name)]
    xa, Pa, C = pred[0]
    Rs = swapping_r(C, Pa, B)
    orders = [_pivot_order(C @ Pa @ C.T + R) for R in Rs]
    conds = [float(np.linalg.cond(C @ Pa @ C.T + R)) for R in Rs]
    print(f"{name}: pivot orders {orders}, cond(S) <= {max(conds):.1f}")
    ident = tuple(range(m.n_y))
    if m.n_y > 2:
        assert all(o != ident for o in orders) and len(set(orders)) >= 3
    else:
        assert all((o != ident) == (b % 2 == 1) for b, o in enumerate(orders))
    assert max(conds) <= 100.0
    assert len(set(orders[:4])) >= 2                      # (the first wavefront itself holds different orders)
    tw = Twin(m)
    ref = [[tw.update(q[0], q[1], q[2], y, u, R, p=p, tvp=tvp) for R in Rs] for q in pred]
    twin_diff = max(max(relerr(a[0], b[0]), relerr(a[1], b[1])) for a, b in zip(ref[0], ref[-1])) if len(ref) > 1 else 0.0
    bound = max(1e-9, 10.0 * twin_diff) if m.model_type == "continuous" else 1e-10
    X, Pc, Y, U, Qc = np.tile(x, (B, 1)), np.tile(P, (B, 1, 1)), np.tile(y, (B, 1)), np.tile(u, (B, 1)), np.tile(Q, (B, 1, 1))
    xo, Po, st = raw_step_batch(ekf, B, X, Pc, Y, U, Qc, Rs)
    assert np.all(st[:B] & 0xFF == 0), st
    assert _tail_untouched(B, xo, Po, st)
    worst = max(max(relerr(xo[b], ref[0][b][0]), relerr(Po[b], ref[0][b][1])) for b in range(B))
    print(f"{name}: kernel - twin = {worst:.3e}, bound = {bound:.3e}")
    assert worst < bound
    _rows_equal_single_calls(ekf, B, X, Pc, Y, U, Qc, Rs, xo, Po, st)
