"""Shared helpers of the plant-integrator tests on lanes that do unequal work (host emulation on CPU, HIP path under -m gpu).

A probe family with a closed form (csrc/dompc_plant.hip runs one sample per thread: per lane its own step sequence, accept / reject
decisions, explicit-to-implicit fallback and Newton solve):

  ODE member   x0' = -lam x0 + u + d + sqrt(q) + w0        parameters lam, om, q; time-varying parameter d
               x1' =  om x2 + w1                           y0 = x0 + 2 x1 x2 + v0
               x2' = -om x1 + d + w2                       y1 = u x2 - d + v1
  DAE member   the same x(t) with z in R^2:  x0' = -z1 + ..., x1' = z0 + w1, 0 = z1 - lam x0, 0 = z0 - om x2; y1 carries + z0.
               The Jacobian of the algebraic rows is [[0, 1], [1, 0]]: the first pivot of every elimination is zero.
  discrete     x+ = the ODE member's right-hand side.

`lam` sets the stiffness of a lane, `om` its step count, q < 0 makes its right-hand side NaN.  The references are the closed form
(a scalar exponential and a forced rotation, plain float64; checked once against scipy.linalg.expm) and a numpy twin of the explicit
pair (the published Dormand-Prince 5(4) tableau as exact fractions and the controller of the kernel).  The twin and the closed form
decide what every lane must do and which lanes count; the code under test decides neither.  Every condition on the inputs is asserted
here, from the twin alone, before the kernel's output is looked at."""
import hostemu_build
from fractions import Fraction as Fr

import numpy as np

from do_mpc_amd import Model, sym
from do_mpc_amd.examples import CASES
from do_mpc_amd.simulator import Simulator

import simulator_common as sc

OUT = sc.OUT
T_STEP = 0.1
CAP = 300                    # explicit_limit (method 0) / max_steps (method 1) of the checks
SEED = 336                   # of the B = 130 batch; the smaller batches are its first rows
SIZES = (63, 64, 65, 130)

# ------------------------------------------------------------------------------------------------ the published pair, as fractions
# Dormand & Prince, "A family of embedded Runge-Kutta formulae", J. Comput. Appl. Math. 6 (1980), table 2 (RK5(4)7M); row 7 = b (FSAL)
DP_C = [Fr(0), Fr(1, 5), Fr(3, 10), Fr(4, 5), Fr(8, 9), Fr(1), Fr(1)]
DP_A = [[],
        [Fr(1, 5)],
        [Fr(3, 40), Fr(9, 40)],
        [Fr(44, 45), Fr(-56, 15), Fr(32, 9)],
        [Fr(19372, 6561), Fr(-25360, 2187), Fr(64448, 6561), Fr(-212, 729)],
        [Fr(9017, 3168), Fr(-355, 33), Fr(46732, 5247), Fr(49, 176), Fr(-5103, 18656)],
        [Fr(35, 384), Fr(0), Fr(500, 1113), Fr(125, 192), Fr(-2187, 6784), Fr(11, 84)]]
DP_B = DP_A[6] + [Fr(0)]                                                              # order 5, continues the solution
DP_BHAT = [Fr(5179, 57600), Fr(0), Fr(7571, 16695), Fr(393, 640), Fr(-92097, 339200), Fr(187, 2100), Fr(1, 40)]      # order 4
DP_E = [b - bh for b, bh in zip(DP_B, DP_BHAT)]                                       # the embedded error estimate
TOL_SAFETY = 0.01            # the local error is controlled at this fraction of (abstol, reltol)


def order_condition_residuals(b, order):
    """left side minus right side of the order conditions of a Runge-Kutta method (one per rooted tree, Hairer, Norsett, Wanner
    II.2) up to `order` <= 5 for the weights `b` on the nodes and matrix of the pair, in rationals"""
    n = len(DP_C)
    A = [[(DP_A[i][j] if j < len(DP_A[i]) else Fr(0)) for j in range(n)] for i in range(n)]
    c = DP_C
    mul = lambda u, v: [a * b_ for a, b_ in zip(u, v)]                                # noqa: E731
    Av = lambda v: [sum(A[i][j] * v[j] for j in range(n)) for i in range(n)]          # noqa: E731
    dot = lambda v: sum(bi * vi for bi, vi in zip(b, v))                              # noqa: E731
    one = [Fr(1)] * n
    c2, c3 = mul(c, c), mul(mul(c, c), c)
    Ac, Ac2 = Av(c), Av(c2)
    trees = [(1, one, Fr(1)), (2, c, Fr(1, 2)),
             (3, c2, Fr(1, 3)), (3, Ac, Fr(1, 6)),
             (4, c3, Fr(1, 4)), (4, mul(c, Ac), Fr(1, 8)), (4, Ac2, Fr(1, 12)), (4, Av(Ac), Fr(1, 24)),
             (5, mul(c2, c2), Fr(1, 5)), (5, mul(c2, Ac), Fr(1, 10)), (5, mul(Ac, Ac), Fr(1, 20)), (5, mul(c, Ac2), Fr(1, 15)),
             (5, Av(c3), Fr(1, 20)), (5, mul(c, Av(Ac)), Fr(1, 30)), (5, Av(mul(c, Ac)), Fr(1, 40)), (5, Av(Ac2), Fr(1, 60)),
             (5, Av(Av(Ac)), Fr(1, 120))]
    return [dot(v) - rhs for o, v, rhs in trees if o <= order]


# ------------------------------------------------------------------------------------------------ the family
def build_model(kind):
    m = Model("discrete" if kind == "discrete" else "continuous")
    x = m.set_variable("_x", "x", (3, 1))
    u = m.set_variable("_u", "u")
    lam, om, q = (m.set_variable("_p", n) for n in ("lam", "om", "q"))
    d = m.set_variable("_tvp", "d")
    force = u + d + sym.sqrt(q)
    if kind == "dae":
        z = m.set_variable("_z", "z", (2, 1))
        m.set_rhs("x", sym.vertcat(-z[1] + force, z[0], -om * x[1] + d), process_noise=True)
        m.set_alg("a0", z[1] - lam * x[0])
        m.set_alg("a1", z[0] - om * x[2])
    else:
        m.set_rhs("x", sym.vertcat(-lam * x[0] + force, om * x[2], -om * x[1] + d), process_noise=True)
    m.set_meas("y0", x[0] + 2.0 * x[1] * x[2], meas_noise=True)
    m.set_meas("y1", u * x[2] - d + (z[0] if kind == "dae" else 0.0), meas_noise=True)
    m.setup()
    return m


def alg_jacobian(m):
    """d alg / d z of the DAE member from the model's own expressions (constant)"""
    ins = [m._x.cat, m._u.cat, m._z.cat, m._tvp.cat, m._p.cat, m._w.cat]
    J = sym.Function("alg_jz", ins, [sym.jacobian(m._alg, m._z.cat)]).eval(np.ones(3), np.ones(1), np.ones(2), np.ones(1), np.ones(3), np.ones(3))[0]
    return np.asarray(J, float).reshape(2, 2, order="F")


_SIMS = {}


def make_simulator(kind, hostemu, tool="cvodes", tol=1e-10, max_steps=0, explicit_limit=CAP):
    """one simulator per (model, flavour, settings): the tests share them (and with them the built code objects)"""
    key = (kind, hostemu, tool, tol, max_steps, explicit_limit)
    if key in _SIMS:
        return _SIMS[key]
    m = build_model(kind)
    sim = Simulator(m)
    sim.set_param(integration_tool=tool, abstol=tol, reltol=tol, t_step=T_STEP, max_steps=max_steps,
                  integration_opts={"explicit_limit": explicit_limit})
    if m.n_p:
        pt = sim.get_p_template()
        sim.set_p_fun(lambda t: pt)
    if m.n_tvp:
        tv = sim.get_tvp_template()
        sim.set_tvp_fun(lambda t: tv)
    if hostemu:
        hdr = sim._lower()
        h = hdr.rsplit('PLANT_MODEL_HASH "', 1)[1].split('"')[0]
        sim.setup(_lib_path=hostemu_build.plant_hostemu_library(hdr, h, OUT), _code_object="")
    else:
        sim.setup()
    _SIMS[key] = sim
    return sim


def draw(B=130, seed=SEED):
    """per-sample, non-zero inputs: lam log-uniform in [1, 1e5], om log-uniform in [0.1, 30]"""
    rng = np.random.default_rng(seed)
    nz = lambda *shape: rng.uniform(0.2, 1.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)      # noqa: E731
    lam = 10.0 ** rng.uniform(0.0, 5.0, size=B)
    om = 10.0 ** rng.uniform(-1.0, np.log10(30.0), size=B)
    q = rng.uniform(0.1, 2.0, size=B)
    return {"X": nz(B, 3), "U": nz(B, 1), "TVP": nz(B, 1), "P": np.stack([lam, om, q], axis=1), "W": 0.3 * nz(B, 3), "V": 0.1 * nz(B, 2)}


def take(inp, rows):
    return {k: np.ascontiguousarray(v[rows]) for k, v in inp.items()}


def run(sim, inp, **kw):
    return sim.make_step_batch(inp["X"], inp["U"], P=inp["P"], TVP=inp["TVP"], W=inp["W"], V=inp["V"], **kw)


# ------------------------------------------------------------------------------------------------ references
def rhs_np(X, inp):
    lam, om, q = inp["P"].T
    u, d, W = inp["U"][:, 0], inp["TVP"][:, 0], inp["W"]
    with np.errstate(invalid="ignore"):
        return np.stack([-lam * X[:, 0] + u + d + np.sqrt(q) + W[:, 0], om * X[:, 2] + W[:, 1], -om * X[:, 1] + d + W[:, 2]], axis=1)


def meas_np(X, inp, dae=False):
    u, d, V = inp["U"][:, 0], inp["TVP"][:, 0], inp["V"]
    y1 = u * X[:, 2] - d + V[:, 1]
    if dae:
        y1 = y1 + inp["P"][:, 1] * X[:, 2]                 # z0 = om x2 at the new state
    return np.stack([X[:, 0] + 2.0 * X[:, 1] * X[:, 2] + V[:, 0], y1], axis=1)


def closed_form(inp, t=T_STEP):
    """x(t): x0 relaxes to c0 / lam, (x1, x2) rotates with om about (b / om, -a / om); w is constant forcing"""
    lam, om, q = inp["P"].T
    X, W = inp["X"], inp["W"]
    c0 = inp["U"][:, 0] + inp["TVP"][:, 0] + np.sqrt(q) + W[:, 0]
    a, b = W[:, 1], inp["TVP"][:, 0] + W[:, 2]
    x0 = c0 / lam + (X[:, 0] - c0 / lam) * np.exp(-lam * t)
    e1, e2 = b / om, -a / om
    co, si = np.cos(om * t), np.sin(om * t)
    d1, d2 = X[:, 1] - e1, X[:, 2] - e2
    return np.stack([x0, e1 + co * d1 + si * d2, e2 - si * d1 + co * d2], axis=1)


def closed_form_against_expm(inp, rows):
    """largest scaled difference of the formulas above from exp of the augmented matrix [[A, c], [0, 0]] t on `rows`"""
    from scipy.linalg import expm
    ref = closed_form(inp)
    worst = 0.0
    for r in rows:
        lam, om, q = inp["P"][r]
        u, d, w = inp["U"][r, 0], inp["TVP"][r, 0], inp["W"][r]
        M = np.zeros((4, 4))
        M[:3, :3] = [[-lam, 0, 0], [0, 0, om], [0, -om, 0]]
        M[:3, 3] = [u + d + np.sqrt(q) + w[0], w[1], d + w[2]]
        x = (expm(M * T_STEP) @ np.append(inp["X"][r], 1.0))[:3]
        worst = max(worst, float(np.max(np.abs(x - ref[r]) / np.maximum(1.0, np.abs(ref[r])))))
    return worst


def relerr(a, ref):
    """per row: the project's measure (check_against_scipy): relative with floor 1"""
    return np.max(np.abs(a - ref) / np.maximum(1.0, np.abs(ref)), axis=1)


def twin(inp, tol=1e-10, cap=CAP, t_step=T_STEP):
    """The explicit pair with the kernel's controller on every sample of `inp` (numpy over the samples, every sample its own step
    sequence): local tolerance TOL_SAFETY * tol, initial step 0.01 d0 / d1 (1e-6 for tiny norms, at most t_step), next step
    h * min(5, max(0.2, 0.9 err^-0.2)), first-same-as-last, a NaN error ends the sample, so does the step cap.
    -> x, n_steps, status (0 reached t_step, 1 NaN or cap), and what makes a comparison of step counts safe:
       margin      smallest |err - 1| over the sample's steps (distance of every accept / reject decision from its threshold)
       end_margin  smallest |t + h - t_step| / t_step over its steps (distance of every 'last step' decision from its threshold)
    (After the shortened last step t + (t_step - t) is t_step again whatever the roundings of t before: the difference is rounded by
    at most half an ulp of t_step, and the sum then rounds back to t_step - a tie goes to the even mantissa, which T_STEP has.)"""
    assert int(float(t_step).hex().split("p")[0][-1], 16) % 2 == 0
    A = [[float(a) for a in row] for row in DP_A]
    E = [float(e) for e in DP_E]
    rt, at = tol * TOL_SAFETY, tol * TOL_SAFETY
    f = lambda X: rhs_np(X, inp)                                                     # noqa: E731
    rms = lambda V: np.sqrt(np.sum(V * V, axis=1) / V.shape[1])                       # noqa: E731
    x = inp["X"].copy()
    B = x.shape[0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        k = [f(x)] + [None] * 6
        s0 = at + rt * np.abs(x)
        d0, d1 = rms(x / s0), rms(k[0] / s0)
        h = np.where((d0 < 1e-5) | (d1 < 1e-5), 1e-6, 0.01 * d0 / d1)
        h = np.where(h > t_step, t_step, h)
        t, n, status = np.zeros(B), np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
        margin, end_margin = np.full(B, np.inf), np.full(B, np.inf)
        active = np.ones(B, dtype=bool)
        while True:
            active &= t < t_step
            hit = active & (n >= cap)
            status[hit] = 1
            active &= ~hit
            if not active.any():
                break
            last = active & (t + h > t_step)
            end_margin = np.where(active, np.fmin(end_margin, np.abs(t + h - t_step) / t_step), end_margin)
            h = np.where(last, t_step - t, h)
            hc = h[:, None]
            for s in range(1, 7):
                acc = A[s][0] * k[0]
                for j in range(1, s):
                    if A[s][j] != 0.0:
                        acc = acc + A[s][j] * k[j]
                xs = x + hc * acc
                k[s] = f(xs)
            xn = xs                                                                   # row 7 of the tableau is b
            ei = hc * sum(E[j] * k[j] for j in range(7) if E[j] != 0.0)
            scale = at + rt * np.fmax(np.abs(x), np.abs(xn))
            err = rms(ei / scale)
            n += active
            nan = active & ~(err == err)
            acc_ = active & (err <= 1.0)
            t = np.where(acc_, t + h, t)
            x = np.where(acc_[:, None], xn, x)
            k[0] = np.where(acc_[:, None], k[6], k[0])
            status[nan] = 1
            active &= ~nan
            margin = np.where(active, np.fmin(margin, np.abs(err - 1.0)), margin)
            fac = np.fmin(5.0, np.fmax(0.2, 0.9 * np.power(np.fmax(err, 1e-10), -0.2)))
            h = np.where(active, h * fac, h)
    return {"x": x, "n_steps": n, "status": status, "margin": margin, "end_margin": end_margin, "t": t}


# every accept / reject decision of the twin is at least this far from its threshold.  Rounding and contraction move err by about
# 1e-6 at 1e-10 (h 1e-16 against a scale of 1e-12) and by 1e-10 at 1e-6: a factor of 1e3 and of 1e5
MARGIN = {1e-10: 1e-3, 1e-6: 1e-5}
_REF = {}


def conditions(inp, tol):
    """what the comparisons with the twin rest on, from the twin alone -> (twin, {condition: holds})"""
    tw = twin(inp, tol)
    near = twin(inp, tol, cap=CAP + 5)                     # a second run with a few steps more
    expl = tw["status"] == 0
    n = tw["n_steps"]
    ok = {"margin": tw["margin"].min() >= MARGIN[tol],
          "end_margin": tw["end_margin"].min() >= 1e-5,        # (h moves by a fifth of what err moves by)
          # no sample is within 5 steps of the cap, on either side: a sample whose decisions are not protected by the margin of the twin -
          # one at the cap, whose later steps the twin never took, or one of the DAE member, whose arithmetic differs - ends on the same side
          "clear_of_cap": bool(np.all(near["status"][~expl] == 1) and np.all(n[expl] <= CAP - 5))}
    if tol == 1e-10:
        full = [slice(lo, lo + 64) for lo in (0, 64)]      # the full wavefronts of the batch
        ok["each_status_in_each_wavefront"] = all(expl[w].sum() >= 8 and (~expl[w]).sum() >= 8 for w in full)
        ok["unequal_work_in_each_wavefront"] = all(n[w].max() >= 10 * n[w].min() for w in full)
    return tw, ok


def reference(tol=1e-10):
    """the B = 130 batch with its closed form and twin, computed once and left unchanged; asserts what the comparisons rest on"""
    if tol in _REF:
        return _REF[tol]
    inp = draw()
    tw, ok = conditions(inp, tol)
    assert all(ok.values()), ok
    ref = {"inp": inp, "x": closed_form(inp), "twin": tw, "explicit": tw["status"] == 0}
    for a in list(ref["inp"].values()) + [ref["x"]] + list(tw.values()):
        a.setflags(write=False)
    _REF[tol] = ref
    return ref


def expected_status(ref, method):
    """under the cap: 0; at the cap: 2 with method 0 and explicit_limit = CAP, 1 with method 1 and max_steps = CAP"""
    return np.where(ref["explicit"], 0, 2 if method == 0 else 1)


# ------------------------------------------------------------------------------------------------ checks (host emulation and device)
def check_values(kind, hostemu, B):
    """values against the closed form with the project's own bounds, status and (ODE member) step counts against the twin"""
    ref = reference()
    inp = take(ref["inp"], slice(0, B))
    r = run(make_simulator(kind, hostemu), inp)
    want = expected_status(ref, 0)[:B]
    assert np.array_equal(r["status"], want), np.nonzero(r["status"] != want)[0]
    expl = ref["explicit"][:B]
    if kind == "ode":
        assert np.array_equal(r["n_steps"][expl], ref["twin"]["n_steps"][:B][expl]), (r["n_steps"][expl], ref["twin"]["n_steps"][:B][expl])
        assert (r["n_steps"][~expl] > CAP).all()
    bound = np.where(expl, 1e-9, 2e-9)
    ex, ey = relerr(r["x"], ref["x"][:B]), relerr(r["y"], meas_np(ref["x"][:B], inp, dae=kind == "dae"))
    print(f"{kind} B={B}: explicit lanes {expl.sum()}, steps {r['n_steps'].min()} .. {r['n_steps'].max()}, "
          f"x error {ex[expl].max():.2e} / {ex[~expl].max():.2e}, y error {ey[expl].max():.2e} / {ey[~expl].max():.2e}")
    assert (ex < bound).all() and (ey < bound).all(), (ex.max(), ey.max())


def check_explicit_only(hostemu):
    """method 1, max_steps = CAP: the lanes at the cap report status 1 and CAP steps, the others are what method 0 gave"""
    ref = reference()
    r = run(make_simulator("ode", hostemu, tool="dopri5", max_steps=CAP), ref["inp"])
    assert np.array_equal(r["status"], expected_status(ref, 1))
    assert np.array_equal(r["n_steps"], ref["twin"]["n_steps"])
    expl = ref["explicit"]
    assert (relerr(r["x"], ref["x"])[expl] < 1e-9).all()


def check_implicit_only(kind, hostemu):
    ref = reference()
    r = run(make_simulator(kind, hostemu, tool="sdirk4"), ref["inp"])
    assert (r["status"] == 2).all(), r["status"]
    ex, ey = relerr(r["x"], ref["x"]), relerr(r["y"], meas_np(ref["x"], ref["inp"], dae=kind == "dae"))
    print(f"{kind} sdirk4: steps {r['n_steps'].min()} .. {r['n_steps'].max()}, x error {ex.max():.2e}, y error {ey.max():.2e}")
    assert ex.max() < 2e-9 and ey.max() < 2e-9


def check_looser_tolerance(hostemu):
    """abstol = reltol = 1e-6: error below 1e-5 (the factor of 10 the project grants at 1e-10), every explicit lane with fewer steps than
    at 1e-10 and with the twin's count at 1e-6"""
    tight, loose = reference(), reference(1e-6)
    r = run(make_simulator("ode", hostemu, tol=1e-6), loose["inp"])
    r10 = run(make_simulator("ode", hostemu), tight["inp"])
    expl = loose["explicit"]
    assert (expl & tight["explicit"]).sum() >= 16          # (lanes that are explicit at both settings)
    assert np.array_equal(r["status"], expected_status(loose, 0))
    assert np.array_equal(r["n_steps"][expl], loose["twin"]["n_steps"][expl])
    assert (r["n_steps"][expl] < r10["n_steps"][expl]).all()
    ex, ey = relerr(r["x"], loose["x"]), relerr(r["y"], meas_np(loose["x"], loose["inp"]))
    print(f"tol 1e-6: explicit lanes {expl.sum()}, x error {ex.max():.2e}, y error {ey.max():.2e}")
    assert ex.max() < 1e-5 and ey.max() < 1e-5


NAN_ROW = np.array([3.0, 1.0, -0.5])                       # q < 0: sqrt(q) is NaN
CAPPED_ROW = np.array([2.0, 300.0, 0.5])                    # thirty radians in the interval: about a thousand explicit steps
BENIGN_ROW = np.array([2.0, 1.0, 0.5])


def check_failures_stay_local(hostemu):
    """a lane with a NaN right-hand side and a lane at the step limit, in the middle of a wavefront and at lanes 0, 63 and 64: status 1,
    1 and CAP steps, x what the twin returns; every other row bit-identical to the batch with benign lanes in their place"""
    base = {k: v.copy() for k, v in reference()["inp"].items()}
    spots = (0, 30, 31, 63, 64)
    base["P"][list(spots)] = BENIGN_ROW
    arrangements = [({0: NAN_ROW, 63: NAN_ROW, 64: NAN_ROW, 30: NAN_ROW, 31: CAPPED_ROW}),
                    ({0: CAPPED_ROW, 63: CAPPED_ROW, 64: CAPPED_ROW, 31: CAPPED_ROW, 30: NAN_ROW})]
    others = np.setdiff1d(np.arange(130), spots)
    for method, sim in ((1, make_simulator("ode", hostemu, tool="dopri5", max_steps=CAP)), (0, make_simulator("ode", hostemu))):
        good = run(sim, base)
        assert (good["status"][list(spots)] == 0).all()
        for arr in arrangements:
            inp = {k: v.copy() for k, v in base.items()}
            for lane, row in arr.items():
                inp["P"][lane] = row
            at = take(inp, list(spots))
            tw = twin(at)
            assert tw["margin"].min() >= 1e-3
            for i, lane in enumerate(spots):               # what the twin says of these lanes
                assert tw["status"][i] == 1 and tw["n_steps"][i] == (1 if arr[lane] is NAN_ROW else CAP)
            r = run(sim, inp)
            for i, lane in enumerate(spots):
                nan_lane = arr[lane] is NAN_ROW
                if nan_lane:                               # no implicit retry for a NaN right-hand side, whatever the method
                    assert r["status"][lane] == 1 and r["n_steps"][lane] == 1
                    assert np.array_equal(r["x"][lane], inp["X"][lane]) and np.array_equal(tw["x"][i], inp["X"][lane])
                elif method == 1:
                    assert r["status"][lane] == 1 and r["n_steps"][lane] == CAP
                    # the state at the cap is a point of the true trajectory (1e-9, as for a whole interval), at the twin's time: the
                    # step sizes of the two differ by 2e-7 relative (a fifth of the 1e-6 by which rounding moves err; the next step
                    # 0.9 h err^-0.2 with err ~ h^5 does not depend on h, so that does not accumulate) - 2e-6 with a factor of 10.
                    # The time the kernel reached: the twin's, corrected by one Gauss-Newton step along the trajectory.
                    one = take(at, [i])
                    f = rhs_np(closed_form(one, tw["t"][i]), one)[0]
                    t_k = tw["t"][i] + float((r["x"][lane] - closed_form(one, tw["t"][i])[0]) @ f / (f @ f))
                    assert 0.0 < tw["t"][i] < T_STEP and abs(t_k - tw["t"][i]) < 2e-6 * tw["t"][i], (t_k, tw["t"][i])
                    assert relerr(r["x"][lane][None], closed_form(one, t_k))[0] < 1e-9
                else:
                    assert r["status"][lane] == 2 and r["n_steps"][lane] > CAP
            for k in ("x", "y", "status", "n_steps"):
                assert np.array_equal(r[k][others], good[k][others]), (method, k)


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("x", "y", "status", "n_steps"))


def check_position(kind, hostemu):
    """a permutation of the batch returns the permuted rows bit for bit (rows cross wavefronts); rows 0, 63, 64, 129 equal their B = 1 calls"""
    inp = reference()["inp"]
    sim = make_simulator(kind, hostemu)
    r = run(sim, inp)
    perm = np.random.default_rng(3).permutation(130)
    assert (perm // 64 != np.arange(130) // 64).sum() >= 32
    rp = run(sim, take(inp, perm))
    assert same(rp, {k: v[perm] for k, v in r.items()})
    for b in (0, 63, 64, 129):
        assert same(run(sim, take(inp, [b])), {k: v[b:b + 1] for k, v in r.items()}), b


def check_shared_rows(kind, hostemu, B=65):
    """one shared row of U, TVP, P, W or V gives the bits of that row tiled B times; W = None and V = None those of explicit zeros"""
    ref = reference()
    inp = take(ref["inp"], slice(0, B))
    sim = make_simulator(kind, hostemu)
    lane = int(np.nonzero(ref["explicit"][:B])[0][1])
    for name in ("U", "TVP", "P", "W", "V"):
        row = inp[name][lane].copy()
        shared = run(sim, dict(inp, **{name: row}))
        tiled = run(sim, dict(inp, **{name: np.tile(row, (B, 1))}))
        assert same(shared, tiled), name
        assert not np.array_equal(shared["y"] if name == "V" else shared["x"], run(sim, inp)["y" if name == "V" else "x"]), name
    for name in ("W", "V"):
        none = run(sim, dict(inp, **{name: None}))
        zeros = run(sim, dict(inp, **{name: np.zeros_like(inp[name])}))
        assert same(none, zeros), name


def check_discrete(hostemu, B=65):
    """x+ = rhs(x, u, d, p, w), y = meas(x+) + v against numpy.  A handful of operations, each moved by at most an ulp of its
    partial sum by contraction: 1e-14 relative to the sum of the magnitudes of an entry's terms"""
    inp = take(reference()["inp"], slice(0, B))
    r = run(make_simulator("discrete", hostemu), inp)
    X, (lam, om, q) = np.abs(inp["X"]), inp["P"].T
    u, d, W, V = (np.abs(inp[k]) for k in ("U", "TVP", "W", "V"))
    xn = rhs_np(inp["X"], inp)
    x_scale = np.stack([lam * X[:, 0] + u[:, 0] + d[:, 0] + np.sqrt(q) + W[:, 0], om * X[:, 2] + W[:, 1], om * X[:, 1] + d[:, 0] + W[:, 2]], axis=1)
    assert (r["status"] == 0).all() and (r["n_steps"] == 1).all()
    assert (np.abs(r["x"] - xn) <= 1e-14 * x_scale).all(), np.max(np.abs(r["x"] - xn) / x_scale)
    xk = np.abs(r["x"])                                    # the measurement of the kernel's own new state
    y_scale = np.stack([xk[:, 0] + 2.0 * xk[:, 1] * xk[:, 2] + V[:, 0], u[:, 0] * xk[:, 2] + d[:, 0] + V[:, 1]], axis=1)
    y = meas_np(r["x"], inp)
    assert (np.abs(r["y"] - y) <= 1e-14 * y_scale).all(), np.max(np.abs(r["y"] - y) / y_scale)


# ------------------------------------------------------------------------------------------------ dip: nonlinear Newton per lane
def dip_batch(B, seed=2):
    ex = CASES["dip"]
    s = np.random.default_rng(seed).uniform(0.0, 1.0, size=(B, 1))
    return ex.X0[None, :] * (1.0 - s) + (ex.X0 * 0.5 + 0.1)[None, :] * s


def check_dip_growing_z_buffer(hostemu):
    """B = 3, then 65, then 3 again with carry_z = False on a new simulator: the buffer of Newton starts is reallocated in between;
    the third call equals the first, and so do the first three rows of the middle one"""
    sim = sc.make_simulator("dip", hostemu)
    X, u = dip_batch(65), np.array(sc.U_TEST["dip"])
    a = sim.make_step_batch(X[:3], u, carry_z=False)
    b = sim.make_step_batch(X, u, carry_z=False)
    c = sim.make_step_batch(X[:3], u, carry_z=False)
    assert (a["status"] == 0).all() and (b["status"] == 0).all()
    assert same(c, a)
    assert same({k: v[:3] for k, v in b.items()}, a)
    sim.close()


def check_dip_permutation(hostemu, B=65):
    sim = sc.make_simulator("dip", hostemu)
    X, u = dip_batch(B), np.array(sc.U_TEST["dip"])
    perm = np.random.default_rng(4).permutation(B)
    assert perm[64] != 64 and (perm[:64] == 64).any()      # rows cross the wavefront boundary
    a = sim.make_step_batch(X, u)
    b = sim.make_step_batch(np.ascontiguousarray(X[perm]), u)
    assert (a["status"] == 0).all() and same(b, {k: v[perm] for k, v in a.items()})
    sim.close()
