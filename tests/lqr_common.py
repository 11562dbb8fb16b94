"""TEST-ONLY helpers of the LQR tests: the host emulation of csrc/dompc_lqr.hip (g++ -DDOMPC_HOST_EMU, the text that ships), a
numpy / scipy twin of the reference (scipy.linalg.solve_discrete_are, scipy.signal.cont2discrete, the recursion of
/root/reference/do_mpc/controller/_lqr.py:166-170) and the cases the CPU and the GPU suite share."""
import os
import warnings

import numpy as np
from scipy.linalg import solve_discrete_are
from scipy.signal import cont2discrete

from do_mpc_amd import sym
from do_mpc_amd.examples import CASES
from do_mpc_amd.lqr import LQR
from do_mpc_amd.model import LinearModel
from ekf_common import relerr  # noqa: F401  (the measure of the stored-run and gain comparisons)
from hostemu_build import OUT, lqr_hostemu_library

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def setup_lqr(lqr, hostemu):
    """lqr.setup() on the host-emulated kernel (every design the controller asks for gets its own library) or on the GPU"""
    if hostemu:
        lqr.setup(_lib_path=lqr_hostemu_library, _code_object="")
    else:
        lqr.setup()
    return lqr


def plant_on(sim, hostemu):
    if hostemu:
        from hostemu_build import plant_hostemu_library
        hdr = sim._lower()
        sim.setup(_lib_path=plant_hostemu_library(hdr, hdr.rsplit('PLANT_MODEL_HASH "', 1)[1].split('"')[0], OUT), _code_object="")
    else:
        sim.setup()
    return sim


# ---------------------------------------------------------------------------------------------- the twin
def twin_design(A, B, Q, R, n_horizon=None, P=None, rate=False, delR=None):
    """(K, P) the way the reference computes them; rate: inputRatePenalization mode with the model-size weights Q, R, P and delR"""
    A, B, Q, R = (np.asarray(a, float) for a in (A, B, Q, R))
    if rate:
        nx, nu = B.shape
        A = np.block([[A, B], [np.zeros((nu, nx)), np.eye(nu)]])
        B = np.block([[B], [np.eye(nu)]])
        z = np.zeros((nx, nu))
        if n_horizon is not None:
            P = np.block([[Q if P is None else P, z], [z.T, R]])
        Q = np.block([[Q, z], [z.T, R]])
        R = np.asarray(delR, float)
    elif n_horizon is not None and P is None:
        P = Q
    if n_horizon is not None:
        tp = P
        for _ in range(n_horizon):
            K = -np.linalg.inv(B.T @ tp @ B + R) @ B.T @ tp @ A
            tp = Q + A.T @ tp @ A - A.T @ tp @ B @ np.linalg.inv(B.T @ tp @ B + R) @ B.T @ tp @ A
        return K, tp
    Pi = solve_discrete_are(A, B, Q, R)
    return -np.linalg.inv(B.T @ Pi @ B + R) @ B.T @ Pi @ A, Pi


def design_pair(A, B, rate):
    if not rate:
        return A, B
    nx, nu = B.shape
    return np.block([[A, B], [np.zeros((nu, nx)), np.eye(nu)]]), np.block([[B], [np.eye(nu)]])


def riccati_residual(A, B, Q, R, P):
    """max |Q + A'PA - A'PB (R + B'PB)^-1 B'PA - P| / max |P| in design size"""
    S = R + B.T @ P @ B
    res = Q + A.T @ P @ A - A.T @ P @ B @ np.linalg.solve(S, B.T @ P @ A) - P
    return float(np.max(np.abs(res)) / np.max(np.abs(P)))


def twin_jacobians(model, x, u, tvp=(), p=()):
    """(A, B) = d rhs / d (x, u) by sym.jacobian on the model's own expressions, noise zero"""
    if getattr(model, "_twin_lin", None) is None:
        ins = [model._x.cat, model._u.cat, model._tvp.cat, model._p.cat, model._w.cat, model._v.cat]
        model._twin_lin = (sym.Function("A", ins, [sym.jacobian(model._rhs, model._x.cat)]),
                           sym.Function("B", ins, [sym.jacobian(model._rhs, model._u.cat)]))
    args = (np.asarray(x, float).ravel(), np.asarray(u, float).ravel(), np.asarray(tvp, float).ravel(), np.asarray(p, float).ravel(),
            np.zeros(model.n_w), np.zeros(model.n_v))
    fa, fb = model._twin_lin
    return (np.asarray(fa.eval(*args)[0], float).reshape((model.n_x, model.n_x), order="F"),
            np.asarray(fb.eval(*args)[0], float).reshape((model.n_x, model.n_u), order="F"))


def twin_zoh(A, B, dt):
    nx, nu = B.shape
    Ad, Bd, *_ = cont2discrete((A, B, np.eye(nx), np.zeros((nx, nu))), dt, "zoh")
    return Ad, Bd


# ---------------------------------------------------------------------------------------------- the two examples
def example(name, hostemu, n_horizon="example", rate=True):
    """(example module, nonlinear or linear plant model, controller) of a shipped example, set up"""
    ex = CASES[name]
    plant = ex.build_model()
    linear = ex.build_linear_model(plant) if name == "cstr_lqr" else plant
    kw = {} if n_horizon == "example" else {"n_horizon": n_horizon}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        lqr = ex.build_lqr(linear, setup=False, rate=rate, **kw)
    return ex, plant, setup_lqr(lqr, hostemu)


def example_weights(ex):
    if ex is CASES["cstr_lqr"]:
        return ex.Q, ex.R, ex.R_DELTA
    return np.identity(4), np.identity(1), np.identity(1)


def replay(name, hostemu, abstol=None):
    """the closed loop of the example's main.py -> (largest relerr of simulator._x, of simulator._u against the stored run)"""
    ex, plant, lqr = example(name, hostemu)
    sim = ex.build_simulator(plant, setup=False)
    if abstol is not None:
        sim.set_param(abstol=abstol, reltol=abstol)
    plant_on(sim, hostemu)
    x0 = ex.X0.reshape(-1, 1)
    sim.x0 = x0
    if name == "cstr_lqr":
        lqr.set_setpoint(xss=ex.XSS, uss=ex.USS)
    for _ in range(ex.N_STEPS):
        u0 = lqr.make_step(x0)
        x0 = sim.make_step(u0)
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    ex_, eu_ = relerr(sim.data["_x"], g["simulator._x"]), relerr(sim.data["_u"], g["simulator._u"])
    print(f"{name}: {ex.N_STEPS} steps, relerr _x = {ex_:.3e}, _u = {eu_:.3e}")
    return ex_, eu_


# ---------------------------------------------------------------------------------------------- random families (default_rng(2026))
def family_a(B=4096):
    """random continuous systems, discretised by zero-order hold with scipy: list of (Ad, Bd, Q, R) grouped by (n, nu)"""
    rng = np.random.default_rng(2026)
    out = []
    for _ in range(B):
        n = int(rng.integers(2, 13))
        nu = int(rng.integers(1, min(n, 4) + 1))
        Ac = rng.standard_normal((n, n)) / np.sqrt(n)
        Bc = rng.standard_normal((n, nu))
        dt = float(rng.uniform(0.1, 0.5))
        Q = np.diag(10.0 ** rng.uniform(-1, 1, n))
        R = np.diag(10.0 ** rng.uniform(-1, 1, nu))
        Ad, Bd = twin_zoh(Ac, Bc, dt)
        out.append((Ad, Bd, Q, R))
    return out


def embed(members, n=12, nu=4):
    """members of family (a) of every size in ONE launch of the (n, nu) = (12, 4) design: a system of n' < n states is completed by
    n - n' decoupled states x+ = 0.5 x with unit weight and no input, a system with nu' < nu inputs by inputs without effect and with
    unit weight.  The Riccati solution is block diagonal and K of the original system is the top left block of the embedded one."""
    Bn = len(members)
    A = np.zeros((Bn, n, n)); Bm = np.zeros((Bn, n, nu)); Q = np.zeros((Bn, n, n)); R = np.zeros((Bn, nu, nu))
    for b, (Ad, Bd, Qb, Rb) in enumerate(members):
        k, ku = Bd.shape
        A[b] = 0.5 * np.eye(n); A[b, :k, :k] = Ad
        Bm[b, :k, :ku] = Bd
        Q[b] = np.eye(n); Q[b, :k, :k] = Qb
        R[b] = np.eye(nu); R[b, :ku, :ku] = Rb
    return A, Bm, Q, R


def model_free_lqr(nx, nu, hostemu, rate=False, n_horizon=None):
    """controller on a placeholder discrete LinearModel of the given size: gains_batch takes the systems themselves"""
    m = LinearModel("discrete")
    m.set_variable("_x", "x", (nx, 1))
    m.set_variable("_u", "u", (nu, 1))
    m.setup(0.5 * np.eye(nx), np.eye(nx, nu))
    lqr = LQR(m)
    lqr.settings.t_step = 1.0
    lqr.settings.n_horizon = n_horizon
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        lqr.set_objective(Q=np.eye(nx), R=np.eye(nu))
    if rate:
        lqr.set_rterm(delR=np.eye(nu))
    return setup_lqr(lqr, hostemu)


def family_b_points(ex, B=1024):
    rng = np.random.default_rng(2026)
    X = ex.XSS.ravel()[None, :] * (1.0 + 0.02 * rng.uniform(-1, 1, (B, 4)))
    U = ex.USS.ravel()[None, :] * (1.0 + 0.02 * rng.uniform(-1, 1, (B, 2)))
    return X, U


# ---------------------------------------------------------------------------------------------- shared checks (CPU: host emulation, GPU: HIP)
# Bounds: ten times the worst value MEASURED ON THE HOST EMULATION against the twin (the factor covers fused against unfused rounding
# between the emulation and the device); the measured values are in the docstrings of tests/test_lqr.py and in DESIGN.md 4j.
K_BOUND_EXAMPLES = 1.8e-9           # measured 1.72e-10 (cstr_lqr, standard mode, infinite horizon)
RES_MARGIN_EXAMPLES = 2.1e-10       # measured 2.04e-11 (cstr_lqr, standard mode, infinite horizon: kernel 2.054e-11, scipy 9.9e-14)
K_BOUND_16, RES_MARGIN_16 = 3.9e-11, 1.8e-12    # measured 3.90e-12 and 1.72e-13 (both in standard mode) over the designs of size 16
K_BOUND_A, RES_MARGIN_A = 1.7e-7, 1.7e-8        # measured 1.64e-8 (member 1747: scipy's residual 7.6e-11, the kernel's 9.9e-13) and 1.66e-9
K_BOUND_B, RES_MARGIN_B, AB_BOUND_B = 4.9e-9, 6.7e-14, 3.6e-12      # measured 4.82e-10, 6.65e-15 and 3.51e-13
AB_BOUND_MIXED = 6.0e-12           # measured 5.97e-13 (check_mixed_squarings: 9 .. 13 squarings, |B_d| up to 2.1e3); K 1.30e-10 and residual 5.6e-16 stay under the bounds of family (b)
SCIPY_RESIDUAL = 1e-10            # a member is compared only when scipy's own solution is that good
LEFT_OUT = 0.05


def check_example_gains(name, rate, n_horizon, hostemu):
    ex, plant, lqr = example(name, hostemu, n_horizon=n_horizon, rate=rate)
    Q, R, dR = example_weights(ex)
    A, B = lqr.model._A, lqr.model._B
    Kt, Pt = twin_design(A, B, Q, R, n_horizon=n_horizon, rate=rate, delR=dR)
    eK = relerr(lqr.K, Kt)
    msg = f"{name} {'rate' if rate else 'standard'} n_horizon={n_horizon}: K - twin = {eK:.3e}, steps = {lqr.design_iters}"
    assert lqr.design_status == 0 and lqr.K.shape == Kt.shape
    if n_horizon is None:
        At, Bt = design_pair(A, B, rate)
        Qt, Rt = (np.block([[Q, np.zeros((Q.shape[0], R.shape[0]))], [np.zeros((R.shape[0], Q.shape[0])), R]]), dR) if rate else (Q, R)
        rk, rs = riccati_residual(At, Bt, Qt, Rt, lqr.P_riccati), riccati_residual(At, Bt, Qt, Rt, Pt)
        msg += f", Riccati residual kernel {rk:.3e} scipy {rs:.3e}"
        print(msg)
        assert rk <= rs + RES_MARGIN_EXAMPLES
    else:
        assert lqr.design_iters == n_horizon
        print(msg)
    assert eK < K_BOUND_EXAMPLES


def check_family_a(hostemu):
    mem = family_a()
    A, B, Q, R = embed(mem)
    lqr = model_free_lqr(12, 4, hostemu)
    r = lqr.gains_batch(A, B, Q, R)
    assert np.all(r["status"] == 0), np.bincount(r["status"])        # (a status is a failure, not a member left out)
    assert np.all(np.isfinite(r["K"])) and np.all(np.isfinite(r["P"]))
    left, worst_k, worst_excess, ratios = 0, 0.0, 0.0, []
    for b, (Ad, Bd, Qb, Rb) in enumerate(mem):
        k, ku = Bd.shape
        Ps = solve_discrete_are(Ad, Bd, Qb, Rb)
        rs = riccati_residual(Ad, Bd, Qb, Rb, Ps)
        if not rs <= SCIPY_RESIDUAL:
            left += 1
            continue
        Ks = -np.linalg.inv(Bd.T @ Ps @ Bd + Rb) @ Bd.T @ Ps @ Ad
        worst_k = max(worst_k, relerr(r["K"][b, :ku, :k], Ks))
        rk = riccati_residual(Ad, Bd, Qb, Rb, r["P"][b, :k, :k])
        worst_excess = max(worst_excess, rk - rs)
        ratios.append(rk / rs)
        # (the completion of the system is decoupled: nothing of it reaches the gain of the system)
        assert np.max(np.abs(r["K"][b, ku:, :]), initial=0.0) < 1e-12 and np.max(np.abs(r["K"][b, :, k:]), initial=0.0) < 1e-12
    print(f"family (a): {len(mem)} members, {left} left out by scipy's residual, K - scipy = {worst_k:.3e} (bound {K_BOUND_A:.1e}), "
          f"residual kernel - scipy = {worst_excess:.3e} (margin {RES_MARGIN_A:.1e}), median kernel / scipy = {np.median(ratios):.3f}, "
          f"doubling steps <= {int(r['iters'].max())}")
    assert left <= LEFT_OUT * len(mem)
    assert worst_k < K_BOUND_A and worst_excess <= RES_MARGIN_A


def size_16_cases(rate, Bn=6):
    """six random systems (not a multiple of 4) drawn like family (a) at the largest design size: (16, 4) in standard mode, (12, 4)
    in inputRatePenalization mode -> A, B [Bn][nx][..], diagonal model-size Q, R and delR"""
    rng = np.random.default_rng(2026 + int(rate))
    n, nu = (12, 4) if rate else (16, 4)
    A = np.empty((Bn, n, n)); Bm = np.empty((Bn, n, nu))
    for b in range(Bn):
        A[b], Bm[b] = twin_zoh(rng.standard_normal((n, n)) / np.sqrt(n), rng.standard_normal((n, nu)), float(rng.uniform(0.1, 0.5)))
    Q = np.diag(10.0 ** rng.uniform(-1, 1, n))
    R = np.diag(10.0 ** rng.uniform(-1, 1, nu))
    dR = np.diag(10.0 ** rng.uniform(-1, 1, nu))
    return A, Bm, Q, R, dR


def check_size_16(rate, hostemu):
    """N = 16, the largest design the kernel maps (every lane of a row owns a matrix row), in both modes, against scipy"""
    A, Bm, Q, R, dR = size_16_cases(rate)
    n, nu = Bm.shape[1:]
    lqr = model_free_lqr(n, nu, hostemu, rate=rate)
    assert lqr.n_design == 16
    lqr.delR = dR
    r = lqr.gains_batch(A, Bm, Q, R)
    assert np.all(r["status"] == 0), r["status"]
    Qt, Rt = (np.block([[Q, np.zeros((n, nu))], [np.zeros((nu, n)), R]]), dR) if rate else (Q, R)
    kept, worst_k, worst_excess = 0, 0.0, 0.0
    for b in range(len(A)):
        Kt, Pt = twin_design(A[b], Bm[b], Q, R, rate=rate, delR=dR)
        At, Bt = design_pair(A[b], Bm[b], rate)
        rs = riccati_residual(At, Bt, Qt, Rt, Pt)
        if not rs <= SCIPY_RESIDUAL:
            continue
        kept += 1
        worst_k = max(worst_k, relerr(r["K"][b], Kt))
        worst_excess = max(worst_excess, riccati_residual(At, Bt, Qt, Rt, r["P"][b]) - rs)
    print(f"N = 16 {'rate' if rate else 'standard'}: {kept} of {len(A)} kept, K - scipy = {worst_k:.3e} (bound {K_BOUND_16:.1e}), "
          f"residual kernel - scipy = {worst_excess:.3e} (margin {RES_MARGIN_16:.1e}), doubling steps <= {int(r['iters'].max())}")
    assert kept >= len(A) - 1          # (scipy's own residual leaves out 3.6 % of such systems: at most one of six here)
    assert worst_k < K_BOUND_16 and worst_excess <= RES_MARGIN_16


def check_family_b(hostemu):
    ex, plant, lqr = example("cstr_lqr", hostemu, n_horizon=None)
    X, U = family_b_points(ex)
    r = lqr.gains_at(plant, X, U)
    assert np.all(r["status"] == 0), np.bincount(r["status"])
    Q, R, dR = example_weights(ex)
    Qt = np.block([[Q, np.zeros((4, 2))], [np.zeros((2, 4)), R]])
    left, worst_k, worst_ab, worst_excess = 0, 0.0, 0.0, 0.0
    for b in range(len(X)):
        Ac, Bc = twin_jacobians(plant, X[b], U[b])
        Ad, Bd = twin_zoh(Ac, Bc, ex.T_STEP)
        worst_ab = max(worst_ab, relerr(r["A"][b], Ad), relerr(r["B"][b], Bd))
        Kt, Pt = twin_design(Ad, Bd, Q, R, rate=True, delR=dR)
        At, Bt = design_pair(Ad, Bd, True)
        rs = riccati_residual(At, Bt, Qt, dR, Pt)
        if not rs <= SCIPY_RESIDUAL:
            left += 1
            continue
        worst_k = max(worst_k, relerr(r["K"][b], Kt))
        worst_excess = max(worst_excess, riccati_residual(At, Bt, Qt, dR, r["P"][b]) - rs)
    print(f"family (b): {len(X)} operating points, {left} left out, K - twin = {worst_k:.3e} (bound {K_BOUND_B:.1e}), discrete pair - "
          f"cont2discrete = {worst_ab:.3e} (bound {AB_BOUND_B:.1e}), residual kernel - scipy = {worst_excess:.3e} (margin {RES_MARGIN_B:.1e})")
    assert left <= LEFT_OUT * len(X)
    assert worst_k < K_BOUND_B and worst_ab < AB_BOUND_B and worst_excess <= RES_MARGIN_B


def status_cases(hostemu):
    """seven designs of size (3, 1) in two wavefronts (not a multiple of 4): good ones around an uncontrollable unstable pair (slot 1)
    and one with R = 0 and B'PB singular (slot 5, per-member weights)"""
    rng = np.random.default_rng(7)
    Bn = 7
    A = 0.6 * rng.standard_normal((Bn, 3, 3))
    Bm = rng.standard_normal((Bn, 3, 1))
    A[1] = np.diag([1.5, 0.5, 0.3]); Bm[1] = [[0.0], [1.0], [1.0]]          # the unstable mode is not reached by the input
    Bm[5] = 0.0                                                                # B = 0: B'PB = 0, with R = 0 singular
    Q = np.tile(np.eye(3), (Bn, 1, 1))
    R = np.tile(np.eye(1), (Bn, 1, 1))
    R[5] = 0.0
    return model_free_lqr(3, 1, hostemu), A, Bm, Q, R


def check_status(hostemu):
    lqr, A, Bm, Q, R = status_cases(hostemu)
    r = lqr.gains_batch(A, Bm, Q, R)
    print("status:", r["status"], "steps:", r["iters"])
    assert r["status"][1] & 1 and r["status"][5] & 2
    assert np.all(np.isfinite(r["K"])) and np.all(np.isfinite(r["P"]))
    assert np.array_equal(r["K"][5], np.zeros((1, 3))) and np.array_equal(r["P"][5], Q[5])
    good = [0, 2, 3, 4, 6]
    assert np.all(r["status"][good] == 0)
    for b in good:                                      # the neighbours: what the single design gives, and what scipy gives
        one = lqr.gains_batch(A[b:b + 1], Bm[b:b + 1], Q[b:b + 1], R[b:b + 1])
        assert np.array_equal(one["K"][0], r["K"][b]) and np.array_equal(one["P"][0], r["P"][b]) and one["status"][0] == 0
        Kt, _ = twin_design(A[b], Bm[b], Q[b], R[b])
        assert relerr(r["K"][b], Kt) < K_BOUND_A
    # shared weights = the same weights per member
    sh = lqr.gains_batch(A[good], Bm[good], Q[0], R[0])
    pm = lqr.gains_batch(A[good], Bm[good], Q[good], R[good])
    assert np.array_equal(sh["K"], pm["K"]) and np.array_equal(sh["P"], pm["P"]) and np.array_equal(sh["K"], r["K"][good])


def check_closed_loop_copies(name, hostemu, B=5):
    """B copies of one x0 in BatchClosedLoopLQR = the single-controller loop of the example, member for member"""
    from do_mpc_amd.closed_loop import BatchClosedLoopLQR
    ex, plant, lqr = example(name, hostemu)
    sim = plant_on(ex.build_simulator(plant, setup=False), hostemu)
    if name == "cstr_lqr":
        lqr.set_setpoint(xss=ex.XSS, uss=ex.USS)
    n = 20
    loop = BatchClosedLoopLQR(lqr, sim, np.tile(ex.X0, (B, 1)), device="cpu" if hostemu else 0)
    rec = loop.run(n)
    assert np.all(rec["plant_status"] == 0)
    x0 = ex.X0.reshape(-1, 1)
    sim.x0 = x0
    for _ in range(n):
        x0 = sim.make_step(lqr.make_step(x0))
    ex_ = max(relerr(rec["x"][:-1, b], sim.data["_x"]) for b in range(B))
    eu_ = max(relerr(rec["u"][:, b], sim.data["_u"]) for b in range(B))
    print(f"{name}: {B} copies over {n} steps, batch - single loop: _x {ex_:.3e}, _u {eu_:.3e}")
    # the same gain and the same plant kernel: the difference is the order of the additions in K (x - xss) (numpy against torch)
    assert ex_ < 1e-12 and eu_ < 1e-12
    assert np.array_equal(rec["x"][:, 0], rec["x"][:, B - 1])


def check_closed_loop_schedule(hostemu, B=6, n=10):
    """per-member gains from gains_at at B operating points = a Python loop over the members (one controller call and one plant call
    per member and step)"""
    from do_mpc_amd.closed_loop import BatchClosedLoopLQR
    ex, plant, lqr = example("cstr_lqr", hostemu)
    sim = plant_on(ex.build_simulator(plant, setup=False), hostemu)
    X, U = family_b_points(ex, B)
    g = lqr.gains_at(plant, X, U)
    assert np.all(g["status"] == 0)
    X0 = X * (1.0 + 0.01 * np.random.default_rng(3).uniform(-1, 1, X.shape))
    rec = BatchClosedLoopLQR(lqr, sim, X0, K=g["K"], XSS=X, USS=U, device="cpu" if hostemu else 0, U_prev0=U).run(n)
    worst = 0.0
    for b in range(B):
        x, up = X0[b:b + 1].copy(), U[b:b + 1].copy()
        for k in range(n):
            u = lqr.make_step_batch(x, K=g["K"][b], XSS=X[b], USS=U[b], U_prev=up)
            worst = max(worst, relerr(rec["u"][k, b], u[0]), relerr(rec["x"][k, b], x[0]))
            x, up = sim.make_step_batch(x, U=u[0])["x"], u
    print(f"schedule of {B} gains over {n} steps: batch - loop over members = {worst:.3e}")
    assert worst < 1e-12


def kernel_metadata(code_object, tmp_dir, kernel="dompc_lqr_kernel"):
    """(private segment bytes, spilled VGPRs) of `kernel` from the code object's amdhsa metadata; None without llvm-readelf"""
    import shutil
    import struct
    import subprocess
    from do_mpc_amd import build
    tool = None
    for cand in (shutil.which("llvm-readelf"), os.path.join(os.path.dirname(os.path.realpath(build._hipcc())), "..", "llvm", "bin", "llvm-readelf"),
                 "/opt/rocm/llvm/bin/llvm-readelf"):
        if cand and os.path.exists(cand):
            tool = cand
            break
    if tool is None:
        return None
    raw = open(code_object, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    if raw.startswith(magic):                      # hipcc --genco wraps the ELF in an offload bundle: take the gfx950 entry out
        pos, elf = len(magic) + 8, None
        for _ in range(struct.unpack_from("<Q", raw, len(magic))[0]):
            off, size, tlen = struct.unpack_from("<QQQ", raw, pos)
            triple = raw[pos + 24:pos + 24 + tlen].decode()
            pos += 24 + tlen
            if "gfx950" in triple:
                elf = raw[off:off + size]
        assert elf is not None, "no gfx950 entry in the code object"
        code_object = str(tmp_dir / "kernel.elf")
        with open(code_object, "wb") as f:
            f.write(elf)
    notes = subprocess.run([tool, "--notes", code_object], stdout=subprocess.PIPE, text=True, check=True).stdout
    blk = next(b for b in notes.split("- .agpr_count") if f".name: {kernel}" in " ".join(b.split()))
    field = lambda k: int(next(l for l in blk.splitlines() if l.strip().startswith(k)).split(":")[1])      # noqa: E731
    return field(".private_segment_fixed_size"), field(".vgpr_spill_count")


# ---------------------------------------------------------------------------------------------- zero-order hold: unequal designs in one wavefront
# On the device the squaring loop of expm runs to the largest s of the wavefront (wave_any(q < s)) and a design that is through keeps
# its T by select.  The host emulation runs one group at a time; "bit for bit against single-member calls" is the point of the GPU twin.
def mixed_squarings_points(ex):
    """16 operating points of the CSTR: T_R = 340 .. 440 K, T_J = T_R - 1, F scaled by 0.5 .. 8"""
    X, U = np.tile(ex.XSS.ravel(), (16, 1)), np.tile(ex.USS.ravel(), (16, 1))
    X[:, 2] = np.linspace(340.0, 440.0, 16)
    X[:, 3] = X[:, 2] - 1.0
    U[:, 0] *= np.linspace(0.5, 8.0, 16)
    return X, U


def squarings(plant, x, u, dt):
    """s of csrc/dompc_lqr.hip expm for E = [[A, B], [0, 0]] dt, with numpy's 1-norm"""
    Ac, Bc = twin_jacobians(plant, x, u)
    n = np.linalg.norm(np.block([[Ac, Bc], [np.zeros((Bc.shape[1], sum(Bc.shape)))]]) * dt, 1)
    return int(np.floor(np.log2(n))) + 2 if n > 0.5 else 0


def _members_equal_single_calls(lqr, plant, X, U, r):
    for b in range(len(X)):
        one = lqr.gains_at(plant, X[b:b + 1], U[b:b + 1])
        for k in ("K", "P", "A", "B", "status", "iters"):
            assert np.array_equal(one[k][0], r[k][b]), (b, k)


def check_mixed_squarings(hostemu, members=None):
    """gains_at at mixed_squarings_points (members: a sub-batch in that order): the squarings differ inside every group of four
    (asserted on the CPU), the pair against twin_zoh, K against twin_design by the rule of check_family_b, every member bit for bit
    against its single-member call"""
    ex, plant, lqr = example("cstr_lqr", hostemu, n_horizon=None)
    X, U = mixed_squarings_points(ex)
    if members is not None:
        X, U = X[members], U[members]
    Bn = len(X)
    s = [squarings(plant, X[b], U[b], ex.T_STEP) for b in range(Bn)]
    groups = [s[g:g + 4] for g in range(0, Bn, 4)]
    assert all(len(set(g)) >= 2 for g in groups if len(g) > 1) and len(set(s)) >= 4, s
    assert s[-1] == max(s)                                 # (the design the idle groups of a partial wavefront repeat is the slowest)
    r = lqr.gains_at(plant, X, U)
    assert np.all(r["status"] == 0), r["status"]
    Q, R, dR = example_weights(ex)
    Qt = np.block([[Q, np.zeros((4, 2))], [np.zeros((2, 4)), R]])
    left, worst_k, worst_ab, worst_excess, bmax = 0, 0.0, 0.0, 0.0, 0.0
    for b in range(Bn):
        Ac, Bc = twin_jacobians(plant, X[b], U[b])
        Ad, Bd = twin_zoh(Ac, Bc, ex.T_STEP)
        worst_ab, bmax = max(worst_ab, relerr(r["A"][b], Ad), relerr(r["B"][b], Bd)), max(bmax, float(np.max(np.abs(Bd))))
        Kt, Pt = twin_design(Ad, Bd, Q, R, rate=True, delR=dR)
        At, Bt = design_pair(Ad, Bd, True)
        rs = riccati_residual(At, Bt, Qt, dR, Pt)
        if not rs <= SCIPY_RESIDUAL:
            left += 1
            continue
        worst_k = max(worst_k, relerr(r["K"][b], Kt))
        worst_excess = max(worst_excess, riccati_residual(At, Bt, Qt, dR, r["P"][b]) - rs)
    print(f"mixed squarings {s}: {Bn} designs, {left} left out, K - twin = {worst_k:.3e} (bound {K_BOUND_B:.1e}), discrete pair - cont2discrete "
          f"= {worst_ab:.3e} (bound {AB_BOUND_MIXED:.1e}, max |B_d| = {bmax:.1e}), residual kernel - scipy = {worst_excess:.3e} "
          f"(margin {RES_MARGIN_B:.1e}), doubling steps {r['iters']}")
    assert left <= LEFT_OUT * Bn
    assert worst_k < K_BOUND_B and worst_ab < AB_BOUND_MIXED and worst_excess <= RES_MARGIN_B
    _members_equal_single_calls(lqr, plant, X, U, r)


def check_failed_exponential(hostemu):
    """B = 7 with T_R = NaN (a norm that is not finite), -300 (finite, more than 60 squarings) and -1 (the Arrhenius terms overflow)
    in slots 1, 3 and 6 among good members.  Pinned as observed: a failed hold reports bits 0 and 1, runs max_iter doubling steps
    (which its wavefront shares), hands out K = 0, P = Q, A = I, B = 0 and nothing that is not finite; the good members are bit-equal
    to a call without the failed ones and to their single calls"""
    ex, plant, lqr = example("cstr_lqr", hostemu, n_horizon=None)
    X, U = mixed_squarings_points(ex)
    X, U = X[[0, 3, 5, 7, 9, 12, 15]], U[[0, 3, 5, 7, 9, 12, 15]]
    bad, good = [1, 3, 6], [0, 2, 4, 5]
    X[bad, 2] = [np.nan, -300.0, -1.0]
    r = lqr.gains_at(plant, X, U)
    print(f"failed exponentials in slots {bad}: status {r['status']}, doubling steps {r['iters']}")
    for k in ("K", "P", "A", "B"):
        assert np.all(np.isfinite(r[k])), k
    Q, R, _ = example_weights(ex)
    Qt = np.block([[Q, np.zeros((4, 2))], [np.zeros((2, 4)), R]])
    for b in bad:
        assert r["status"][b] == 3 and r["iters"][b] == lqr.settings.max_iter == 50, (b, r["status"][b], r["iters"][b])
        assert not r["K"][b].any() and np.array_equal(r["P"][b], Qt)
        assert np.array_equal(r["A"][b], np.eye(4)) and not r["B"][b].any()
    assert np.all(r["status"][good] == 0)
    alone = lqr.gains_at(plant, X[good], U[good])
    for k in ("K", "P", "A", "B", "status", "iters"):
        assert np.array_equal(alone[k], r[k][good]), k
    _members_equal_single_calls(lqr, plant, X, U, r)
