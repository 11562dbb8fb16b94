"""TEST-ONLY checks of the time-varying LQR (csrc/dompc_lqr.hip: dompc_lqr_pairs_kernel, dompc_lqr_tv_kernel; LQR.gains_tv_batch,
LQR.gains_along and their device entries), of the law record per step in the general plant rollout (Simulator.rollout_device with
law_step) and of closed_loop.BatchClosedLoopTVLQR, shared by the CPU suite (host emulation) and the GPU suite - each check with a
`hostemu=` switch.  The numpy twin is the recursion of lqr_common.twin_design with a pair per pass."""
import ctypes as C
import warnings

import numpy as np
import torch

import lqr_common as lc
import lqr_dae_common as ldc
import plant_family_common as pf
import rollout_common as rc
from asmpc_hostemu import asmpc_hostemu_library
from do_mpc_amd import sym
from do_mpc_amd.asmpc import AffineLaw
from do_mpc_amd.closed_loop import BatchClosedLoopTVLQR
from do_mpc_amd.examples import CASES, cstr_tracking
from do_mpc_amd.model import Model
from do_mpc_amd.simulator import RolloutDesc
from rollout_common import Dev, h, p, same


# ---------------------------------------------------------------------------------------------- the twin
def _solve(S, rhs):
    """S^-1 rhs by Gaussian elimination with partial pivoting in the dtype of S (np.linalg has no longdouble)"""
    S, rhs = S.copy(), rhs.copy()
    n = S.shape[0]
    for k in range(n):
        piv = k + int(np.argmax(np.abs(S[k:, k])))
        if piv != k:
            S[[k, piv]], rhs[[k, piv]] = S[[piv, k]], rhs[[piv, k]]
        for r in range(k + 1, n):
            f = S[r, k] / S[k, k]
            S[r, k:] -= f * S[k, k:]
            rhs[r] -= f * rhs[k]
    for k in range(n - 1, -1, -1):
        rhs[k] = (rhs[k] - S[k, k + 1:] @ rhs[k + 1:]) / S[k, k]
    return rhs


def twin_tv(A, B, Q, R, Pf, rate=False, dtype=np.float64):
    """one trajectory: A [K][nx][nx], B [K][nx][nu] model size, Q, R, Pf DESIGN size -> (K [K][nu][n], P [K+1][n][n]); per pass the
    formulas of lqr_common.twin_design: K = -(B'PB + R)^-1 B'PA, P <- Q + A'PA - A'PB (B'PB + R)^-1 B'PA"""
    K_ = A.shape[0]
    Q, R, P = (np.asarray(a, dtype=dtype) for a in (Q, R, Pf))
    n, nu = Q.shape[0], R.shape[0]
    Ks, Ps = np.zeros((K_, nu, n), dtype=dtype), np.zeros((K_ + 1, n, n), dtype=dtype)
    Ps[K_] = P
    for k in range(K_ - 1, -1, -1):
        Ak, Bk = (np.asarray(a, dtype=dtype) for a in lc.design_pair(A[k], B[k], rate))
        BPA = Bk.T @ P @ Ak
        Kk = -_solve(Bk.T @ P @ Bk + R, BPA)
        P = Q + Ak.T @ P @ Ak + BPA.T @ Kk
        Ks[k], Ps[k] = Kk, P
    return Ks, Ps


def nerr(a, ref):
    """largest difference relative to max(1, max |ref|) (norm-wise: entries of a gain that are zero by structure carry no scale)"""
    a, ref = np.asarray(a, np.longdouble), np.asarray(ref, np.longdouble)
    return float(np.max(np.abs(a - ref)) / max(1.0, float(np.max(np.abs(ref))))) if a.size else 0.0


def spread(A, B, Q, R, Pf, rate):
    """the twin's own rounding: max over K, P of |twin in float64 - twin in numpy longdouble| (nerr), for a batch [K][Bn][..]"""
    worst = 0.0
    for b in range(A.shape[1]):
        Qb, Rb, Pb = (w if w.ndim == 2 else w[b] for w in (Q, R, Pf))
        K64, P64 = twin_tv(A[:, b], B[:, b], Qb, Rb, Pb, rate)
        Kld, Pld = twin_tv(A[:, b], B[:, b], Qb, Rb, Pb, rate, dtype=np.longdouble)
        assert np.all(np.isfinite(K64)) and np.all(np.isfinite(P64))               # (no member may be left out: the twin is finite)
        worst = max(worst, nerr(K64, Kld), nerr(P64, Pld))
    return worst


def bound_of(spread_, n):
    """16 times the twin's rounding spread (the kernel eliminates by Gauss-Jordan with another pivot order and contracts to fma),
    with a relative floor of 64 n 2^-53"""
    return max(16.0 * spread_, 64.0 * n * 2.0 ** -53)


# The twin's rounding spread per family of check_random_pairs, MEASURED on the CPU (x86-64: numpy longdouble is the 80-bit format),
# and the bound that follows from it by bound_of; test_lqr_tv.py asserts that the spread measured now is the one written here, and
# prints what the host emulation reaches.  (mode, K, weights) -> spread; n = 12 standard, 16 rate.
SPREAD = {
    ('standard', 1, 'per'): 5.192e-16,      # bound 8.527e-14 (the floor); host emulation - twin measured 4.019e-16
    ('standard', 1, 'shared'): 6.417e-16,   # bound 8.527e-14 (the floor); 3.559e-16
    ('standard', 4, 'per'): 2.254e-15,      # bound 8.527e-14 (the floor); 3.692e-15
    ('standard', 4, 'shared'): 5.868e-16,   # bound 8.527e-14 (the floor); 8.024e-16
    ('standard', 20, 'per'): 7.379e-15,     # bound 1.181e-13; 7.508e-15
    ('standard', 20, 'shared'): 1.992e-15,  # bound 8.527e-14 (the floor); 3.104e-15
    ('rate', 1, 'per'): 3.405e-16,          # bound 1.137e-13 (the floor); 3.331e-16
    ('rate', 1, 'shared'): 3.111e-16,       # bound 1.137e-13 (the floor); 3.331e-16
    ('rate', 4, 'per'): 1.225e-15,          # bound 1.137e-13 (the floor); 2.346e-15
    ('rate', 4, 'shared'): 8.495e-16,       # bound 1.137e-13 (the floor); 1.221e-15
    # 20 random pairs with the integrators of the rate design: the recursion itself is ill-conditioned there - the float64 twin is
    # this far from the longdouble one, and the host emulation's distance to the float64 twin is the twin's own error
    ('rate', 20, 'per'): 5.065e-10,         # bound 8.104e-09; 5.066e-10
    ('rate', 20, 'shared'): 1.205e-10,      # bound 1.928e-09; 1.206e-10
}


def tv_lqr(nx, nu, hostemu, rate=False):
    return lc.model_free_lqr(nx, nu, hostemu, rate=rate)


# ---------------------------------------------------------------------------------------------- 1. constant pair = finite horizon
CONSTANT_DESIGNS = [(3, 1, False), (12, 4, False), (12, 4, True), (16, 4, False)]


def check_constant_pair(nx, nu, rate, K, hostemu, Bn=5):
    """the same (A, B) at every step: K[0] and P0 of gains_tv_batch equal gains_batch with n_horizon = K bit for bit (step order,
    strides, the shared pass body); Bn = 5: two wavefronts, the second with one live row"""
    rng = np.random.default_rng(100 * nx + nu)
    pairs = [lc.twin_zoh(rng.standard_normal((nx, nx)) / np.sqrt(nx), rng.standard_normal((nx, nu)), 0.3) for _ in range(Bn)]
    A, Bm = np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])
    Q = np.stack([np.diag(10.0 ** rng.uniform(-1, 1, nx)) for _ in range(Bn)])
    R = np.stack([np.diag(10.0 ** rng.uniform(-1, 1, nu)) for _ in range(Bn)])
    lqr = lc.model_free_lqr(nx, nu, hostemu, rate=rate, n_horizon=K)
    fin = lqr.gains_batch(A, Bm, Q, R, P=Q)
    tv = lqr.gains_tv_batch(np.tile(A, (K, 1, 1, 1)), np.tile(Bm, (K, 1, 1, 1)), Q, R, P=Q, P_traj=True)
    assert np.all(fin["status"] == 0) and np.all(tv["status"] == 0)
    assert same(tv["K"][0], fin["K"]), "K[0]"
    assert same(tv["P0"], fin["P"]) and same(tv["P"][0], tv["P0"]), "P0"
    if K > 1:                                  # (the gain of step 1 is the finite-horizon gain over K - 1 passes: the steps are in order)
        lqr.settings.n_horizon = K - 1
        assert same(tv["K"][1], lqr.gains_batch(A, Bm, Q, R, P=Q)["K"]), "K[1]"


# ---------------------------------------------------------------------------------------------- 2. random pairs against the twin
def random_pairs(K, Bn=7, nx=12, nu=4, seed=2026):
    """a different pair at every step of every trajectory, each drawn like a member of lqr_common.family_a at (nx, nu)"""
    rng = np.random.default_rng(seed + K)
    A, Bm = np.empty((K, Bn, nx, nx)), np.empty((K, Bn, nx, nu))
    for k in range(K):
        for b in range(Bn):
            A[k, b], Bm[k, b] = lc.twin_zoh(rng.standard_normal((nx, nx)) / np.sqrt(nx), rng.standard_normal((nx, nu)), float(rng.uniform(0.1, 0.5)))
    Q = np.stack([np.diag(10.0 ** rng.uniform(-1, 1, nx)) for _ in range(Bn)])
    R = np.stack([np.diag(10.0 ** rng.uniform(-1, 1, nu)) for _ in range(Bn)])
    dR = np.diag(10.0 ** rng.uniform(-1, 1, nu))
    return A, Bm, Q, R, dR


def design_weights(Q, R, dR, rate):
    """model-size Q, R (one or a batch) -> design-size (Q, R, P_f = Q)"""
    if not rate:
        return Q, R, Q
    Qd = np.stack([np.block([[q, np.zeros((q.shape[0], r.shape[0]))], [np.zeros((r.shape[0], q.shape[0])), r]]) for q, r in zip(Q, R)]) \
        if Q.ndim == 3 else np.block([[Q, np.zeros((Q.shape[0], R.shape[0]))], [np.zeros((R.shape[0], Q.shape[0])), R]])
    return Qd, dR, Qd


RANDOM_CASES = [(rate, K, shared) for rate in (False, True) for K in (1, 4, 20) for shared in (False, True)]


def check_random_pairs(rate, K, shared, hostemu, measure=False):
    """gains_tv_batch on random_pairs against the twin: every K_k, P0 and P_traj within bound_of(SPREAD) of the float64 twin.
    measure: return (spread measured now, worst error) without asserting"""
    A, Bm, Q, R, dR = random_pairs(K)
    if shared:
        Q, R = Q[0], R[0]
    Qd, Rd, Pd = design_weights(Q, R, dR, rate)
    lqr = tv_lqr(12, 4, hostemu, rate=rate)
    lqr.delR = dR
    r = lqr.gains_tv_batch(A, Bm, Q, R, P_traj=True)
    assert np.all(r["status"] == 0), r["status"]
    worst = 0.0
    for b in range(A.shape[1]):
        Qb, Rb, Pb = (w if w.ndim == 2 else w[b] for w in (Qd, Rd, Pd))
        Kt, Pt = twin_tv(A[:, b], Bm[:, b], Qb, Rb, Pb, rate)
        worst = max(worst, nerr(r["K"][:, b], Kt), nerr(r["P"][:, b], Pt), nerr(r["P0"][b], Pt[0]))
        assert same(r["P"][0, b], r["P0"][b]) and same(r["P"][K, b], np.ascontiguousarray(Pb))
    key = ("rate" if rate else "standard", K, "shared" if shared else "per")
    if measure:
        return spread(A, Bm, Qd, Rd, Pd, rate), worst
    bound = bound_of(SPREAD[key], 16 if rate else 12)
    print(f"random pairs {key}: kernel - twin = {worst:.3e}, twin spread {SPREAD[key]:.3e}, bound {bound:.3e}")
    assert worst <= bound


# ---------------------------------------------------------------------------------------------- 3. gains_along
def tvp_model():
    """continuous, n_x = 2, n_u = 1, one _tvp d and one _p a, both in the Jacobians"""
    m = Model("continuous")
    x = m.set_variable("_x", "x", (2, 1))
    u = m.set_variable("_u", "u")
    a = m.set_variable("_p", "a")
    d = m.set_variable("_tvp", "d")
    m.set_rhs("x", sym.vertcat(-a * x[0] + d * x[1] * x[1] + u, x[0] - d * x[1] + a * u * x[0]))
    m.setup()
    return m


# designs of this file whose code objects are prebuilt (__graft_entry__.PREBUILT_LQR: ("tv", name, mode)): name -> (builder, rate)
DESIGNS = {"tvp_model": (tvp_model, False)}


def design(name, hostemu):
    build, rate = DESIGNS[name]
    model = build()
    return model, ldc.controller(model, hostemu, rate=rate)


def _along_case(name, hostemu, Bn=5, K=6):
    """-> (model, lqr, X [K][Bn][nx], U [K][Bn][nu], kwargs of gains_along, rate, t_step or None): knots of a short simulated transition"""
    rng = np.random.default_rng(31)
    if name == "cstr_lqr":
        ex, plant, lqr = lc.example("cstr_lqr", hostemu, n_horizon=None, rate=False)
        sim = lc.plant_on(ex.build_simulator(plant, setup=False), hostemu)
        U = np.tile(cstr_tracking.input_sequence(K)[:, None, :], (1, Bn, 1)) * (1.0 + 0.05 * rng.uniform(-1, 1, (K, Bn, 2)))
        X = sim.simulate_batch(cstr_tracking.starts(Bn, seed=5), U)["x"][:K]
        return plant, lqr, X, U, {}, False, ex.T_STEP
    if name == "oscillating_masses_lqr":
        ex, plant, lqr = lc.example("oscillating_masses_lqr", hostemu, n_horizon=None, rate=True)
        sim = lc.plant_on(ex.build_simulator(plant, setup=False), hostemu)
        U = rng.uniform(-1, 1, (K, Bn, 1))
        X = sim.simulate_batch(ex.X0[None, :] * (1.0 + 0.3 * rng.uniform(-1, 1, (Bn, 4))), U)["x"][:K]
        return plant, lqr, X, U, {}, True, None
    if name == "batch_reactor":
        from do_mpc_amd.simulator import Simulator
        model, lqr = ldc.design("batch_reactor", hostemu)
        sim = Simulator(model)
        sim.set_param(t_step=ldc.T_STEP)
        lc.plant_on(sim, hostemu)
        XSS, _ = ldc.steady_states(Bn)
        U = 0.2 * rng.uniform(-1, 1, (K, Bn, 1))
        X = sim.simulate_batch(XSS + 0.2 * rng.uniform(-1, 1, XSS.shape), U)["x"][:K]
        return model, lqr, X, U, {}, False, ldc.T_STEP
    if name.startswith("tvp_model"):
        model, lqr = design("tvp_model", hostemu)
        par = rng.uniform(0.5, 1.5, (Bn, 1))
        tvp = rng.uniform(0.2, 0.8, (K, Bn, 1))
        if name == "tvp_model_shared":                       # [K][ntvp] shared by the trajectories
            tvp = tvp[:, :1].repeat(Bn, axis=1)
        # explicit Euler on the model's own right-hand side: a simulated transition without a plant code object of its own
        X, U = np.empty((K, Bn, 2)), 0.3 * rng.uniform(-1, 1, (K, Bn, 1))
        x = rng.uniform(-0.5, 0.5, (Bn, 2))
        for k in range(K):
            X[k] = x
            a, d, u = par[:, 0], tvp[k, :, 0], U[k, :, 0]
            x = x + 0.1 * np.stack([-a * x[:, 0] + d * x[:, 1] ** 2 + u, x[:, 0] - d * x[:, 1] + a * u * x[:, 0]], axis=1)
        kw = {"TVP": tvp[:, 0] if name == "tvp_model_shared" else tvp, "PAR": par}
        return model, lqr, X, U, kw, False, ldc.T_STEP
    raise KeyError(name)


ALONG_CASES = ["cstr_lqr", "oscillating_masses_lqr", "batch_reactor", "tvp_model_shared", "tvp_model_per_loop"]
# bounds of the discrete pairs: those of lqr_common (family (b): the CSTR; the others are milder)
ALONG_AB_BOUND = lc.AB_BOUND_B


def twin_pair(model, x, u, tvp, par, dt):
    """the discrete pair and z of one knot: twin Jacobians (twin reduction for algebraic states), twin zero-order hold"""
    z = None
    if model.n_z:
        Ac, Bc, z, _, ok = ldc.twin_reduce(model, x, u, np.zeros(model.n_z))
        assert ok
    else:
        Ac, Bc = lc.twin_jacobians(model, x, u, tvp, par)
    return (lc.twin_zoh(Ac, Bc, dt) if model.model_type == "continuous" else (Ac, Bc)) + (z,)


def check_gains_along(name, hostemu, Bn=5, K=6):
    """pairs against twin Jacobians + twin zero-order hold at every knot (bound: ALONG_AB_BOUND), Z against the host Newton solve,
    gains against the twin recursion on the kernel's own pairs (the pairs are compared separately) by the rule of check_random_pairs:
    16 times the twin's rounding spread on these pairs, floor 64 n 2^-53"""
    model, lqr, X, U, kw, rate, dt = _along_case(name, hostemu, Bn, K)
    r = lqr.gains_along(model, X, U, P_traj=True, **kw)
    assert np.all(r["status"] == 0) and np.all(r["pair_status"] == 0), (r["status"], r["pair_status"])
    nx, nu = model.n_x, model.n_u
    wab, wz = 0.0, 0.0
    for k in range(K):
        for b in range(Bn):
            tvp = np.zeros(0) if "TVP" not in kw else (kw["TVP"][k] if kw["TVP"].ndim == 2 else kw["TVP"][k, b])
            par = kw["PAR"][b] if "PAR" in kw else np.zeros(0)
            Ad, Bd, z = twin_pair(model, X[k, b], U[k, b], tvp, par, dt)
            wab = max(wab, lc.relerr(r["A"][k, b], Ad), lc.relerr(r["B"][k, b], Bd))
            if z is not None:
                wz = max(wz, lc.relerr(r["Z"][k, b], z))
    # the weights of the controller in design size
    Qm, Rm = np.asarray(lqr._Q_user, float), np.asarray(lqr._R_user, float)
    Qd, Rd, Pd = design_weights(Qm, Rm, np.asarray(getattr(lqr, "delR", Rm), float), rate)
    sp, worst = spread(r["A"], r["B"], Qd, Rd, Pd, rate), 0.0
    for b in range(Bn):
        Kt, Pt = twin_tv(r["A"][:, b], r["B"][:, b], Qd, Rd, Pd, rate)
        worst = max(worst, nerr(r["K"][:, b], Kt), nerr(r["P"][:, b], Pt), nerr(r["P0"][b], Pt[0]))
    bound = bound_of(sp, nx + (nu if rate else 0))
    print(f"gains_along {name}: pair - twin = {wab:.3e} (bound {ALONG_AB_BOUND:.1e}), Z - host Newton = {wz:.3e}, gains - twin recursion = "
          f"{worst:.3e} (twin spread {sp:.3e}, bound {bound:.3e})")
    assert wab < ALONG_AB_BOUND and wz < ALONG_AB_BOUND and worst <= bound
    return model, lqr, X, U, kw, r


def check_item_decomposition(hostemu, Bn=5, K=6, k1=3, b1=2):
    """every knot the same point but (k1, b1): its pair alone differs, and is the pair gains_at forms at that point"""
    model, lqr, X, U, kw, _, _ = _along_case("cstr_lqr", hostemu, Bn, K)
    Xs, Us = np.tile(X[0, 0], (K, Bn, 1)), np.tile(U[0, 0], (K, Bn, 1))
    Xs[k1, b1], Us[k1, b1] = X[K - 1, Bn - 1], U[K - 1, Bn - 1]
    r = lqr.gains_along(model, Xs, Us)
    one = lqr.gains_at(model, np.stack([X[0, 0], X[K - 1, Bn - 1]]), np.stack([U[0, 0], U[K - 1, Bn - 1]]))
    for k in range(K):
        for b in range(Bn):
            w = 1 if (k, b) == (k1, b1) else 0
            assert same(r["A"][k, b], one["A"][w]) and same(r["B"][k, b], one["B"][w]), (k, b)
    assert not same(one["A"][0], one["A"][1])


# ---------------------------------------------------------------------------------------------- 4. status and neighbours
def check_status_and_neighbours(hostemu, K=6, kb=3):
    """four trajectories in one wavefront: 1 has a NaN in its pair at step kb, 3 has R = 0 and B_kb = 0 (B'PB + R singular there);
    0 and 2 are healthy"""
    rng = np.random.default_rng(11)
    Bn, nx, nu = 4, 3, 1
    A = 0.6 * rng.standard_normal((K, Bn, nx, nx))
    Bm = rng.standard_normal((K, Bn, nx, nu))
    Q = np.tile(np.eye(nx), (Bn, 1, 1))
    R = np.tile(np.eye(nu), (Bn, 1, 1))
    R[3] = 0.0
    lqr = tv_lqr(nx, nu, hostemu)
    clean = lqr.gains_tv_batch(A, Bm, Q, R, P_traj=True)
    assert np.all(clean["status"] == 0)
    Ab, Bb = A.copy(), Bm.copy()
    Ab[kb, 1, 1, 2] = np.nan
    Bb[kb, 3] = 0.0
    r = lqr.gains_tv_batch(Ab, Bb, Q, R, P_traj=True)
    print("status:", r["status"], "step:", r["step"])
    for key in ("K", "P0", "P"):
        assert np.all(np.isfinite(r[key])), key
    assert r["status"][1] == 4 and r["status"][3] == 2 and r["step"][1] == kb and r["step"][3] == kb
    assert r["status"][0] == 0 and r["status"][2] == 0
    for b in (1, 3):
        assert not r["K"][:kb + 1, b].any(), "K_j = 0 for j <= k"
        assert same(r["K"][kb + 1:, b], clean["K"][kb + 1:, b]), "the gains behind the failing step are those of a clean run"
        assert same(r["P"][kb + 1:, b], clean["P"][kb + 1:, b])
        assert same(r["P0"][b], Q[b])
    for b in (0, 2):                         # the healthy neighbours: their stand-alone runs, bit for bit
        one = lqr.gains_tv_batch(Ab[:, b:b + 1], Bb[:, b:b + 1], Q[b:b + 1], R[b:b + 1], P_traj=True)
        assert one["status"][0] == 0
        for key in ("K", "P"):
            assert same(one[key][:, 0], r[key][:, b]), (b, key)
        assert same(one["P0"][0], r["P0"][b])
        assert same(r["K"][:, b], clean["K"][:, b])


def check_failed_knot(hostemu, Bn=4, K=5, kb=2):
    """gains_along on the CSTR with T_R = NaN at knot (kb, 1): the pair is zero with its status bit, the trajectory reports bit 2 at that
    step and replays u* up to it; the others equal the run without the failure"""
    model, lqr, X, U, kw, _, _ = _along_case("cstr_lqr", hostemu, Bn, K)
    clean = lqr.gains_along(model, X, U)
    Xb = X.copy()
    Xb[kb, 1, 2] = np.nan
    r = lqr.gains_along(model, Xb, U)
    for key in ("K", "P0", "A", "B"):
        assert np.all(np.isfinite(r[key])), key
    assert r["pair_status"][kb, 1] == 2 and np.count_nonzero(r["pair_status"]) == 1
    assert not r["A"][kb, 1].any() and not r["B"][kb, 1].any()
    assert r["status"][1] == 4 and r["step"][1] == kb and not r["K"][:kb + 1, 1].any()
    assert same(r["K"][kb + 1:, 1], clean["K"][kb + 1:, 1])
    others = [0, 2, 3]
    assert np.all(r["status"][others] == 0) and same(r["K"][:, others], clean["K"][:, others]) and same(r["P0"][others], clean["P0"][others])


# ---------------------------------------------------------------------------------------------- 5. device-pointer entries
def check_device_entries(hostemu, Bn=67, K=4, ld=70):
    d = Dev(hostemu)
    A, Bm, Q, R, _ = random_pairs(K, Bn=Bn, seed=77)
    lqr = tv_lqr(12, 4, hostemu)
    ref = lqr.gains_tv_batch(A, Bm, Q, R, P_traj=True)
    Kt, M, Pt, P0, st = d.empty(K, Bn, 4, 12), d.empty(K, 4, 12, ld), d.empty(K + 1, Bn, 12, 12), d.empty(Bn, 12, 12), d.ints(Bn)
    dA, dB, dQ, dR = d.t(A), d.t(Bm), d.t(Q), d.t(R)
    stream = 0 if hostemu else torch.cuda.current_stream().cuda_stream
    lqr.gains_tv_batch_device(Bn, K, p(dA), p(dB), p(dQ), p(dR), p(dQ), p(P0), K_traj=p(Kt), law_M=p(M), ld=ld, P_traj=p(Pt), status=p(st),
                              stream=stream)
    d.sync()
    assert same(h(Kt), ref["K"]) and same(h(Pt), ref["P"]) and same(h(P0), ref["P0"]) and not h(st).any()
    Mh = h(M)
    assert same(Mh[..., :Bn], np.ascontiguousarray(ref["K"].transpose(0, 2, 3, 1))), "law layout = transposed K_traj"
    assert np.isnan(Mh[..., Bn:]).all(), "nothing behind column Bn of the law layout is written"
    # the law layout alone, shared weights
    M2 = d.empty(K, 4, 12, ld)
    lqr.gains_tv_batch_device(Bn, K, p(dA), p(dB), p(dQ[0]), p(dR[0]), p(dQ[0]), p(P0), law_M=p(M2), ld=ld, shared_mask=7, stream=stream)
    d.sync()
    sh = lqr.gains_tv_batch(A, Bm, Q[0], R[0])
    assert same(h(M2)[..., :Bn], np.ascontiguousarray(sh["K"].transpose(0, 2, 3, 1)))
    # gains_along_device on the CSTR
    model, lq, X, U, kw, _, _ = _along_case("cstr_lqr", hostemu, Bn, 3)
    ref = lq.gains_along(model, X, U)
    Qd, Rd = np.asarray(lq._Q_user, float), np.asarray(lq._R_user, float)
    dX, dU, dQ, dR = d.t(X), d.t(U), d.t(Qd), d.t(Rd)
    Ad, Bd, Kt, P0, st, ps = d.empty(3, Bn, 4, 4), d.empty(3, Bn, 4, 2), d.empty(3, Bn, 2, 4), d.empty(Bn, 4, 4), d.ints(Bn), d.ints(3, Bn)
    lq.gains_along_device(model, Bn, 3, p(dX), p(dU), p(Ad), p(Bd), p(dQ), p(dR), p(dQ), p(P0), K_traj=p(Kt), pair_status=p(ps), status=p(st),
                          shared_mask=7, stream=stream)
    d.sync()
    for have, want in ((Ad, ref["A"]), (Bd, ref["B"]), (Kt, ref["K"]), (P0, ref["P0"])):
        assert same(h(have), want)
    assert not h(st).any() and not h(ps).any()


def _refused(call, words):
    try:
        call()
    except RuntimeError as e:
        assert all(w in str(e) for w in words), (str(e), words)
        return
    raise AssertionError(f"accepted: expected a refusal naming {words}")


def check_lqr_refusals(hostemu):
    """the refusals of dompc_lqr_pairs_device / dompc_lqr_tv_device by name, from C (return code 1, dompc_lqr_last_error) and from
    Python (RuntimeError with that text); B <= 0, and K <= 0 without outputs, launch nothing"""
    d = Dev(hostemu)
    buf = d.empty(4096)
    q = p(buf)
    std, rate = tv_lqr(3, 1, hostemu), tv_lqr(12, 4, hostemu, rate=True)
    model, with_model, *_ = _along_case("cstr_lqr", hostemu, 2, 2)
    tvd = lambda l, *a, **k: (lambda: l.gains_tv_batch_device(*a, **k))      # noqa: E731
    cases = [
        (tvd(std, 2, 2, 0, q, q, q, q, q, K_traj=q), ("null trajectory",)),
        (tvd(std, 2, 2, q, 0, q, q, q, q, K_traj=q), ("null trajectory",)),
        (tvd(std, 2, 0, q, q, q, q, q, q, K_traj=q), ("K <= 0",)),
        (tvd(std, 2, -1, q, q, q, q, q, q), ("K <= 0",)),
        (tvd(rate, 2, 2, q, q, q, q, q, q, law_M=q, ld=2), ("law layout", "standard mode")),
        (tvd(std, 3, 2, q, q, q, q, q, q, law_M=q, ld=2), ("ld < B",)),
        (lambda: std.gains_along_device(None, 2, 2, q, q, q, q, q, q, q, q), ("no model",)),
        (lambda: with_model.gains_along_device(model, 2, 2, 0, q, q, q, q, q, q, q), ("null trajectory",)),
        (lambda: with_model.gains_along_device(model, 2, 0, q, q, q, q, q, q, q, q), ("K <= 0",)),
    ]
    for call, words in cases:
        _refused(call, ("dompc_lqr",) + words)
    # ... and from C
    dsg = std._design(None)
    vp = C.c_void_p
    assert dsg.lib.dompc_lqr_tv_device(dsg.h, 2, 2, None, vp(q), None, vp(q), vp(q), vp(q), 0, vp(q), None, 0, None, vp(q), None, None) == 1
    assert b"null trajectory" in dsg.lib.dompc_lqr_last_error(dsg.h)
    assert dsg.lib.dompc_lqr_tv_device(dsg.h, 3, 2, vp(q), vp(q), None, vp(q), vp(q), vp(q), 0, None, vp(q), 2, None, vp(q), None, None) == 1
    assert b"ld < B" in dsg.lib.dompc_lqr_last_error(dsg.h)
    assert dsg.lib.dompc_lqr_pairs_device(dsg.h, 2, 2, vp(q), vp(q), None, None, None, 0, vp(q), vp(q), None, None, None) == 1
    assert b"no model" in dsg.lib.dompc_lqr_last_error(dsg.h)
    dr = rate._design(None)
    assert dr.lib.dompc_lqr_tv_device(dr.h, 2, 2, vp(q), vp(q), None, vp(q), vp(q), vp(q), 0, None, vp(q), 2, None, vp(q), None, None) == 1
    assert b"law layout" in dr.lib.dompc_lqr_last_error(dr.h)
    # nothing to do: no launch, no refusal
    std.gains_tv_batch_device(0, 2, 0, 0, 0, 0, 0, 0)
    std.gains_tv_batch_device(2, 0, 0, 0, 0, 0, 0, 0)
    with_model.gains_along_device(model, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0)
    assert np.isnan(h(buf)).all()


# ---------------------------------------------------------------------------------------------- 6. the rollout with law_step
LB, UB = np.array([-0.6]), np.array([0.7])


def family_law(d, Bn, K, ld, seed=41):
    """a law record per step for the probe family (n_x = 3, n_u = 1): random references and gains, fallback flags, the clip; arrays
    [K][..][ld] with the loops innermost -> (record of step 0, tensors that own the memory)"""
    rng = np.random.default_rng(seed)
    keep = {"x_ref": d.t(rng.uniform(-1, 1, (K, 3, ld))), "u_ref": d.t(rng.uniform(-0.5, 0.5, (K, 1, ld))),
            "M": d.t(rng.uniform(-1, 1, (K, 1, 3, ld))), "flags": d.t(rng.integers(0, 4, (K, ld)) * (rng.uniform(0, 1, (K, ld)) < 0.2), torch.int32),
            "lb": d.t(LB), "ub": d.t(UB), "x_scale": d.t(np.ones(3))}

    def record(k):
        return AffineLaw(x_ref=p(keep["x_ref"][k]), u_ref=p(keep["u_ref"][k]), M=p(keep["M"][k]), flags=p(keep["flags"][k]), lb=p(keep["lb"]),
                         ub=p(keep["ub"]), x_scale=p(keep["x_scale"]), ld=ld, max_dx=1.5, clip=1, pad=0)
    return record, keep


def check_rollout_law_step(kind, K, hostemu, Bn=65, ld=68):
    """one launch of K steps with law_step = ld equals, bit for bit, K launches of one step with the law record advanced by hand:
    X_traj, U_traj, law_status, plant_status (and Y_traj, Z_traj); noise, measurements and per-loop parameters as in the general
    rollout; Bn = 65: one lane in the second wavefront; ld > Bn: the step of the law arrays is not the batch"""
    d = Dev(hostemu)
    sim = pf.make_simulator(kind, hostemu)
    m = sim.model
    base = pf.take(pf.draw(), slice(0, Bn))
    steps = [pf.take(pf.draw(seed=pf.SEED + 11 + k), slice(0, Bn)) for k in range(K)]
    W, V, P, TVP = d.t(np.stack([s["W"] for s in steps])), d.t(np.stack([s["V"] for s in steps])), d.t(base["P"]), d.t(base["TVP"][:K].copy())
    record, keep = family_law(d, Bn, K, ld)
    nz = m.n_z

    def launch(Xt, Ut, Yt, Zt, pst, lst, k0, K_, law_step, reseed):
        sim.rollout_device(Bn, K_, p(Xt), p(Ut), law=record(k0), W_traj=p(W[k0]), V_traj=p(V[k0]), Y_traj=p(Yt), Z_traj=p(Zt) if nz else 0,
                           tvp_rows=p(TVP[k0]), p_loops=p(P), plant_status=p(pst), law_status=p(lst), reseed_z=reseed, law_step=law_step)
        d.sync()

    def buffers():
        return d.empty(K + 1, Bn, 3), d.empty(K, Bn, 1), d.empty(K, Bn, 2), d.empty(K, Bn, max(nz, 1)), d.ints(K, Bn), d.ints(K, Bn)
    a = buffers()
    a[0][0].copy_(d.t(base["X"]))
    launch(*a, 0, K, ld, True)
    b = buffers()
    b[0][0].copy_(d.t(base["X"]))
    for k in range(K):
        launch(b[0][k:k + 2], b[1][k:k + 1], b[2][k:k + 1], b[3][k:k + 1], b[4][k:k + 1], b[5][k:k + 1], k, 1, 0, k == 0)
    names = ("X_traj", "U_traj", "Y_traj", "Z_traj", "plant_status", "law_status")
    for name, x, y in zip(names, a, b):
        if name == "Z_traj" and not nz:
            continue
        assert same(h(x), h(y)), name
    U, ls = h(a[1]), h(a[5])
    assert np.isfinite(h(a[0])).all() and np.isfinite(U).all()
    print(f"rollout with law_step, {kind} K={K}: clipped {int(((ls & 4) != 0).sum())}, far {int(((ls & 8) != 0).sum())}, fallback "
          f"{int(((ls & 3) != 0).sum())} of {K * Bn} law steps")
    assert ((ls & 4) != 0).any() and ((ls & 4) == 0).any() and ((ls & 3) != 0).any()
    if K > 1:                                # the record moves: step 1 with the record of step 0 gives other inputs
        c = buffers()
        c[0][0].copy_(d.t(base["X"]))
        launch(*c, 0, K, 0, True)
        assert same(h(c[1][0]), U[0]) and not same(h(c[1][1]), U[1])


def check_rollout_refusals(hostemu):
    """law_step > 0 with G / up_ref, without a law, below B, and a negative one: refused by name from Python and from C"""
    d = Dev(hostemu)
    Bn, K = 3, 2
    sim = pf.make_simulator("ode", hostemu)
    record, keep = family_law(d, Bn, K, Bn)
    Xt, Ut, dummy = d.empty(K + 1, Bn, 3), d.empty(K, Bn, 1), d.t(np.zeros(16))
    good = dict(tvp_rows=p(dummy), p_loops=p(dummy))
    cases = [(dict(law=record(0), G=p(dummy), up_ref=p(dummy), U_prev0=p(dummy), law_step=Bn), ("law_step", "G", "up_ref")),
             (dict(law_step=Bn), ("law_step", "without a law")),
             (dict(law=record(0), law_step=Bn - 1), ("law_step < B",)),
             (dict(law=record(0), law_step=-1), ("law_step", "negative"))]
    for kw, words in cases:
        try:
            sim.rollout_device(Bn, K, p(Xt), p(Ut), **good, **kw)
        except RuntimeError as e:
            assert all(w in str(e) for w in ("dompc_plant_rollout_device",) + words), (str(e), words)
        else:
            raise AssertionError(f"accepted: expected a refusal naming {words}")
        r = RolloutDesc()
        law = kw.get("law")
        r.law = C.addressof(law) if law is not None else None
        r.X_traj, r.U_traj, r.tvp_rows, r.p_loops = p(Xt), p(Ut), p(dummy), p(dummy)
        for k_ in ("G", "up_ref", "U_prev0"):
            setattr(r, k_, kw.get(k_) or None)
        r.law_step = kw["law_step"]
        assert sim._lib.dompc_plant_rollout_device(sim._h, Bn, K, C.byref(r), None) == 1
        assert all(w.encode() in sim._lib.dompc_plant_last_error(sim._h) for w in words)
    assert np.isnan(h(Xt)).all() and np.isnan(h(Ut)).all()


# ---------------------------------------------------------------------------------------------- 7. the loop
def tracking_case(hostemu, Bn=9, noise=False):
    """(controller, plant, X_ref, U_ref, starts) of examples/cstr_tracking.py"""
    ct = cstr_tracking
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        lqr = lc.setup_lqr(ct.build_lqr(setup=False), hostemu)
    sim = lc.plant_on(ct.build_simulator(ct.build_model(process_noise=noise), setup=False), hostemu)
    X_ref, U_ref = ct.record(sim)
    return lqr, sim, X_ref, U_ref, ct.starts(Bn)


def make_loop(hostemu, *args, **kw):
    """BatchClosedLoopTVLQR on the device or on the host emulation (its law-step kernel included)"""
    return BatchClosedLoopTVLQR(*args, device="cpu" if hostemu else 0, _law_lib=asmpc_hostemu_library if hostemu else None, **kw)


def check_loop_paths(hostemu, noise, Bn=9, n=7):
    """run(n, fused=True, chunk=c) - rollout launches with a law record per step - equals n calls of step() - the law-step kernel, then
    the plant step - bit for bit for c in {1, 3, n}, with and without W, and leaves the loop where they do; the two can be mixed; a
    step past the end of the reference raises"""
    lqr, sim, X_ref, U_ref, X0 = tracking_case(hostemu, Bn)
    base = make_loop(hostemu, lqr, sim, X0, X_ref, U_ref)          # (designs its gains on the resident reference)
    assert not base.design_status["status"].any() and not base.design_status["pair_status"].any()
    Ktraj = np.ascontiguousarray(base.M.cpu().numpy().transpose(0, 3, 1, 2))
    assert Ktraj.any()
    W = None
    if noise:                                # the plant with process noise; the gains are those of the design above
        _, sim, X_ref, U_ref, _ = tracking_case(hostemu, Bn, noise=True)
        W = rc.noise_of(sim, Bn, n)
        base = make_loop(hostemu, lqr, sim, X0, X_ref, U_ref, K_traj=Ktraj)
    xs, us = [X0], []
    for k in range(n):
        s = base.step(w=None if W is None else W[k])
        xs.append(s["x"].copy()); us.append(s["u0"].copy())
        assert not s["plant_status"].any()
    xs, us = np.stack(xs), np.stack(us)
    assert np.isfinite(xs).all() and base.k == n
    for c in (1, 3, n):
        loop = make_loop(hostemu, lqr, sim, X0, X_ref, U_ref, K_traj=Ktraj)
        rec = loop.run(n, fused=True, chunk=c, W=W)
        assert same(rec["x"], xs) and same(rec["u"], us), c
        assert loop.k == n and same(loop.plant.X.cpu().numpy(), xs[n]) and same(loop.U.cpu().numpy(), us[n - 1])
        assert rec["plant_status"].shape == (n, Bn) and rec["law_status"].shape == (n, Bn)
    unfused = make_loop(hostemu, lqr, sim, X0, X_ref, U_ref, K_traj=Ktraj).run(n, fused=False, W=W)
    assert same(unfused["x"], xs) and same(unfused["u"], us)
    if noise:
        quiet = make_loop(hostemu, lqr, sim, X0, X_ref, U_ref, K_traj=Ktraj).run(n)
        assert not same(quiet["x"], xs)
        assert same(rec["law_status"][-1], loop.lstat.cpu().numpy())
    # the rest of the reference (the two paths mixed), then one step too many
    rest = base.run()
    assert base.k == base.K and rest["x"].shape[0] == base.K - n + 1
    for call in (base.step, lambda: base.run(1)):
        try:
            call()
        except ValueError as e:
            assert "past the end" in str(e)
        else:
            raise AssertionError("a step past the end of the reference was accepted")


# What the host emulation gives on examples/cstr_tracking.py (B = 9 starts of cstr_tracking.starts, 20 steps): see the docstring of
# check_tracking_beats_replay; MARGIN: the closed loop's final deviation has to be below this fraction of the open loop's
TRACKING_MARGIN = 0.5


def deviation(x, X_ref):
    """distance to the reference at the last step, per loop, in the scale of the states (kmol/m^3, kmol/m^3, 100 K, 100 K)"""
    return np.linalg.norm((x[-1] - X_ref[-1]) / np.array([1.0, 1.0, 100.0, 100.0]), axis=1)


def check_tracking_beats_replay(hostemu, Bn=9):
    """on examples/cstr_tracking.py every perturbed start ends nearer to the reference under the time-varying law than when U_ref is
    replayed open loop (below TRACKING_MARGIN of it).  The perturbation (cstr_tracking.START_SPREAD: up to 0.1 kmol/m^3 and 2 K) was
    checked on the host emulation first.  Observed there and, to the digits printed, on the MI355X (B = 9, 20 steps, scaled
    distance at the last step): closed loop 6.9e-5 .. 4.7e-4, open loop 1.0e-3 .. 5.6e-2, ratio closed / open 0.005 .. 0.18 - the
    worst member has a factor 2.7 of room under the margin of 0.5"""
    lqr, sim, X_ref, U_ref, X0 = tracking_case(hostemu, Bn)
    K = U_ref.shape[0]
    loop = make_loop(hostemu, lqr, sim, X0, X_ref, U_ref)
    rec = loop.run()
    assert not rec["plant_status"].any() and not loop.design_status["status"].any()
    replay = sim.simulate_batch(X0, U_ref[:, 0])
    assert not (replay["status"] & 1).any()
    dc, do = deviation(rec["x"], X_ref), deviation(replay["x"], X_ref)
    print(f"cstr_tracking, {Bn} starts, {K} steps: final deviation closed loop {dc[1:]}\n  open loop {do[1:]}\n  ratio {dc[1:] / do[1:]}")
    assert same(rec["x"][:, 0], X_ref[:, 0]) or np.max(np.abs(rec["x"][:, 0] - X_ref[:, 0])) < 1e-9      # (start 0 is the reference's own)
    assert np.all(dc[1:] < TRACKING_MARGIN * do[1:])
    return dc, do
