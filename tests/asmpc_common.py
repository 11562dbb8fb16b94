"""TEST-ONLY helpers of the sensitivity-based MPC tests: the host emulation of csrc/dompc_asmpc.hip (the text that ships), synthetic
law records, numpy's evaluation of the reference formula, and the checks the CPU and the GPU suite share (each with a `hostemu=`
switch: the host emulation with "device" memory = host memory, or the HIP path)."""
from types import SimpleNamespace

import numpy as np

import differentiator_batch_common as bc
import plant
from asmpc_hostemu import asmpc_hostemu_library
from do_mpc_amd.asmpc import ASMPC
from do_mpc_amd.closed_loop import BatchClosedLoopASMPC
from do_mpc_amd.examples import CASES
from do_mpc_amd.simulator import Simulator
from lqr_common import plant_on
from simulator_common import T_STEP

# (n_x, n_u): one input, two, a size that is no multiple of anything, a full row of lanes, the limit
SHAPES = [(1, 1), (4, 1), (4, 2), (17, 3), (3, 16), (64, 16)]
# 1, one full wavefront of the preparation, a partial last one, a partial last workgroup of the step and the rollout
BATCHES = [1, 4, 5, 67]
_CACHE = {}


def make_asmpc(mpc, hostemu):
    return ASMPC(mpc, _lib_path=asmpc_hostemu_library, _code_object="") if hostemu else ASMPC(mpc)


def stub_mpc(nx, nu, lbu=None, ubu=None, x_scaling=None):
    """what ASMPC reads of a controller for set_law and the law step: sizes, input bounds, state scaling"""
    v = lambda a, n, d: SimpleNamespace(master=np.full(n, d) if a is None else np.asarray(a, float))      # noqa: E731
    return SimpleNamespace(flags={"setup": True}, model=SimpleNamespace(n_x=nx, n_u=nu), S=None, settings=SimpleNamespace(gpu_index=0),
                           _u_lb=v(lbu, nu, -np.inf), _u_ub=v(ubu, nu, np.inf), _x_scaling=v(x_scaling, nx, 1.0), u0=v(None, nu, 0.0))


def record(nx, nu, B, seed):
    """a synthetic solve: x_prev, u0, J, G with the infinity norm of G at most 0.5 (cond(I - G) <= 3), and states X to step at"""
    rng = np.random.default_rng(seed)
    G = rng.uniform(-1.0, 1.0, (B, nu, nu))
    G *= 0.5 / np.max(np.sum(np.abs(G), axis=2), axis=1)[:, None, None]
    J = rng.standard_normal((B, nu, nx))
    x_prev, u0 = rng.standard_normal((B, nx)), rng.standard_normal((B, nu))
    X = x_prev + 0.1 * rng.standard_normal((B, nx))
    return dict(x_prev=x_prev, u0=u0, J=J, G=G, ok=np.ones(B, bool), X=X)


def reference(r, b, x):
    """(M, u) of member b: numpy's evaluation of the reference formula inv(I - G) @ (u0 + J dx - G u0) (main.py:170-172)"""
    nu = r["u0"].shape[1]
    inv = np.linalg.inv(np.eye(nu) - r["G"][b])
    u0 = r["u0"][b].reshape(-1, 1)
    return inv @ r["J"][b], (inv @ (u0 + r["J"][b] @ (x - r["x_prev"][b]).reshape(-1, 1) - r["G"][b] @ u0)).ravel()


def close(a, ref):
    """the bound of differentiator_batch_common.check_asmpc"""
    return np.max(np.abs(a - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))


def law_of(r, hostemu, **settings):
    nx, nu = r["x_prev"].shape[1], r["u0"].shape[1]
    a = make_asmpc(stub_mpc(nx, nu, **{k: settings.pop(k) for k in ("lbu", "ubu", "x_scaling") if k in settings}), hostemu)
    for k, v in settings.items():
        setattr(a.settings, k, v)
    a.set_law(r["x_prev"], r["u0"], r["J"], r["G"], r["ok"])
    return a


def check_shape(nx, nu, B, hostemu):
    r = record(nx, nu, B, seed=1000 * nx + 10 * nu + B)
    a = law_of(r, hostemu)
    L = a.law
    assert L["M"].shape == (B, nu, nx) and L["x_ref"].shape == (B, nx) and L["u_ref"].shape == (B, nu) and not L["flags"].any()
    assert np.array_equal(L["x_ref"], r["x_prev"]) and np.array_equal(L["u_ref"], r["u0"])
    U, st = a.make_step_batch(r["X"])
    assert U.shape == (B, nu) and not st.any()
    worst = 0.0
    for b in range(B):
        M, u = reference(r, b, r["X"][b])
        worst = max(worst, np.max(np.abs(L["M"][b] - M)), np.max(np.abs(U[b] - u)))
        assert close(L["M"][b], M) and close(U[b], u), (b, np.max(np.abs(L["M"][b] - M)), np.max(np.abs(U[b] - u)))
    print(f"n_x = {nx}, n_u = {nu}, B = {B}: max |M - ref|, |U - ref| = {worst:.3e}")
    # at the expansion point the law returns u0 itself
    U0, _ = a.make_step_batch(r["x_prev"])
    assert np.array_equal(U0, r["u0"])


def check_pivoting(hostemu):
    """(I - G)[0][0] = 0 in a non-singular I - G = [[0, 1], [1, 1]]: solved, by the pivot search over the lanes"""
    r = record(3, 2, 5, seed=7)
    r["G"][2] = np.eye(2) - np.array([[0.0, 1.0], [1.0, 1.0]])
    a = law_of(r, hostemu)
    L = a.law
    assert not L["flags"].any()
    U, st = a.make_step_batch(r["X"])
    for b in range(5):
        M, u = reference(r, b, r["X"][b])
        assert close(L["M"][b], M) and close(U[b], u), b
    assert not st.any()


def check_fallbacks(hostemu):
    """singular I - G, ok = False and a NaN in J: each flags its own member, gives M = 0 and u = u0 there, and leaves the other members
    of the same wavefront as they are in a run without the bad member, bit for bit"""
    base = record(4, 2, 5, seed=11)
    good = law_of(base, hostemu)
    Lg = good.law
    Ug, _ = good.make_step_batch(base["X"])
    for what, member, bit in (("singular", 1, 2), ("not ok", 2, 1), ("nan", 3, 1)):
        r = {k: v.copy() for k, v in base.items()}
        if what == "singular":
            r["G"][member] = np.eye(2) - np.array([[1.0, 2.0], [2.0, 4.0]])
        elif what == "not ok":
            r["ok"][member] = False
        else:
            r["J"][member, 1, 2] = np.nan
        a = law_of(r, hostemu)
        L = a.law
        U, st = a.make_step_batch(r["X"])
        expect = np.zeros(5, dtype=np.int32)
        expect[member] = bit
        assert np.array_equal(L["flags"], expect) and np.array_equal(st, expect), (what, L["flags"], st)
        assert not L["M"][member].any() and np.array_equal(U[member], r["u0"][member]), what
        others = [b for b in range(5) if b != member]
        assert np.array_equal(L["M"][others], Lg["M"][others]) and np.array_equal(U[others], Ug[others]), what


def check_clip_nan_and_max_dx(hostemu):
    r = record(4, 2, 67, seed=13)
    free = law_of(r, hostemu, clip_to_bounds=False)
    Uf, stf = free.make_step_batch(r["X"])
    assert not stf.any()
    # a finite bound on input 0 only, input 1 unbounded: clipped rows carry bit 2, an infinite bound never clips
    lo, hi = float(np.quantile(Uf[:, 0], 0.3)), float(np.quantile(Uf[:, 0], 0.7))
    a = law_of(r, hostemu, lbu=[lo, -np.inf], ubu=[hi, np.inf])
    U, st = a.make_step_batch(r["X"])
    clipped = (Uf[:, 0] < lo) | (Uf[:, 0] > hi)
    assert clipped.any() and not clipped.all()
    assert np.array_equal(st, np.where(clipped, 4, 0)) and np.array_equal(U[:, 0], np.minimum(np.maximum(Uf[:, 0], lo), hi))
    assert np.array_equal(U[:, 1], Uf[:, 1])
    # ... and clip_to_bounds = False with the same bounds does not clip
    off = law_of(r, hostemu, lbu=[lo, -np.inf], ubu=[hi, np.inf], clip_to_bounds=False)
    assert np.array_equal(off.make_step_batch(r["X"])[0], Uf)
    # a NaN state: NaN inputs in that row only, also with the clip on
    X = r["X"].copy()
    X[5, 1] = np.nan
    Un, stn = a.make_step_batch(X)
    assert np.isnan(Un[5]).all() and np.array_equal(np.delete(Un, 5, axis=0), np.delete(U, 5, axis=0))
    assert np.array_equal(np.delete(stn, 5), np.delete(st, 5))
    # max_dx: the infinity norm of (x - x_ref) / x_scaling
    xs = np.array([1.0, 2.0, 0.5, 4.0])
    dist = np.max(np.abs(r["X"] - r["x_prev"]) / xs, axis=1)
    thr = float(np.median(dist))
    f = law_of(r, hostemu, x_scaling=xs, max_dx=thr, clip_to_bounds=False)
    Ud, std = f.make_step_batch(r["X"])
    assert np.array_equal(std, np.where(dist > thr, 8, 0)) and (std == 8).any() and (std == 0).any()
    assert np.array_equal(Ud, Uf)                              # (it only flags)


def check_refusals(make_mpc, solver_context):
    """what make_step_batch(..., sensitivities=True) refuses, and the two sizes, each by name"""
    import parity_common as pc
    for nx, nu, word in ((65, 1, "n_x = 65"), (4, 17, "n_u = 17")):
        try:
            ASMPC(stub_mpc(nx, nu))
        except NotImplementedError as e:
            assert word in str(e), str(e)
        else:
            raise AssertionError("not refused: " + word)
    for mpc, word in ((make_mpc("CSTR", nl_cons_single_slack=True), "nl_cons_single_slack"),
                      (make_mpc("CSTR", open_loop=True, **pc.OPEN_LOOP_CASES[0][1]), "open_loop")):
        try:
            ASMPC(mpc)
        except NotImplementedError as e:
            assert word in str(e), (word, str(e))
        else:
            raise AssertionError("not refused: " + word)
    a = ASMPC(stub_mpc(4, 1))
    try:
        a.law
    except RuntimeError as e:
        assert "solve" in str(e)
    else:
        raise AssertionError("a law before any solve")


# ---------------------------------------------------------------------------------------------- end to end
def solved(make_mpc, name, hostemu):
    """(controller, ASMPC, result of ASMPC.solve at batch_states(name), the law without clipping) - once per case"""
    key = (name, hostemu)
    if key not in _CACHE:
        mpc = make_mpc(name, max_batch=5)
        a = make_asmpc(mpc, hostemu)
        a.settings.clip_to_bounds = False
        r = a.solve(bc.batch_states(name))
        _CACHE[key] = (mpc, a, r)
    return _CACHE[key]


def check_solve_equals_example(make_mpc, name, hostemu):
    """ASMPC.solve + make_step_batch without clipping = examples.batch_reactor_asmpc.ASMPC (the numpy restatement of the reference
    class) at the bound of check_asmpc; with clipping = that value clipped"""
    from do_mpc_amd.examples.batch_reactor_asmpc import ASMPC as Example
    mpc, a, r = solved(make_mpc, name, hostemu)
    X0 = bc.batch_states(name)
    assert r["ok"].all() and not a.law["flags"].any()
    ex = Example(mpc)
    ex.last = {"x_prev": X0.copy(), "u0": r["u0"].copy(), "du0dx0": r["du0dx0"].copy(), "du0du_prev": r["du0du_prev"].copy(), "ok": r["ok"].copy()}
    X = X0 * (1.0 + 0.01 * np.random.default_rng(3).standard_normal(X0.shape))
    ref = ex.make_step_batch(X)
    a.settings.clip_to_bounds = False
    U, st = a.make_step_batch(X)
    print(f"{name}: max |U - example| = {np.max(np.abs(U - ref)):.3e}, max |U - u0| = {np.max(np.abs(U - r['u0'])):.3e}")
    for q in range(5):
        assert close(U[q], ref[q]), (q, U[q], ref[q])
    assert not st.any() and np.max(np.abs(U - r["u0"])) > 1e-6
    U0, _ = a.make_step_batch(X0)
    assert np.array_equal(U0, r["u0"])                            # at the expansion point: the solver's u0, difference exactly 0
    a.settings.clip_to_bounds = True
    Uc, stc = a.make_step_batch(X)
    lb, ub = mpc._u_lb.master, mpc._u_ub.master
    assert np.array_equal(Uc, np.minimum(np.maximum(U, lb), ub)) and np.array_equal(stc != 0, np.any(Uc != U, axis=1))
    a.settings.clip_to_bounds = False


def make_plant(name, hostemu, varying=False):
    """the example's plant; varying: its parameters move with the loop time"""
    m = CASES[name].build_model()
    sim = Simulator(m)
    sim.set_param(integration_tool="cvodes", abstol=1e-10, reltol=1e-10, t_step=T_STEP.get(name, 0.5))
    if m.n_p:
        pt = sim.get_p_template()
        vals = plant.PLANT_P[name]

        def p_fun(t):
            for i, (k, v) in enumerate(vals.items()):
                pt[k] = v * (1.0 + (0.02 * np.sin(40.0 * t / T_STEP[name] + i) if varying else 0.0))
            return pt
        sim.set_p_fun(p_fun)
    if m.n_tvp:
        tv = sim.get_tvp_template()
        sim.set_tvp_fun(lambda t: tv)
    return plant_on(sim, hostemu)


def make_loop(make_mpc, name, hostemu, resolve_every, varying=False, **settings):
    mpc = make_mpc(name, max_batch=5)
    a = make_asmpc(mpc, hostemu)
    a.settings.resolve_every = resolve_every
    for k, v in settings.items():
        setattr(a.settings, k, v)
    return BatchClosedLoopASMPC(a, make_plant(name, hostemu, varying), bc.batch_states(name), device="cpu" if hostemu else 0)


def same_records(ra, rb):
    return all(np.array_equal(ra[k], rb[k], equal_nan=True) for k in ("x", "u", "plant_status", "law_status")) and ra["solve_steps"] == rb["solve_steps"]


def check_fused_equals_stepwise(make_mpc, name, hostemu, varying=False, n=6, resolve_every=3):
    """run(n, fused=True) = run(n, fused=False) bit for bit on x, u and both statuses: the fma contract of csrc/dompc_affine.h"""
    fused = make_loop(make_mpc, name, hostemu, resolve_every, varying).run(n, fused=True)
    step = make_loop(make_mpc, name, hostemu, resolve_every, varying).run(n, fused=False)
    B = 5
    assert fused["x"].shape == (n + 1, B, 4) and fused["law_status"].shape == (n, B) and fused["solve_steps"] == list(range(0, n, resolve_every))
    assert len(fused["stats"]) == len(fused["solve_steps"]) and all(s["success"].all() for s in fused["stats"])
    assert not fused["plant_status"].any()
    assert np.max(np.abs(fused["u"][1] - fused["u"][0])) > 0.0                 # (the continuation moves the inputs)
    assert same_records(fused, step), {k: float(np.nanmax(np.abs(fused[k].astype(float) - step[k]))) for k in ("x", "u")}
    return fused


def check_make_step_equals_row0(make_mpc, name, hostemu, n=6, resolve_every=3):
    """ASMPC.make_step over n calls = row 0 of the batched loop.  Both solve on the steps 0, 3 with the same warm start and u_prev.  On
    the host emulation the single solve and the batched solve run the same code for a problem: equal bits.  On the GPU they are two
    launch shapes of the solver (reductions in another order), compared at the 1e-9 the suite compares them at elsewhere
    (test_gpu_ekf: closed loops per sample against the batch)."""
    tol = 0.0 if hostemu else 1e-9
    rec = make_loop(make_mpc, name, hostemu, resolve_every).run(n, fused=False)
    mpc = make_mpc(name)
    a = make_asmpc(mpc, hostemu)
    a.settings.resolve_every = resolve_every
    sim = make_plant(name, hostemu)
    x0 = bc.batch_states(name)[0].reshape(-1, 1)
    mpc.x0 = x0
    mpc.u0 = np.zeros((mpc.model.n_u, 1))
    mpc.set_initial_guess()
    sim.x0 = x0
    worst = 0.0
    for k in range(n):
        u = a.make_step(x0)
        x0 = sim.make_step(u)
        eu = np.max(np.abs(u.ravel() - rec["u"][k, 0]) / np.maximum(1.0, np.abs(rec["u"][k, 0])))
        ex = np.max(np.abs(np.asarray(x0).ravel() - rec["x"][k + 1, 0]) / np.maximum(1.0, np.abs(rec["x"][k + 1, 0])))
        worst = max(worst, eu, ex)
        assert eu <= tol and ex <= tol, (k, eu, ex)
    print(f"{name}: make_step against row 0 of the batched loop, worst relative deviation {worst:.3e}")
    assert a.u_data.shape == (mpc.model.n_u, n + 1) and np.array_equal(a.u_data[:, -1], u.ravel())


def check_dae_plant_is_refused(make_mpc, hostemu):
    name = "oscillating_masses_dae"
    mpc = make_mpc(name)
    a = make_asmpc(mpc, hostemu)
    sim = make_plant(name, hostemu)
    loop = BatchClosedLoopASMPC(a, sim, np.asarray(CASES[name].X0, float).reshape(1, -1), device="cpu" if hostemu else 0)
    try:
        loop.run(2, fused=True)
    except NotImplementedError as e:
        assert "algebraic states" in str(e)
    else:
        raise AssertionError("a DAE plant was accepted by the rollout")
    try:
        sim.rollout_affine_device(1, 1, a.law_record() if a.batch else None, 0, 0)
    except NotImplementedError as e:
        assert "algebraic states" in str(e)
    else:
        raise AssertionError("a DAE plant was accepted by Simulator.rollout_affine_device")


def check_rollout_with_synthetic_law(hostemu, B=67, K=4):
    """Simulator.rollout_affine_device with a law from set_law on the CSTR plant with parameters that move with time, B = 67 (a
    partial last workgroup): trajectories and statuses = the step-wise launches law step -> plant step, bit for bit"""
    import torch
    name = "CSTR"
    sim = make_plant(name, hostemu, varying=True)
    rng = np.random.default_rng(17)
    X0 = np.asarray(CASES[name].X0, float) * (1.0 + 0.02 * rng.standard_normal((B, 4)))
    r = dict(x_prev=X0 * (1.0 + 0.01 * rng.standard_normal((B, 4))), u0=np.tile([50.0, -4000.0], (B, 1)) * (1.0 + 0.1 * rng.standard_normal((B, 2))),
             J=rng.standard_normal((B, 2, 4)) * np.array([[10.0], [500.0]]), G=np.zeros((B, 2, 2)), ok=np.ones(B, bool))
    r["ok"][3] = False
    a = law_of(r, hostemu, lbu=[5.0, -8500.0], ubu=[60.0, 0.0], max_dx=0.05)
    dev = torch.device("cpu") if hostemu else torch.device("cuda", 0)
    t = lambda v, dt=torch.float64: torch.tensor(v, dtype=dt, device=dev)      # noqa: E731
    dt_ = T_STEP[name]
    rows = np.array([np.asarray(sim.p_fun(j * dt_).master, float).reshape(-1).copy() for j in range(K)])
    assert np.max(np.abs(rows[1] - rows[0])) > 0.0
    Xt, Ut = torch.empty((K + 1, B, 4), dtype=torch.float64, device=dev), torch.empty((K, B, 2), dtype=torch.float64, device=dev)
    pst, lst = (torch.zeros((K, B), dtype=torch.int32, device=dev) for _ in range(2))
    Xt[0].copy_(t(X0))
    P, dummy = t(rows), t(np.zeros(1))
    sim.rollout_affine_device(B, K, a.law_record(), Xt.data_ptr(), Ut.data_ptr(), dummy.data_ptr(), P.data_ptr(), pst.data_ptr(), lst.data_ptr())
    if not hostemu:
        torch.cuda.synchronize()
    X, U, Xn = t(X0), torch.empty((B, 2), dtype=torch.float64, device=dev), torch.empty((B, 4), dtype=torch.float64, device=dev)
    ls, ps_ = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2))
    for k in range(K):
        a.make_step_batch_device(B, X.data_ptr(), U.data_ptr(), ls.data_ptr())
        sim.step_batch_device(B, X.data_ptr(), U.data_ptr(), dummy.data_ptr(), P[k].data_ptr(), Xn.data_ptr(), 0, ps_.data_ptr(), shared_mask=2 | 4 | 8 | 16)
        if not hostemu:
            torch.cuda.synchronize()
        assert np.array_equal(U.cpu().numpy(), Ut[k].cpu().numpy()) and np.array_equal(Xn.cpu().numpy(), Xt[k + 1].cpu().numpy()), k
        assert np.array_equal(ls.cpu().numpy(), lst[k].cpu().numpy()) and np.array_equal(ps_.cpu().numpy(), pst[k].cpu().numpy()), k
        X, Xn = Xn, X
    lsh = lst.cpu().numpy()
    assert (lsh[:, 3] & 1).all() and (lsh & 4).any() and (lsh & 8).any() and not (pst.cpu().numpy() & 1).any()
    assert np.array_equal(Ut[:, 3].cpu().numpy(), np.tile(np.minimum(np.maximum(r["u0"][3], [5.0, -8500.0]), [60.0, 0.0]), (K, 1)))


# ---------------------------------------------------------------------------------------------- pivot orders that are not the identity
def _lu_order(A):
    from scipy.linalg import lu
    return tuple(int(i) for i in np.argmax(lu(A)[0], axis=0))


def permuted_record(nx, nu, B, seed):
    """record() with I - G = (signed permutation with entries in +-[1, 2]) + (0.4 / n_u) uniform(-1, 1): condition number about 2, and
    the pivot of a column is not the row of the same number.  Even members get a cyclic shift (by 1 + b / 2), odd members a random
    permutation that is neither the identity nor one of an earlier member"""
    r = record(nx, nu, B, seed)
    rng = np.random.default_rng(seed + 1)
    seen = {tuple(range(nu))}
    for b in range(B):
        if b % 2 == 0:
            perm = np.roll(np.arange(nu), 1 + (b // 2) % (nu - 1))
        else:
            perm = rng.permutation(nu)
            while tuple(perm) in seen:
                perm = rng.permutation(nu)
        seen.add(tuple(perm))
        A = np.zeros((nu, nu))
        A[np.arange(nu), perm] = rng.uniform(1.0, 2.0, nu) * rng.choice([-1.0, 1.0], nu)
        r["G"][b] = np.eye(nu) - (A + (0.4 / nu) * rng.uniform(-1.0, 1.0, (nu, nu)))
    return r


def check_pivot_orders(nx, nu, hostemu, B=5):
    """the Gauss-Jordan routine of csrc/dompc_lanes_la.h with a pivot order that is not the identity in every member, and another one
    in every member of the wavefront (asserted on the CPU with scipy.linalg.lu): the lane_gather at its end moves every row.  M and U
    against the reference formula at `close`; flags all 0.  n_u = 16: member 2 with row 5 of I - G zero (rank 15, the zero pivot is met
    in the last column) gets flag 2 and M = 0, the others are bit-equal to the run without it"""
    r = permuted_record(nx, nu, B, seed=5000 + 10 * nx + nu)
    orders = [_lu_order(np.eye(nu) - r["G"][b]) for b in range(B)]
    conds = [float(np.linalg.cond(np.eye(nu) - r["G"][b])) for b in range(B)]
    ident = tuple(range(nu))
    assert all(o != ident for o in orders) and all(orders[b] != orders[b + 1] for b in range(B - 1)) and len(set(orders)) >= 3, orders
    assert len(set(orders[:4])) >= 3 and max(conds) < 10.0, (orders, conds)
    a = law_of(r, hostemu)
    L = a.law
    U, st = a.make_step_batch(r["X"])
    assert not L["flags"].any() and not st.any(), (L["flags"], st)
    worst = 0.0
    for b in range(B):
        M, u = reference(r, b, r["X"][b])
        worst = max(worst, np.max(np.abs(L["M"][b] - M)) / max(1.0, np.max(np.abs(M))), np.max(np.abs(U[b] - u)) / max(1.0, np.max(np.abs(u))))
        assert close(L["M"][b], M) and close(U[b], u), (b, np.max(np.abs(L["M"][b] - M)), np.max(np.abs(U[b] - u)))
    print(f"n_x = {nx}, n_u = {nu}: cond(I - G) <= {max(conds):.2f}, {len(set(orders))} pivot orders, max |M - ref|, |U - ref| relative = {worst:.3e}")
    if nu == 16:
        s = {k: v.copy() for k, v in r.items()}
        s["G"][2, 5] = np.eye(nu)[5]
        assert np.linalg.matrix_rank(np.eye(nu) - s["G"][2]) == nu - 1
        bad = law_of(s, hostemu)
        Lb = bad.law
        Ub, stb = bad.make_step_batch(s["X"])
        expect = np.array([0, 0, 2, 0, 0], dtype=np.int32)
        assert np.array_equal(Lb["flags"], expect) and np.array_equal(stb, expect), (Lb["flags"], stb)
        assert not Lb["M"][2].any() and np.array_equal(Ub[2], s["u0"][2])
        others = [0, 1, 3, 4]
        assert np.array_equal(Lb["M"][others], L["M"][others]) and np.array_equal(Ub[others], U[others])
        bad.close()
    a.close()
