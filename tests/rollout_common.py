"""TEST-ONLY checks of the general plant rollout (csrc/dompc_plant.hip: dompc_plant_loop_kernel; Simulator.rollout_device,
Simulator.simulate_batch, BatchClosedLoopLQR.run(fused=True)), shared by the CPU suite (host emulation: "device" memory = host memory)
and the GPU suite - each check with a `hostemu=` switch.

Bits are compared with `same`: equal as 64-bit words where the arrays are float64 (a NaN equals the same NaN), np.array_equal else."""
import ctypes as C

import numpy as np
import torch

import asmpc_common as ac
import lqr_common as lc
import lqr_dae_common as ldc
import plant_family_common as pf
from do_mpc_amd import sym
from do_mpc_amd.asmpc import AffineLaw
from do_mpc_amd.closed_loop import BatchClosedLoopLQR
from do_mpc_amd.examples import CASES
from do_mpc_amd.simulator import RolloutDesc, Simulator
from simulator_common import T_STEP


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        return bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))
    return bool(np.array_equal(a, b))


class Dev:
    """tensors where the plant of a check lives"""

    def __init__(self, hostemu):
        self.hostemu = hostemu
        self.dev = torch.device("cpu") if hostemu else torch.device("cuda", 0)

    def t(self, a, dt=torch.float64):
        return torch.tensor(np.asarray(a), dtype=dt, device=self.dev)

    def empty(self, *shape):
        return torch.full(shape, np.nan, dtype=torch.float64, device=self.dev)

    def ints(self, *shape):
        return torch.full(shape, -1, dtype=torch.int32, device=self.dev)

    def sync(self):
        if not self.hostemu:
            torch.cuda.synchronize()


def p(a):
    return a.data_ptr() if a is not None else 0


def h(a):
    return a.cpu().numpy()


# ---------------------------------------------------------------------------------------------- 1. the bits of the law rollout
def cstr_law_case(hostemu, B, seed=17):
    """the plant, start and law of asmpc_common.check_rollout_with_synthetic_law: CSTR with parameters that move with time, a law from
    set_law with a fallback member, clipping and max_dx"""
    name = "CSTR"
    sim = ac.make_plant(name, hostemu, varying=True)
    rng = np.random.default_rng(seed)
    X0 = np.asarray(CASES[name].X0, float) * (1.0 + 0.02 * rng.standard_normal((B, 4)))
    r = dict(x_prev=X0 * (1.0 + 0.01 * rng.standard_normal((B, 4))), u0=np.tile([50.0, -4000.0], (B, 1)) * (1.0 + 0.1 * rng.standard_normal((B, 2))),
             J=rng.standard_normal((B, 2, 4)) * np.array([[10.0], [500.0]]), G=np.zeros((B, 2, 2)), ok=np.ones(B, bool))
    r["ok"][B // 2] = False
    a = ac.law_of(r, hostemu, lbu=[5.0, -8500.0], ubu=[60.0, 0.0], max_dx=0.05)
    return sim, X0, a


def cstr_rows(sim, K):
    rows = np.array([np.asarray(sim.p_fun(j * T_STEP["CSTR"]).master, float).reshape(-1).copy() for j in range(K)])
    assert K == 1 or np.max(np.abs(rows[1] - rows[0])) > 0.0
    return rows


def check_same_bits_as_law_rollout(hostemu, B, K):
    d = Dev(hostemu)
    sim, X0, a = cstr_law_case(hostemu, B)
    P, dummy = d.t(cstr_rows(sim, K)), d.t(np.zeros(1))
    out = []
    for general in (False, True):
        Xt, Ut, pst, lst = d.empty(K + 1, B, 4), d.empty(K, B, 2), d.ints(K, B), d.ints(K, B)
        Xt[0].copy_(d.t(X0))
        if general:
            sim.rollout_device(B, K, p(Xt), p(Ut), law=a.law_record(), tvp_rows=p(dummy), p_rows=p(P), plant_status=p(pst), law_status=p(lst))
        else:
            sim.rollout_affine_device(B, K, a.law_record(), p(Xt), p(Ut), p(dummy), p(P), p(pst), p(lst))
        d.sync()
        out.append([h(v) for v in (Xt, Ut, pst, lst)])
    old, new = out
    assert not np.isnan(old[0]).any() and (old[3][:, B // 2] & 1).all() and not (old[2] & 1).any()
    if B > 1:
        assert (old[3] & 4).any() and (old[3] & 8).any()
    for name, x, y in zip(("X_traj", "U_traj", "plant_status", "law_status"), old, new):
        assert same(x, y), name


# ---------------------------------------------------------------------------------------------- 2. open loop with noise
NAN_LANES = (5, 64)
# what the step-wise launches of check_open_loop_with_noise report per step (counted on the host emulation; asserted there before the
# rollout is looked at): lanes that took the implicit fallback, lanes that failed (the NaN lanes)
OPEN_LOOP_COUNTS = {"implicit": [26, 8, 9], "failed": [2, 2, 2]}


def open_loop_inputs(B, K):
    """per-loop lam, om, q of draw() with q < 0 in the lanes NAN_LANES, per step the inputs and noise of a draw of its own, the
    time-varying d shared by the batch"""
    base = pf.take(pf.draw(), slice(0, B))
    P = base["P"].copy()
    P[list(NAN_LANES), 2] = -0.5
    # (draws at which no lane of any step comes near the step cap: asserted in check_open_loop_with_noise, from the twin)
    steps = [pf.take(pf.draw(seed=pf.SEED + 4 + k), slice(0, B)) for k in range(K)]
    return {"X0": base["X"], "P": P, "U": np.stack([s["U"] for s in steps]), "W": np.stack([s["W"] for s in steps]),
            "V": np.stack([s["V"] for s in steps]), "TVP": base["TVP"][:K].copy()}


def stepwise(d, sim, inp, B, K, w=True, v=True, y=True):
    """K launches of step_batch_device with the rows of `inp` -> x [K + 1][B][nx], y [K][B][ny], status words [K][B]"""
    m = sim.model
    X, Xn, Y, st = d.t(inp["X0"]), d.empty(B, m.n_x), d.empty(B, max(m.n_y, 1)), d.ints(B)
    U, W, V, P, TVP = (d.t(inp[k]) for k in ("U", "W", "V", "P", "TVP"))
    xs, ys, ss = [h(X).copy()], [], []
    for k in range(K):
        sim.step_batch_device(B, p(X), p(U[k]), p(TVP[k]), p(P), p(Xn), p(Y) if y else 0, p(st), w=p(W[k]) if w else 0,
                              v=p(V[k]) if v else 0, shared_mask=2 | (0 if w else 8) | (0 if v else 16))
        d.sync()
        xs.append(h(Xn).copy()); ys.append(h(Y).copy()); ss.append(h(st).copy())
        X, Xn = Xn, X
    return np.stack(xs), np.stack(ys), np.stack(ss)


def check_open_loop_with_noise(hostemu, B=65, K=3):
    d = Dev(hostemu)
    sim = pf.make_simulator("ode", hostemu)
    inp = open_loop_inputs(B, K)
    xs, ys, ss = stepwise(d, sim, inp, B, K)
    # what the comparison is worth, from the step-wise results alone
    status, steps = ss & 0xFF, ss >> 8
    wave = steps[:, :64]
    healthy = np.setdiff1d(np.arange(64), NAN_LANES)
    assert any(len(set(wave[k, healthy])) > 1 for k in range(K)), "no step in which two lanes of the first wavefront differ in their step count"
    implicit = (status & 2) != 0
    print(f"open loop B={B} K={K}: implicit lanes per step {implicit.sum(axis=1)}, steps {steps.min()} .. {steps.max()}, "
          f"failed lanes per step {(status & 1).sum(axis=1)}, explicit lanes' largest step count {steps[~implicit].max()} (cap {pf.CAP})")
    assert np.array_equal(implicit.sum(axis=1), OPEN_LOOP_COUNTS["implicit"]) and (~implicit[:, healthy]).any()
    # (the counts hold on the device too: by the numpy twin of the explicit pair no lane of any step is within 5 steps of the cap, on
    #  either side - the condition 'clear_of_cap' of plant_family_common.conditions, here for every step's own start and rows)
    for k in range(K):
        at = {"X": xs[k], "U": inp["U"][k], "TVP": np.tile(inp["TVP"][k], (B, 1)), "P": inp["P"], "W": inp["W"][k], "V": inp["V"][k]}
        tw, near = pf.twin(at), pf.twin(at, cap=pf.CAP + 5)
        expl = tw["status"] == 0
        assert np.array_equal(~expl[healthy], implicit[k, healthy]), k
        assert np.all(near["status"][~expl] == 1) and np.all(tw["n_steps"][expl] <= pf.CAP - 5), (k, tw["n_steps"][expl].max())
    assert np.array_equal((status & 1).sum(axis=1), OPEN_LOOP_COUNTS["failed"])
    assert (status[:, list(NAN_LANES)] & 1).all() and not (status[:, healthy] & 1).any()
    assert np.isfinite(xs[:, healthy]).all()
    # ... and the rollout
    Xt, Yt, pst = d.empty(K + 1, B, 3), d.empty(K, B, 2), d.ints(K, B)
    Xt[0].copy_(d.t(inp["X0"]))
    U, W, V, P, TVP = (d.t(inp[k]) for k in ("U", "W", "V", "P", "TVP"))
    U0 = h(U).copy()
    sim.rollout_device(B, K, p(Xt), p(U), W_traj=p(W), V_traj=p(V), Y_traj=p(Yt), tvp_rows=p(TVP), p_loops=p(P), plant_status=p(pst))
    d.sync()
    assert same(h(Xt), xs), "X_traj"
    assert same(h(Yt), ys), "Y_traj"
    assert same(h(pst), ss), "status and step counts"
    assert same(h(U), U0), "an open-loop rollout wrote to U_traj"


# ---------------------------------------------------------------------------------------------- 3. plants with algebraic states
def dae_case(which, hostemu, B, K):
    """(simulator, inputs) of the DAE member of the probe family / the discrete oscillating-masses DAE"""
    if which == "family":
        sim = pf.make_simulator("dae", hostemu)
        base = pf.take(pf.draw(), slice(0, B))
        steps = [pf.take(pf.draw(seed=pf.SEED + 1 + k), slice(0, B)) for k in range(K)]
        return sim, {"X0": base["X"], "P": base["P"], "U": np.stack([s["U"] for s in steps]), "TVP": base["TVP"][:K].copy()}
    sim = ac.make_plant("oscillating_masses_dae", hostemu)
    rng = np.random.default_rng(5)
    X0 = np.asarray(CASES["oscillating_masses_dae"].X0, float)[None, :] * (1.0 + 0.3 * rng.standard_normal((B, 4)))
    return sim, {"X0": X0, "P": None, "U": rng.uniform(-1.0, 1.0, (K, B, 1)), "TVP": None}


def host_newton_z(model, x, u, tvp, pp, z_start):
    """z with alg(x, u, z, tvp, p, 0) = 0 by Newton's method on the model's own functions, stopped at a relative step of 1e-13"""
    ins = [model._x.cat, model._u.cat, model._z.cat, model._tvp.cat, model._p.cat, model._w.cat]
    jac = sym.Function("alg_jz", ins, [sym.jacobian(model._alg, model._z.cat)])
    z, w = np.array(z_start, float), np.zeros(model.n_w)
    for _ in range(30):
        a = np.asarray(model._alg_fun.eval(x, u, z, tvp, pp, w)[0], float).ravel()
        J = np.asarray(jac.eval(x, u, z, tvp, pp, w)[0], float).reshape(model.n_z, model.n_z, order="F")
        dz = np.linalg.solve(J, a)
        z = z - dz
        if np.max(np.abs(dz)) <= 1e-13 * max(1.0, np.max(np.abs(z))):
            return z
    raise AssertionError("the host Newton iteration did not converge")


def check_dae_plant(which, hostemu, B=65, K=5):
    d = Dev(hostemu)
    sim, inp = dae_case(which, hostemu, B, K)
    m = sim.model
    nx, nu, nz = m.n_x, m.n_u, m.n_z
    U = d.t(inp["U"])
    P = d.t(inp["P"]) if inp["P"] is not None else None
    TVP = d.t(inp["TVP"]) if inp["TVP"] is not None else None

    def launch(Xt, Zt, pst, k0, K_, reseed):
        sim.rollout_device(B, K_, p(Xt), p(U[k0]), Z_traj=p(Zt), tvp_rows=p(TVP[k0]) if TVP is not None else 0, p_loops=p(P),
                           plant_status=p(pst), reseed_z=reseed)
        d.sync()

    # one launch of K steps
    Xa, Za, sa = d.empty(K + 1, B, nx), d.empty(K, B, nz), d.ints(K, B)
    Xa[0].copy_(d.t(inp["X0"]))
    launch(Xa, Za, sa, 0, K, True)
    Xa, Za, sa = h(Xa), h(Za), h(sa)
    assert np.isfinite(Xa).all() and np.isfinite(Za).all() and not (sa & 1).any()
    # K launches of one step, the Newton starts carried from one to the next
    Xb, Zb, sb = d.empty(K + 1, B, nx), d.empty(K, B, nz), d.ints(K, B)
    Xb[0].copy_(d.t(inp["X0"]))
    for k in range(K):
        launch(Xb[k:k + 2], Zb[k:k + 1], sb[k:k + 1], k, 1, k == 0)
    assert same(h(Xb), Xa) and same(h(Zb), Za) and same(h(sb), sa), "one launch of K steps against K launches of one step"
    # K step-wise launches from a freshly seeded buffer
    sim.set_initial_guess()
    X, Xn, st = d.t(inp["X0"]), d.empty(B, nx), d.ints(B)
    dummy = d.t(np.zeros(1))
    for k in range(K):
        sim.step_batch_device(B, p(X), p(U[k]), p(TVP[k]) if TVP is not None else p(dummy), p(P) if P is not None else p(dummy), p(Xn), 0,
                              p(st), shared_mask=2 | 8 | 16 | (0 if P is not None else 4))
        d.sync()
        assert same(h(Xn), Xa[k + 1]) and same(h(st), sa[k]), ("step_batch_device", k)
        X, Xn = Xn, X
    # the algebraic states against the model's own equations.  Both Newton iterations stop at a relative step of 1e-13; 1e3 for conditioning
    worst = 0.0
    z0 = np.asarray(sim._z0.master, float)
    for k in range(K):
        for b in range(B):
            z = host_newton_z(m, Xa[k + 1, b], inp["U"][k, b], inp["TVP"][k] if inp["TVP"] is not None else np.zeros(0),
                              inp["P"][b] if inp["P"] is not None else np.zeros(0), z0)
            worst = max(worst, float(np.max(np.abs(Za[k, b] - z) / np.maximum(1.0, np.abs(z)))))
    print(f"DAE plant '{which}' B={B} K={K}: Z_traj against a host Newton solve of the model's alg, worst relative difference {worst:.3e}")
    assert worst <= 1e-10


# ---------------------------------------------------------------------------------------------- 4. the previous-input term
LB, UB = np.array([5.0, -8500.0]), np.array([60.0, 0.0])


def prev_input_case(hostemu, B, seed=23):
    """CSTR plant, random M, G and references with the clip; arrays with the loops innermost"""
    sim = ac.make_plant("CSTR", hostemu, varying=True)
    rng = np.random.default_rng(seed)
    X0 = np.asarray(CASES["CSTR"].X0, float) * (1.0 + 0.02 * rng.standard_normal((B, 4)))
    c = dict(X0=X0, x_ref=X0 * (1.0 + 0.01 * rng.standard_normal((B, 4))),
             u_ref=np.tile([50.0, -4000.0], (B, 1)) * (1.0 + 0.1 * rng.standard_normal((B, 2))),
             M=rng.standard_normal((B, 2, 4)) * np.array([[10.0], [500.0]]),
             G=rng.uniform(-0.5, 0.5, (B, 2, 2)) * np.array([[1.0, 0.01], [100.0, 1.0]]))
    c["up_ref"] = c["u_ref"] * (1.0 + 0.05 * rng.standard_normal((B, 2)))
    c["U_prev0"] = c["u_ref"] * (1.0 + 0.1 * rng.standard_normal((B, 2)))
    return sim, c


def hand_law(d, c, B):
    """-> (record, G, up_ref, the tensors that own the memory)"""
    keep = {"x_ref": d.t(c["x_ref"].T.copy()), "u_ref": d.t(c["u_ref"].T.copy()), "M": d.t(np.transpose(c["M"], (1, 2, 0)).copy()),
            "G": d.t(np.transpose(c["G"], (1, 2, 0)).copy()), "up_ref": d.t(c["up_ref"].T.copy()), "lb": d.t(LB), "ub": d.t(UB),
            "x_scale": d.t(np.ones(4))}
    rec = AffineLaw(x_ref=p(keep["x_ref"]), u_ref=p(keep["u_ref"]), M=p(keep["M"]), flags=None, lb=p(keep["lb"]), ub=p(keep["ub"]),
                    x_scale=p(keep["x_scale"]), ld=B, max_dx=float("inf"), clip=1, pad=0)
    return rec, keep["G"], keep["up_ref"], keep


def check_previous_input_term(hostemu, B=67, K=4):
    d = Dev(hostemu)
    sim, c = prev_input_case(hostemu, B)
    rec, G, up_ref, keep = hand_law(d, c, B)
    P, dummy = d.t(cstr_rows(sim, K)), d.t(np.zeros(1))

    def launch(X0, U_prev0, k0, K_, with_G=True):
        Xt, Ut, pst, lst = d.empty(K_ + 1, B, 4), d.empty(K_, B, 2), d.ints(K_, B), d.ints(K_, B)
        Xt[0].copy_(d.t(X0))
        Up = d.t(U_prev0)
        sim.rollout_device(B, K_, p(Xt), p(Ut), law=rec, G=p(G) if with_G else 0, up_ref=p(up_ref) if with_G else 0,
                           U_prev0=p(Up) if with_G else 0, tvp_rows=p(dummy), p_rows=p(P[k0]), plant_status=p(pst), law_status=p(lst))
        d.sync()
        return h(Xt), h(Ut), h(pst), h(lst)

    # one step against float64 numpy: an fma chain of nx + nu terms after one subtraction each, then the clip
    X1, U1, _, l1 = launch(c["X0"], c["U_prev0"], 0, 1)
    dx, dup = c["X0"] - c["x_ref"], c["U_prev0"] - c["up_ref"]
    u = c["u_ref"] + np.einsum("bik,bk->bi", c["M"], dx) + np.einsum("bij,bj->bi", c["G"], dup)
    bound = (4 + 2 + 2) * 2.0 ** -53 * (np.abs(c["u_ref"]) + np.einsum("bik,bk->bi", np.abs(c["M"]), np.abs(dx))
                                         + np.einsum("bij,bj->bi", np.abs(c["G"]), np.abs(dup)))
    err = np.abs(U1[0] - np.minimum(np.maximum(u, LB), UB))
    clipped = (u < LB) | (u > UB)
    print(f"previous-input term B={B}: |U - float64| / bound at most {np.max(err / bound):.3f}; {clipped.any(axis=1).sum()} of {B} loops clip")
    assert (err <= bound).all()
    assert 4 <= clipped.any(axis=1).sum() <= B - 4
    far = ~(np.abs(u - LB) <= bound).any(axis=1) & ~(np.abs(u - UB) <= bound).any(axis=1)      # (no entry within rounding of a bound)
    assert np.array_equal((l1[0][far] & 4) != 0, clipped.any(axis=1)[far])
    # the term matters: without it the inputs differ
    assert np.max(np.abs(np.einsum("bij,bj->bi", c["G"], dup)) / bound) > 1e6
    # K steps in one launch against K launches of one step that are handed the inputs applied before
    XK, UK, pK, lK = launch(c["X0"], c["U_prev0"], 0, K)
    assert not (pK & 1).any() and np.isfinite(XK).all()
    x, up = c["X0"], c["U_prev0"]
    for k in range(K):
        Xs, Us, ps_, ls_ = launch(x, up, k, 1)
        assert same(Xs[1], XK[k + 1]) and same(Us[0], UK[k]) and same(ps_[0], pK[k]) and same(ls_[0], lK[k]), k
        x, up = Xs[1], Us[0]
    assert ((lK[:-1] & 4) != 0).any(), "no clipped input is handed on to a next step"
    # G = null: the law of the law rollout
    Xn_, Un_, pn_, ln_ = launch(c["X0"], c["U_prev0"], 0, K, with_G=False)
    Xt, Ut, pst, lst = d.empty(K + 1, B, 4), d.empty(K, B, 2), d.ints(K, B), d.ints(K, B)
    Xt[0].copy_(d.t(c["X0"]))
    sim.rollout_affine_device(B, K, rec, p(Xt), p(Ut), p(dummy), p(P), p(pst), p(lst))
    d.sync()
    assert same(h(Xt), Xn_) and same(h(Ut), Un_) and same(h(pst), pn_) and same(h(lst), ln_)
    assert not same(Un_, UK)


# ---------------------------------------------------------------------------------------------- 5. the LQR loop
def lqr_case(name, hostemu):
    """-> (make_loop, B): make_loop() builds a fresh loop of the case (same controller, same plant object, its Newton starts re-seeded)"""
    dev = "cpu" if hostemu else 0
    if name in ("cstr_rate", "cstr_standard", "cstr_standard_far", "cstr_noise"):
        ex, plant, lqr = lc.example("cstr_lqr", hostemu, rate=not name.startswith("cstr_standard"))
        if name == "cstr_noise":
            plant = ex.build_model(process_noise=True)
        sim = lc.plant_on(ex.build_simulator(plant, setup=False), hostemu)
        lqr.set_setpoint(xss=ex.XSS, uss=ex.USS)
        B = 67
        # standard mode: starts within CSTR_STANDARD_START of the set-point (derived there); the others, and 'cstr_standard_far', within 1 %
        X0 = ex.XSS.ravel()[None, :] * (1.0 + (CSTR_STANDARD_START if name == "cstr_standard" else 0.01) * np.random.default_rng(8).uniform(-1, 1, (B, 4)))
        kw = {}
    elif name == "oscillating_masses":
        ex, plant, lqr = lc.example("oscillating_masses_lqr", hostemu)
        sim = lc.plant_on(ex.build_simulator(plant, setup=False), hostemu)
        B = 67
        X0 = ex.X0[None, :] * (1.0 + 0.3 * np.random.default_rng(9).uniform(-1, 1, (B, 4)))
        kw = {}
    elif name == "schedule":
        ex, plant, lqr = lc.example("cstr_lqr", hostemu)
        sim = lc.plant_on(ex.build_simulator(plant, setup=False), hostemu)
        B = 6
        X, U = lc.family_b_points(ex, B)
        g = lqr.gains_at(plant, X, U)
        assert np.all(g["status"] == 0)
        X0 = X * (1.0 + 0.01 * np.random.default_rng(3).uniform(-1, 1, X.shape))
        kw = dict(K=g["K"], XSS=X, USS=U, U_prev0=U)
    elif name == "batch_reactor_dae":
        model, lqr = ldc.design("batch_reactor", hostemu, setup=True)
        B = 6
        XSS, USS = ldc.steady_states(B)
        g = lqr.gains_at(model, XSS, USS)
        assert np.all(g["status"] == 0)
        sim = Simulator(model)
        sim.set_param(t_step=ldc.T_STEP)
        lc.plant_on(sim, hostemu)
        X0 = XSS + 0.2 * np.random.default_rng(4).uniform(-1, 1, XSS.shape)
        kw = dict(K=g["K"], XSS=XSS, USS=USS)
    elif name == "one_term":
        # standard mode, u = k_b (x_0 - xss_0): one term, uss = 0 (check_lqr_chunks_and_mixing)
        ex, plant, lqr = lc.example("oscillating_masses_lqr", hostemu, rate=False)
        sim = lc.plant_on(ex.build_simulator(plant, setup=False), hostemu)
        B = 67
        rng = np.random.default_rng(10)
        X0 = ex.X0[None, :] * (1.0 + 0.3 * rng.uniform(-1, 1, (B, 4)))
        Kb = np.zeros((B, 1, 4))
        Kb[:, 0, 0] = -rng.uniform(0.1, 0.5, B)
        kw = dict(K=Kb, XSS=rng.uniform(-1, 1, (B, 4)), USS=np.zeros((B, 1)))
    else:
        raise KeyError(name)

    def make_loop():
        if sim.model.n_z:
            sim.set_initial_guess()
        return BatchClosedLoopLQR(lqr, sim, X0, device=dev, **kw)
    return make_loop, B, sim


# The start of 'cstr_standard'.  The comparison of the inputs is RELATIVE (1e-12 of |u|, the project's measure: absolute below |u| = 1), and
# what separates the two paths is not only the order of the additions in one input (a few 1e-15 of |uss| = 18.6) but, from the second
# step on, the states the two runs have reached: they agree to a few units in the last place, ulp(400 K) = 5.7e-14, and the standard-mode
# gain of the example has |K| = 16.6 + 14.4 on the two temperatures - ONE ulp in both is 1.8e-12 in Q_J, whatever the code does.  A
# relative 1e-12 of Q_J can therefore hold only while |Q_J| stays of the order of its set-point value 18.6 (five ulp, a random walk
# over 20 steps, are 8.8e-12 = 1e-12 of |u| = 8.8); where a run takes Q_J through zero it asks for states equal to the bit, which two
# orders of additions cannot give.  With sum_j |K_2j| |xss_j| = 1.24e4 a start within 2.5e-4 of the set-point keeps |K (x - xss)| <= 3.1,
# so |Q_J| >= 15.4 at the start; check_lqr_fused asserts from the step-wise run, before it compares, that |Q_J| >= uss / 2 throughout.
# The starts within 1 % ('cstr_standard_far': Q_J passes through zero; measured there 1.8e-12 on the host emulation, 4.1e-12 on the
# MI355X) are checked by check_lqr_law_far: states to 1e-12, and both paths' inputs against the float64 law at their OWN states to the
# rounding bound of the chain - sharper than 1e-12 where it can be.
CSTR_STANDARD_START = 2.5e-4

LQR_CASES = ("cstr_rate", "cstr_standard", "oscillating_masses", "schedule", "batch_reactor_dae", "cstr_noise")


def noise_of(sim, B, n):
    """process noise that moves the states by about 1e-3 relative per step"""
    scale = np.array([1.6, 1.1, 400.0, 400.0]) * 1e-3 / float(sim.settings.t_step)
    return np.random.default_rng(12).standard_normal((n, B, 4)) * scale


def check_lqr_fused(name, hostemu, n=20):
    """run(n, fused=True) against run(n) of a fresh, identical loop: x and u to 1e-12 relative - the project's bound for the order of the
    additions in K (x - xss) (lqr_common.check_closed_loop_copies) -, the plant status equal.
    Measured on the host emulation (x, u): cstr_rate 9.3e-15, 5.3e-14; oscillating_masses 1.2e-15, 9.2e-16; schedule 7.8e-15, 8.9e-15;
    batch_reactor_dae 1.6e-15, 3.6e-15; cstr_noise 1.0e-14, 7.0e-14; cstr_standard (start: CSTR_STANDARD_START)
    3.4e-15, 2.4e-13.  On the MI355X: cstr_standard 3.3e-15, 2.9e-13, the others between 5e-16 and 1.1e-13."""
    make_loop, B, sim = lqr_case(name, hostemu)
    W = noise_of(sim, B, n) if name == "cstr_noise" else None
    step = make_loop().run(n, W=W)
    loop = make_loop()
    fused = loop.run(n, fused=True, W=W)
    assert fused["x"].shape == step["x"].shape == (n + 1, B, sim.model.n_x) and fused["u"].shape == step["u"].shape == (n, B, sim.model.n_u)
    assert fused["plant_status"].shape == step["plant_status"].shape == (n, B)
    ex_, eu_ = lc.relerr(fused["x"], step["x"]), lc.relerr(fused["u"], step["u"])
    print(f"LQR loop '{name}' B={B} n={n}: fused - step-wise: x {ex_:.3e}, u {eu_:.3e}")
    assert np.max(np.abs(step["x"][n] - step["x"][0])) > 0.0
    if W is not None:
        quiet = make_loop().run(n)
        assert lc.relerr(quiet["x"], step["x"]) > 1e-6           # (the noise is felt)
    if name == "cstr_standard":                                  # (what makes the relative bound one that can hold: CSTR_STANDARD_START)
        uss2 = float(np.asarray(CASES["cstr_lqr"].USS).ravel()[1])
        assert np.abs(step["u"][:, :, 1]).min() >= 0.5 * uss2 and np.max(np.abs(step["u"][1:] - step["u"][:-1])) > 1e-6
    assert ex_ <= 1e-12 and eu_ <= 1e-12
    assert np.array_equal(fused["plant_status"], step["plant_status"]) and not step["plant_status"].any()
    assert loop.k == n and same(h(loop.plant.X), fused["x"][n]) and same(h(loop.U), fused["u"][n - 1])


def check_lqr_law_far(hostemu, n=20):
    """cstr_lqr in standard mode from starts within 1 % of the set-point, where Q_J passes through zero (CSTR_STANDARD_START): the
    states of the fused and the step-wise run to 1e-12, equal plant status, and every input of either run against the float64 law
    uss + K (x - xss) at the states of ITS OWN run to the rounding bound of a sum of nx + 1 terms in any order,
    (nx + 2) 2^-53 (|uss| + sum |K| |x - xss|) - so that the difference of the two runs' inputs is K times the difference of their states"""
    make_loop, B, sim = lqr_case("cstr_standard_far", hostemu)
    step = make_loop().run(n)
    loop = make_loop()
    fused = loop.run(n, fused=True)
    K, xss, uss = (h(v).astype(np.float64) for v in (loop.K, loop.xss, loop.uss))
    assert np.abs(step["u"][:, :, 1]).min() < 1.0                # (the inputs do pass through zero)
    worst = 0.0
    for rec in (step, fused):
        dx = rec["x"][:-1] - xss[None]
        u64 = uss[None] + np.einsum("ik,nbk->nbi", K[0], dx)
        bound = (4 + 2) * 2.0 ** -53 * (np.abs(uss)[None] + np.einsum("ik,nbk->nbi", np.abs(K[0]), np.abs(dx)))
        worst = max(worst, float(np.max(np.abs(rec["u"] - u64) / bound)))
    ex_ = lc.relerr(fused["x"], step["x"])
    print(f"LQR loop 'cstr_standard_far' B={B} n={n}: fused - step-wise: x {ex_:.3e}, u {lc.relerr(fused['u'], step['u']):.3e} (not asserted: "
          f"Q_J passes through zero); |u - float64 law at the run's own states| / bound at most {worst:.3f}")
    assert worst <= 1.0 and ex_ <= 1e-12
    assert np.array_equal(fused["plant_status"], step["plant_status"]) and not step["plant_status"].any()


def same_run(a, b):
    return all(same(a[k], b[k]) for k in ("x", "u", "plant_status"))


def check_lqr_chunks_and_mixing(name, hostemu):
    """chunk = 3 with n = 7 equals one launch, bit for bit.  run(3, fused), step(), run(3, fused) against run(7, fused): k, the states,
    the inputs applied last and the plant's own buffers are where 7 fused steps leave them.  The step in the middle forms its input
    with torch (a product, then + uss), the law as an fma chain from u_ref: the SAME arithmetic - and then equal bits over all 7
    steps - exactly where the gain has one non-zero column and uss = 0 (one rounded product; products with 0 and sums with 0 are
    exact): the case 'one_term'.  With a full gain the two inputs differ by a rounding: the records are equal bit for bit up to
    the step, and to the 1e-12 of check_lqr_fused after it."""
    make_loop, B, sim = lqr_case(name, hostemu)
    whole = make_loop().run(7, fused=True)
    assert same_run(make_loop().run(7, fused=True, chunk=3), whole)
    loop = make_loop()
    a = loop.run(3, fused=True)
    r = {k: v.copy() for k, v in loop.step().items()}
    b = loop.run(3, fused=True)
    assert loop.k == 7
    mixed = {"x": np.concatenate([a["x"], r["x"][None], b["x"][1:]]), "u": np.concatenate([a["u"], r["u0"][None], b["u"]]),
             "plant_status": np.concatenate([a["plant_status"], r["plant_status"][None], b["plant_status"]])}
    print(f"LQR loop '{name}': run(3, fused), step(), run(3, fused) - run(7, fused): x {lc.relerr(mixed['x'], whole['x']):.3e}, "
          f"u {lc.relerr(mixed['u'], whole['u']):.3e}")
    head = lambda rec: {k: v[:3 + (k == "x")] for k, v in rec.items()}      # noqa: E731
    assert same_run(head(mixed), head(whole))
    if name == "one_term":
        assert same_run(mixed, whole)
    else:
        assert lc.relerr(mixed["x"], whole["x"]) <= 1e-12 and lc.relerr(mixed["u"], whole["u"]) <= 1e-12


# ---------------------------------------------------------------------------------------------- 6. simulate_batch
def check_simulate_batch(kind, hostemu, B=65, K=3):
    sim = pf.make_simulator(kind, hostemu)
    base = pf.take(pf.draw(), slice(0, B))
    steps = [pf.take(pf.draw(seed=pf.SEED + 1 + k), slice(0, B)) for k in range(K)]
    U, W, V = (np.stack([s[k] for s in steps]) for k in ("U", "W", "V"))
    t0, x0 = sim.t0.copy(), np.asarray(sim.x0.master, float).copy()
    r = sim.simulate_batch(base["X"], U, W=W, V=V, P=base["P"])
    assert np.array_equal(sim.t0, t0) and np.array_equal(sim.x0.master, x0)
    assert r["x"].shape == (K + 1, B, 3) and r["y"].shape == (K, B, 2) and r["z"].shape == (K, B, sim.model.n_z)
    assert r["status"].shape == r["n_steps"].shape == (K, B)
    sim.set_initial_guess()
    x = base["X"]
    tvp = np.asarray(sim.tvp_fun(0.0).master, float).reshape(-1)
    for k in range(K):
        s = sim.make_step_batch(x, U[k], P=base["P"], TVP=tvp, W=W[k], V=V[k], carry_z=True)
        assert same(s["x"], r["x"][k + 1]) and same(s["y"], r["y"][k]), k
        assert np.array_equal(s["status"], r["status"][k]) and np.array_equal(s["n_steps"], r["n_steps"][k]), k
        x = s["x"]
    assert not (r["status"] & 1).any() and (r["status"] & 2).any() and not (r["status"] & 2).all()
    # inputs shared by the batch = the same rows tiled
    shared = sim.simulate_batch(base["X"], U[:, 0], W=W[:, 0], V=V[:, 0], P=base["P"])
    tiled = sim.simulate_batch(base["X"], np.tile(U[:, :1], (1, B, 1)), W=np.tile(W[:, :1], (1, B, 1)), V=np.tile(V[:, :1], (1, B, 1)), P=base["P"])
    assert all(same(shared[k], tiled[k]) for k in ("x", "y", "z", "status", "n_steps"))
    assert not same(shared["x"], r["x"])


# ---------------------------------------------------------------------------------------------- 7. refusals
def _refused(call, words):
    try:
        call()
    except RuntimeError as e:
        assert all(w in str(e) for w in words), (str(e), words)
        return str(e)
    raise AssertionError(f"accepted: expected a refusal naming {words}")


def check_refusals(hostemu):
    """every refusal of dompc_plant_rollout_device by name: from C (return code 1 and the text of dompc_plant_last_error) and from
    Python (RuntimeError with that text); B <= 0 and K <= 0 return without a launch"""
    d = Dev(hostemu)
    B, K = 3, 2
    ode, dae, noin = pf.make_simulator("ode", hostemu), pf.make_simulator("dae", hostemu), ac.make_plant("CSTR", hostemu)
    Xt, Ut, dummy = d.empty(K + 1, B, 4), d.empty(K, B, 2), d.t(np.zeros(8))
    good = dict(tvp_rows=p(dummy), p_loops=p(dummy))
    cases = [
        (ode, dict(X_traj=0, U_traj=p(Ut), **good), ("X_traj",)),
        (ode, dict(X_traj=p(Xt), U_traj=0, **good), ("U_traj",)),
        (ode, dict(X_traj=p(Xt), U_traj=p(Ut), tvp_rows=p(dummy)), ("p_rows", "p_loops")),
        (ode, dict(X_traj=p(Xt), U_traj=p(Ut), tvp_rows=p(dummy), p_rows=p(dummy), p_loops=p(dummy)), ("p_rows", "p_loops", "both")),
        (ode, dict(X_traj=p(Xt), U_traj=p(Ut), p_loops=p(dummy)), ("tvp_rows",)),
        (ode, dict(X_traj=p(Xt), U_traj=p(Ut), Z_traj=p(dummy), **good), ("Z_traj", "algebraic states")),
    ]
    _, c = prev_input_case(hostemu, B)
    rec, G, up_ref, keep = hand_law(d, c, B)
    cstr = dict(X_traj=p(Xt), U_traj=p(Ut), p_rows=p(dummy))
    cases += [
        (noin, dict(law=rec, G=p(G), U_prev0=p(dummy), **cstr), ("G", "up_ref")),
        (noin, dict(law=rec, G=p(G), up_ref=p(up_ref), **cstr), ("G", "U_prev0")),
    ]
    for field in ("x_ref", "u_ref", "M", "x_scale", "lb", "ub"):
        bad = AffineLaw.from_buffer_copy(rec)
        setattr(bad, field, None)
        cases.append((noin, dict(law=bad, **cstr), ("incomplete law",)))
    small = AffineLaw.from_buffer_copy(rec)
    small.ld = B - 1
    cases.append((noin, dict(law=small, **cstr), ("incomplete law", "ld")))
    # a plant without inputs
    from do_mpc_amd import Model
    m0 = Model("discrete")
    x = m0.set_variable("_x", "x", (2, 1))
    m0.set_rhs("x", 0.5 * x)
    m0.setup()
    s0 = Simulator(m0)
    s0.set_param(t_step=1.0)
    lc.plant_on(s0, hostemu)
    cases.append((s0, dict(law=rec, X_traj=p(Xt), U_traj=p(Ut)), ("law", "without inputs")))
    for sim, kw, words in cases:
        kw = dict(kw)
        X_traj, U_traj = kw.pop("X_traj"), kw.pop("U_traj")
        text = _refused(lambda: sim.rollout_device(B, K, X_traj, U_traj, **kw), ("dompc_plant_rollout_device",) + words)
        # ... and from C
        r = RolloutDesc()
        law = kw.pop("law", None)
        r.law = C.addressof(law) if law is not None else None
        r.X_traj, r.U_traj = X_traj or None, U_traj or None
        for k, v in kw.items():
            setattr(r, k, v or None)
        assert sim._lib.dompc_plant_rollout_device(sim._h, B, K, C.byref(r), None) == 1
        assert sim._lib.dompc_plant_last_error(sim._h).decode() in text
    # nothing to do: no launch, no refusal, whatever the description holds
    for b_, k_ in ((0, K), (B, 0), (-1, -1)):
        ode.rollout_device(b_, k_, 0, 0)
    # the law rollout still refuses plants with algebraic states, the general one serves them (check_dae_plant)
    try:
        dae.rollout_affine_device(1, 1, rec, 0, 0)
    except NotImplementedError as e:
        assert "algebraic states" in str(e)
    else:
        raise AssertionError("a DAE plant was accepted by Simulator.rollout_affine_device")
