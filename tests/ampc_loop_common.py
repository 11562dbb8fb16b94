"""TEST-ONLY checks of the fused approximate-MPC loop (csrc/dompc_ampc_loop.hip: dompc_ampc_loop_kernel; Simulator.rollout_ampc_device,
BatchClosedLoopAMPC.run(fused=True)), shared by the CPU suite (host emulation: "device" memory = host memory) and the GPU suite - each
check with a `hostemu=` switch.

The reference of every comparison is the step-wise path: `ApproxMPC.make_step_batch_device` then `Simulator.step_batch_device` per
control step, or `BatchClosedLoopAMPC.step()`.  Both paths run the same functions on the same operands, so the comparison is equal
bits (`rollout_common.same`) - states, inputs, measurements, algebraic states and the status words with their step counts.  No
tolerance anywhere.  The step-wise network is pinned to its float64 twin by tests/ampc_common.py, the step-wise plant to closed forms
and to scipy by tests/plant_family_common.py and tests/simulator_common.py."""
import ctypes as C

import numpy as np
import torch

import ampc_common as amc
import asmpc_common as ac
import plant_family_common as pf
import rollout_common as rc
from ampc_loop_hostemu import on_pairs
from do_mpc_amd.closed_loop import BatchClosedLoopAMPC
from do_mpc_amd.simulator import AmpcLoopDesc
from rollout_common import Dev, h, p, same

PAD = 64                          # rows behind the last record of every buffer: must stay as they were filled
FAMILY_BOX = dict(lbx=[-2.0] * 3, ubx=[2.0] * 3, lbu=[-1.0], ubu=[1.0])      # outputs inside the |u| <= 1 of plant_family_common.draw
FAMILY_NET = dict(n_hidden_layers=1, n_neurons=33, act_fn="tanh", output_act_fn="linear")
# the prebuilt pairs (__graft_entry__.PREBUILT_AMPC_LOOP): plant, then the network as (nx, nu, rterm, settings)
PAIRS = {
    1: ("CSTR", "stored"),
    2: ("CSTR", (4, 2, True, dict(n_hidden_layers=3, n_neurons=128, act_fn="leaky_relu", output_act_fn="tanh"))),
    3: ("CSTR", (4, 2, False, dict(n_hidden_layers=0, n_neurons=2, act_fn="tanh", output_act_fn="linear"))),
    4: ("dae", (3, 1, True, FAMILY_NET)),
    5: ("discrete", (3, 1, True, FAMILY_NET)),
}


def pair(n, hostemu, family=None):
    """(simulator, network) of prebuilt pair n; `family`: a member of ampc_common.FAMILY on the CSTR instead (host emulation)"""
    plant, net = PAIRS[n]
    if family is not None:
        net = family
    sim = ac.make_plant("CSTR", hostemu, varying=True) if plant == "CSTR" else pf.make_simulator(plant, hostemu)
    on_pairs(sim, hostemu)
    if net == "stored":
        return sim, amc.stored_cstr(hostemu)
    nx, nu, rterm, st = net
    if plant == "CSTR":
        return sim, amc.network(nx, nu, rterm, hostemu, seed=3, box=amc.CSTR_BOX, **st)
    # (the seed at which torch's initial weights put the inputs of the family's draws on both sides of the lower bound: check_family asserts it)
    return sim, amc.network(nx, nu, rterm, hostemu, seed=7, box=FAMILY_BOX, **st)


def cstr_case(sim, ampc, B, K, seed=1, spread=1.5):
    """starts (and previous inputs) up to `spread` x the network's box, the CSTR's parameter rows of the K loop times"""
    X0, Up0 = amc.inputs(ampc, B, seed=seed, spread=spread)
    return {"X0": X0, "Up0": Up0, "P_rows": rc.cstr_rows(sim, K)}


def family_case(B, K, ampc):
    """the draws of rollout_common.open_loop_inputs: per-loop parameters with lanes that turn stiff and the lanes NAN_LANES that fail,
    noise of a draw of its own per step, the time-varying parameter shared by the batch; previous inputs inside the output box"""
    inp = rc.open_loop_inputs(B, K)
    return {"X0": inp["X0"], "Up0": 0.5 * inp["U"][0] if ampc.rterm else None, "P_loops": inp["P"], "W": inp["W"], "V": inp["V"],
            "TVP": inp["TVP"]}


def at(c, k0, K, X0=None, Up0=None):
    """the case from step k0 on for K steps, from the given state and previous inputs"""
    out = dict(c)
    for k in ("W", "V", "TVP", "P_rows"):
        if c.get(k) is not None:
            out[k] = c[k][k0:k0 + K]
    if X0 is not None:
        out["X0"] = X0
    if Up0 is not None:
        out["Up0"] = Up0
    return out


def _dev(d, c):
    return {k: (d.t(c[k]) if c.get(k) is not None else None) for k in ("W", "V", "TVP", "P_rows", "P_loops", "Up0")}


def stepwise(d, sim, ampc, c, K, y=False, clip=True):
    """K pairs of launches make_step_batch_device, step_batch_device -> x [K + 1][B][nx], u [K][B][nu], status words [K][B], y [K][B][ny]"""
    m = sim.model
    B = c["X0"].shape[0]
    t = _dev(d, c)
    X, Xn, Un, Y, st = d.t(c["X0"]), d.empty(B, m.n_x), d.empty(B, m.n_u), d.empty(B, max(m.n_y, 1)), d.ints(B)
    U = t["Up0"] if t["Up0"] is not None else d.empty(B, m.n_u)
    dummy = d.t(np.zeros(8))
    xs, us, ss, ys = [h(X).copy()], [], [], []
    for k in range(K):
        ampc.make_step_batch_device(B, p(X), p(U) if ampc.rterm else 0, p(Un), clip_to_bounds=clip)
        U, Un = Un, (U if U is not t["Up0"] else d.empty(B, m.n_u))
        per_loop = t["P_loops"] is not None
        pp = t["P_loops"] if per_loop else (t["P_rows"][k] if t["P_rows"] is not None else dummy)
        sim.step_batch_device(B, p(X), p(U), p(t["TVP"][k]) if t["TVP"] is not None else p(dummy), p(pp), p(Xn), p(Y) if y else 0, p(st),
                              w=p(t["W"][k]) if t["W"] is not None else 0, v=p(t["V"][k]) if t["V"] is not None else 0,
                              shared_mask=2 | (0 if per_loop else 4) | (0 if t["W"] is not None else 8) | (0 if t["V"] is not None else 16))
        d.sync()
        xs.append(h(Xn).copy()); us.append(h(U).copy()); ss.append(h(st).copy()); ys.append(h(Y).copy())
        X, Xn = Xn, X
    return {"x": np.stack(xs), "u": np.stack(us), "status": np.stack(ss), "y": np.stack(ys)}


def fused(d, sim, ampc, c, K, y=False, z=False, clip=True, reseed=False):
    """one launch of K steps into buffers filled with NaN / -1 and PAD rows longer than the records; asserts that the rows behind the
    records are as they were filled"""
    m = sim.model
    B = c["X0"].shape[0]
    t = _dev(d, c)
    Xf, Uf, sf = d.empty((K + 1) * B + PAD, m.n_x), d.empty(K * B + PAD, m.n_u), d.ints(K * B + PAD)
    Yf = d.empty(K * B + PAD, max(m.n_y, 1)) if y else None
    Zf = d.empty(K * B + PAD, max(m.n_z, 1)) if z else None
    Xf[:B].copy_(d.t(c["X0"]))
    sim.rollout_ampc_device(ampc, B, K, p(Xf), p(Uf), U_prev0=p(t["Up0"]), W_traj=p(t["W"]), V_traj=p(t["V"]), Y_traj=p(Yf), Z_traj=p(Zf),
                            tvp_rows=p(t["TVP"]), p_rows=p(t["P_rows"]), p_loops=p(t["P_loops"]), plant_status=p(sf), clip_to_bounds=clip,
                            reseed_z=reseed)
    d.sync()
    out = {"x": h(Xf)[:(K + 1) * B].reshape(K + 1, B, m.n_x), "u": h(Uf)[:K * B].reshape(K, B, m.n_u), "status": h(sf)[:K * B].reshape(K, B)}
    assert np.isnan(h(Xf)[(K + 1) * B:]).all() and np.isnan(h(Uf)[K * B:]).all() and (h(sf)[K * B:] == -1).all(), "rows behind the records were written"
    if y:
        out["y"] = h(Yf)[:K * B].reshape(K, B, -1)
        assert np.isnan(h(Yf)[K * B:]).all()
    if z:
        out["z"] = h(Zf)[:K * B].reshape(K, B, -1)
        assert np.isnan(h(Zf)[K * B:]).all()
    return out


def assert_same(a, b, keys=("x", "u", "status"), what=""):
    for k in keys:
        assert same(a[k], b[k]), (what, k)


# ---------------------------------------------------------------------------------------------- 1. lane layout
LANE_B = (5, 33, 65, 97)


def check_lane_layout(hostemu, B, K=4):
    """pair 1 with the stored network, previous inputs given, starts beyond the box so that some inputs clip"""
    d = Dev(hostemu)
    sim, ampc = pair(1, hostemu)
    c = cstr_case(sim, ampc, B, K)
    ref = stepwise(d, sim, ampc, c, K)
    lbu, ubu = np.asarray(amc.CSTR_BOX["lbu"]), np.asarray(amc.CSTR_BOX["ubu"])
    on_bound = (ref["u"] == lbu) | (ref["u"] == ubu)
    assert on_bound.any(), "no input clips"
    assert (~on_bound & np.isfinite(ref["u"])).any(), "every input clips"
    assert ((ref["u"] >= lbu) & (ref["u"] <= ubu)).all()
    assert all(np.max(np.abs(ref["u"][k + 1] - ref["u"][k])) > 0.0 for k in range(K - 1)), "the inputs do not change from step to step"
    assert np.max(np.abs(ref["x"][K] - ref["x"][0])) > 0.0
    got = fused(d, sim, ampc, c, K)
    print(f"lane layout B={B} K={K}: {on_bound.any(axis=2).sum()} of {K * B} steps clip, plant steps {(ref['status'] >> 8).min()} .. "
          f"{(ref['status'] >> 8).max()}, failed {(ref['status'] & 1).sum()}")
    assert_same(got, ref, what=f"B={B}")


# ---------------------------------------------------------------------------------------------- 2. previous inputs
def check_previous_inputs(hostemu, B=37, K=4):
    d = Dev(hostemu)
    sim, ampc = pair(1, hostemu)
    c = cstr_case(sim, ampc, B, K, seed=2)
    whole = fused(d, sim, ampc, c, K)
    assert_same(whole, stepwise(d, sim, ampc, c, K))
    # other previous inputs, other inputs at k = 0
    other = fused(d, sim, ampc, at(c, 0, K, Up0=c["Up0"][::-1].copy()), K)
    assert not same(other["u"][0], whole["u"][0])
    # K launches of one step, each handed the inputs applied before
    x, up = c["X0"], c["Up0"]
    for k in range(K):
        one = fused(d, sim, ampc, at(c, k, 1, X0=x, Up0=up), 1)
        assert same(one["x"][1], whole["x"][k + 1]) and same(one["u"][0], whole["u"][k]) and same(one["status"][0], whole["status"][k]), k
        x, up = one["x"][1], one["u"][0]
    lbu, ubu = np.asarray(amc.CSTR_BOX["lbu"]), np.asarray(amc.CSTR_BOX["ubu"])
    assert ((whole["u"][:-1] == lbu) | (whole["u"][:-1] == ubu)).any(), "no clipped input is handed on to a next step"
    # no rterm: U_prev0 = 0
    sim3, ampc3 = pair(3, hostemu)
    c3 = cstr_case(sim3, ampc3, B, K, seed=2, spread=1.0)
    assert c3["Up0"] is None and not ampc3.rterm
    assert_same(fused(d, sim3, ampc3, c3, K), stepwise(d, sim3, ampc3, c3, K), what="pair 3")


# ---------------------------------------------------------------------------------------------- 3. shapes
def check_shape(hostemu, n, B=67, K=3, family=None):
    d = Dev(hostemu)
    sim, ampc = pair(n, hostemu, family=family)
    c = cstr_case(sim, ampc, B, K, seed=5, spread=1.0)
    # with torch's initial weights a small output range lies on one side of a bound (pair 2: every input clips to lbu): the unclipped
    # run is the one whose inputs move with the states
    for clip in (True, False):
        ref = stepwise(d, sim, ampc, c, K, clip=clip)
        assert np.isfinite(ref["u"]).all() and np.isfinite(ref["x"]).all()
        if not clip:
            assert np.max(np.abs(ref["u"][1] - ref["u"][0])) > 0.0 and len(np.unique(ref["u"][0, :, 0])) > B // 2
        assert_same(fused(d, sim, ampc, c, K, clip=clip), ref, what=f"pair {n} clip={clip}")


# ---------------------------------------------------------------------------------------------- 4. unequal work, noise, per-loop parameters, DAE
def check_family(hostemu, n, B=65, K=3):
    """pair 4 (DAE member of the probe family) or 5 (discrete): lanes of one wavefront that take different numbers of plant steps, lanes
    that fall back to the implicit method, lanes that fail; process and measurement noise, measurements, parameters per loop"""
    d = Dev(hostemu)
    sim, ampc = pair(n, hostemu)
    m = sim.model
    dae = m.n_z > 0
    c = family_case(B, K, ampc)
    sim.set_initial_guess()
    ref = stepwise(d, sim, ampc, c, K, y=True)
    status, steps = ref["status"] & 0xFF, ref["status"] >> 8
    healthy = np.setdiff1d(np.arange(64), rc.NAN_LANES)
    if m.model_type == "discrete":
        assert (steps == 1).all() and not (status[:, healthy] & 1).any()
    else:
        assert any(len(set(steps[k, healthy])) > 1 for k in range(K)), "no step in which two lanes of the first wavefront differ in their step count"
        assert ((status & 2) != 0).any() and ((status[:, healthy] & 2) == 0).any(), "implicit and explicit lanes"
        assert (status[:, list(rc.NAN_LANES)] & 1).all() and not (status[:, healthy] & 1).any()
    assert np.isfinite(ref["x"][:, healthy]).all() and np.max(np.abs(ref["u"][1] - ref["u"][0])) > 0.0
    lbu, ubu = np.asarray(FAMILY_BOX["lbu"]), np.asarray(FAMILY_BOX["ubu"])
    assert (np.isnan(ref["u"]) | ((ref["u"] >= lbu) & (ref["u"] <= ubu))).all()
    on_bound = (ref["u"] == lbu) | (ref["u"] == ubu)
    assert on_bound.sum() >= 8 and (~on_bound).sum() >= 8, "inputs on a bound and inputs inside the box"
    print(f"pair {n} B={B} K={K}: plant steps {steps.min()} .. {steps.max()}, implicit lanes per step {((status & 2) != 0).sum(axis=1)}, "
          f"failed lanes per step {(status & 1).sum(axis=1)}, NaN inputs {np.isnan(ref['u']).sum()}")
    sim.set_initial_guess()
    got = fused(d, sim, ampc, c, K, y=True, z=dae)
    assert_same(got, ref, keys=("x", "u", "status", "y"), what=f"pair {n}")
    if dae:
        # the algebraic states: the step-wise launches keep them in the handle; the general rollout, one step per launch with the
        # inputs of the step-wise run, writes them out (rollout_common.check_dae_plant pins it to step_batch_device)
        sim.set_initial_guess()
        t = _dev(d, c)
        U = d.t(ref["u"])
        Xt, Zt, Yt, st = d.empty(K + 1, B, m.n_x), d.empty(K, B, m.n_z), d.empty(K, B, m.n_y), d.ints(K, B)
        Xt[0].copy_(d.t(c["X0"]))
        for k in range(K):
            sim.rollout_device(B, 1, p(Xt[k:k + 2]), p(U[k]), W_traj=p(t["W"][k]), V_traj=p(t["V"][k]), Y_traj=p(Yt[k]), Z_traj=p(Zt[k]),
                               tvp_rows=p(t["TVP"][k]), p_loops=p(t["P_loops"]), plant_status=p(st[k]))
            d.sync()
        assert same(h(Xt), ref["x"]) and same(h(st), ref["status"]) and same(h(Yt), ref["y"])
        assert same(got["z"], h(Zt)), "Z_traj"
        assert np.isfinite(got["z"][:, healthy]).all()


# ---------------------------------------------------------------------------------------------- 5. the loop
def loop_case(n, hostemu, B=37):
    """-> (make_loop, simulator, network, noise [7][B][nw] or None, per-loop parameters)"""
    sim, ampc = pair(n, hostemu)
    dev = "cpu" if hostemu else 0
    if n == 1:
        X0, Up0 = amc.inputs(ampc, B, seed=7, spread=1.5)
        W = None
        rng = np.random.default_rng(13)
        P = np.asarray(sim.p_fun(0.0).master, float).reshape(1, -1) * (1.0 + 0.05 * rng.uniform(-1, 1, (B, sim.model.n_p)))
    else:
        B = 65
        inp = rc.open_loop_inputs(B, 7)
        X0, Up0, W, P = inp["X0"], 0.5 * inp["U"][0], inp["W"], inp["P"]

    def make_loop():
        if sim.model.n_z:
            sim.set_initial_guess()
        return BatchClosedLoopAMPC(ampc, sim, X0, U_prev0=Up0, device=dev)
    return make_loop, sim, ampc, W, P


def same_run(a, b):
    return all(same(a[k], b[k]) for k in ("x", "u", "plant_status"))


def where_it_belongs(loop, rec, n):
    return loop.k == n and same(h(loop.plant.X), rec["x"][n]) and same(h(loop.U), rec["u"][n - 1])


def relerr(a, b):
    ok = np.isfinite(a) & np.isfinite(b)
    return float(np.max(np.abs(a - b)[ok] / np.maximum(1.0, np.abs(b[ok]))))


def check_loop(hostemu, n):
    make_loop, sim, ampc, W, P = loop_case(n, hostemu)
    # pair 4: the family's p_fun is the zero template - the loop runs on the per-loop parameters throughout
    base = dict(P=P) if n != 1 else {}
    ref_loop = make_loop()
    step = ref_loop.run(7, **base)
    B = ref_loop.B
    assert step["x"].shape == (8, B, sim.model.n_x) and step["u"].shape == (7, B, sim.model.n_u) and step["plant_status"].shape == (7, B)
    assert np.max(np.abs(step["u"][1:] - step["u"][:-1])[np.isfinite(step["u"][1:] - step["u"][:-1])]) > 0.0
    loop = make_loop()
    whole = loop.run(7, fused=True, **base)
    assert same_run(whole, step), "run(7, fused=True) against run(7)"
    assert where_it_belongs(loop, whole, 7) and same(h(loop.plant.pstat), h(ref_loop.plant.pstat))
    loop = make_loop()
    assert same_run(loop.run(7, fused=True, chunk=3, **base), whole), "chunk = 3"
    assert where_it_belongs(loop, whole, 7) and same(h(loop.plant.pstat), h(ref_loop.plant.pstat))
    loop = make_loop()
    a = loop.run(3, fused=True, **base)
    assert where_it_belongs(loop, a, 3)
    r = {k: v.copy() for k, v in loop.step().items()}
    assert loop.k == 4
    b = loop.run(3, fused=True)
    mixed = {"x": np.concatenate([a["x"], r["x"][None], b["x"][1:]]), "u": np.concatenate([a["u"], r["u0"][None], b["u"]]),
             "plant_status": np.concatenate([a["plant_status"], r["plant_status"][None], b["plant_status"]])}
    assert same_run(mixed, whole), "run(3, fused), step(), run(3, fused) against run(7, fused)"
    assert where_it_belongs(loop, whole, 7) and same(h(loop.plant.pstat), h(ref_loop.plant.pstat))
    # parameters per loop and process noise: felt, and equal on both paths
    if n == 1:
        sp, fp = make_loop().run(7, P=P), make_loop().run(7, fused=True, P=P)
        print(f"loop pair {n}: per-loop parameters move the states by {relerr(sp['x'], step['x']):.3e}")
        assert relerr(sp["x"], step["x"]) > 1e-6 and same_run(fp, sp)
    else:
        quiet_p = make_loop().run(7)
        assert relerr(quiet_p["x"], step["x"]) > 1e-6
        sw, fw = make_loop().run(7, W=W, P=P), make_loop().run(7, fused=True, W=W, P=P)
        fc = make_loop().run(7, fused=True, chunk=3, W=lambda k: W[k], P=P)
        print(f"loop pair {n}: process noise moves the states by {relerr(sw['x'], step['x']):.3e}")
        assert relerr(sw["x"], step["x"]) > 1e-6 and same_run(fw, sw) and same_run(fc, sw)


def check_closed_loop_copies(hostemu, n_steps=7, B=5):
    """ampc_common.check_closed_loop with fused=True: B copies of one start give B identical trajectories, each the single loop
    ampc.make_step -> simulator.make_step"""
    from do_mpc_amd.examples import cstr_ampc as ex
    from lqr_common import plant_on
    ampc = amc.stored_cstr(hostemu)
    sim = on_pairs(plant_on(ex.build_simulator(ex.build_model(), setup=False), hostemu), hostemu)
    sim.x0 = ex.X0
    ampc.u0 = ex.U0.reshape(-1, 1)
    loop = BatchClosedLoopAMPC(ampc, sim, np.tile(ex.X0, (B, 1)), device="cpu" if hostemu else 0)
    rec = loop.run(n_steps, fused=True)
    assert rec["x"].shape == (n_steps + 1, B, 4) and rec["u"].shape == (n_steps, B, 2) and not rec["plant_status"].any()
    for b in range(1, B):
        assert np.array_equal(rec["x"][:, b], rec["x"][:, 0]) and np.array_equal(rec["u"][:, b], rec["u"][:, 0])
    x0 = ex.X0.reshape(-1, 1)
    for k in range(n_steps):
        u0 = ampc.make_step(x0)
        x0 = sim.make_step(u0)
        assert np.array_equal(u0.ravel(), rec["u"][k, 0]) and np.array_equal(np.asarray(x0).ravel(), rec["x"][k + 1, 0])


# ---------------------------------------------------------------------------------------------- 6. weights are data
def check_weights_are_data(hostemu, B=33, K=3):
    d = Dev(hostemu)
    sim, ampc = pair(1, hostemu)
    c = cstr_case(sim, ampc, B, K, seed=4, spread=1.0)
    first = fused(d, sim, ampc, c, K)
    assert_same(first, stepwise(d, sim, ampc, c, K))
    nat = sim._pairs[ampc.model_hash]
    handle = nat.h.value
    with torch.no_grad():
        ampc.net.layers[2].weight[1, 7] += 0.25
    changed = fused(d, sim, ampc, c, K)
    assert not same(changed["u"], first["u"]) and not same(changed["x"], first["x"])
    assert_same(changed, stepwise(d, sim, ampc, c, K), what="after the in-place change")
    ampc.load_from_state_dict(amc.STORED)
    again = fused(d, sim, ampc, c, K)
    assert_same(again, stepwise(d, sim, ampc, c, K), what="after load_from_state_dict")
    assert_same(again, first) and not same(again["u"], changed["u"])
    assert sim._pairs[ampc.model_hash] is nat and nat.h.value == handle, "the pair's handle was rebuilt"


# ---------------------------------------------------------------------------------------------- 7. refusals
def check_refusals(hostemu):
    """every refusal of dompc_plant_ampc_loop_device by name: from C (return code 1 and the text of dompc_plant_last_error) and from
    Python (RuntimeError with that text); B <= 0 and K <= 0 return without a launch"""
    d = Dev(hostemu)
    B, K = 3, 2
    sim4, ampc4 = pair(4, hostemu)               # _p, _tvp, algebraic states, rterm
    sim5, ampc5 = pair(5, hostemu)               # no algebraic states
    sim1, ampc1 = pair(1, hostemu)
    Xt, Ut, dummy = d.empty(K + 1, B, 4), d.empty(K, B, 2), d.t(np.zeros(16))
    good = dict(X_traj=p(Xt), U_traj=p(Ut), U_prev0=p(dummy), tvp_rows=p(dummy), p_loops=p(dummy))
    rest = {k: v for k, v in good.items() if k not in ("X_traj", "U_traj")}
    cases = [
        (sim4, ampc4, dict(good, X_traj=0), ("X_traj",)),
        (sim4, ampc4, dict(good, U_traj=0), ("U_traj",)),
        (sim4, ampc4, dict(good, p_loops=0), ("p_rows", "p_loops")),
        (sim4, ampc4, dict(good, p_rows=p(dummy)), ("p_rows", "p_loops", "both")),
        (sim4, ampc4, dict(good, tvp_rows=0), ("tvp_rows",)),
        (sim5, ampc5, dict(good, Z_traj=p(dummy)), ("Z_traj", "algebraic states")),
        (sim4, ampc4, dict(good, U_prev0=0), ("rterm", "U_prev0")),
    ]

    def desc_of(sim, ampc, kw, **shape):
        r = AmpcLoopDesc()
        r.w, r.par = ampc.device_weights()
        for k, v in {**ampc.shape_fields(), **shape}.items():
            setattr(r, k, v)
        r.clip = 1
        for k, v in kw.items():
            setattr(r, k, v or None)
        return r

    def from_c(nat, r, text):
        assert nat.lib.dompc_plant_ampc_loop_device(nat.h, B, K, C.byref(r), None) == 1
        assert nat.lib.dompc_plant_last_error(nat.h).decode() in text, (nat.lib.dompc_plant_last_error(nat.h).decode(), text)

    for sim, ampc, kw, words in cases:
        kw = dict(kw)
        X_traj, U_traj = kw.pop("X_traj"), kw.pop("U_traj")
        text = rc._refused(lambda: sim.rollout_ampc_device(ampc, B, K, X_traj, U_traj, **kw), ("dompc_plant_ampc_loop_device",) + words)
        from_c(sim._pair(ampc), desc_of(sim, ampc, dict(kw, X_traj=X_traj, U_traj=U_traj)), text)
    # a network of other sizes: n_out != nu (the CSTR's network on the family plant), n_in neither nx nor nx + nu
    text = rc._refused(lambda: sim4.rollout_ampc_device(ampc1, B, K, p(Xt), p(Ut), **rest),
                       ("dompc_plant_ampc_loop_device", "n_out", "nu"))
    from_c(sim4._pair(ampc4), desc_of(sim4, ampc4, good, n_out=2), text)
    odd5 = amc.network(5, 1, False, hostemu, seed=3, **FAMILY_NET)        # n_in = 5: neither 3 nor 4
    text = rc._refused(lambda: sim4.rollout_ampc_device(odd5, B, K, p(Xt), p(Ut), **rest),
                       ("dompc_plant_ampc_loop_device", "n_in", "nx"))
    from_c(sim4._pair(ampc4), desc_of(sim4, ampc4, good, n_in=5), text)
    # a handle whose code object has no loop kernel: the plant's own
    keep = dict(sim5._pairs)
    try:
        sim5._pairs[ampc5.model_hash] = sim5._native
        text = rc._refused(lambda: sim5.rollout_ampc_device(ampc5, B, K, p(Xt), p(Ut), **rest),
                           ("dompc_plant_ampc_loop_device", "no loop kernel"))
        from_c(sim5._native, desc_of(sim5, ampc5, good), text)
    finally:
        sim5._pairs.clear()
        sim5._pairs.update(keep)
    # nothing to do: no launch, no refusal, whatever the description holds
    for b_, k_ in ((0, K), (B, 0), (-1, -1)):
        sim4.rollout_ampc_device(ampc4, b_, k_, 0, 0)
        nat = sim4._pair(ampc4)
        assert nat.lib.dompc_plant_ampc_loop_device(nat.h, b_, k_, None, None) == 0
    # a controller of other sizes than the plant's is refused by the loop as before
    try:
        BatchClosedLoopAMPC(ampc1, sim4, np.zeros((B, 3)), device="cpu" if hostemu else 0)
    except AssertionError as e:
        assert "share states and inputs" in str(e)
    else:
        raise AssertionError("a controller of other sizes was accepted by BatchClosedLoopAMPC")
