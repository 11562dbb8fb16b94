"""Rate of the time-varying LQR along trajectories (LQR.gains_along_device: csrc/dompc_lqr.hip, dompc_lqr_pairs_kernel and
dompc_lqr_tv_kernel) on resident inputs, B = 16 384 trajectories of K = 20 knots, for the CSTR (continuous: zero-order hold per knot,
standard mode) and the oscillating masses (discrete, rate mode): trajectories per second, split into the pairs launch and the
recursion launch; beside it gains_at_device on the same B K knots (the frozen gain schedule, infinite horizon: what the project
could do before) and the numpy twin on one core.  Then the loop on the CSTR transition of examples/cstr_tracking.py:
BatchClosedLoopTVLQR.run(20, fused=True) against its own step() path, both with their copies, and the tracking error of the
time-varying gains against the frozen schedule over the same starts.  The variants of a group are timed in alternating rounds
(device events around each round); the figure is the median round.
usage: python tools/gpu_lqr_tv_rate.py [--batch 16384] [--steps 20] [--rounds 7] [--twin 4] > profiles/lqr_tv_rate.txt"""
import argparse
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import lqr_common as lc
import lqr_tv_common as tc
from do_mpc_amd.closed_loop import BatchClosedLoopTVLQR
from do_mpc_amd.examples import cstr_tracking as ct

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--twin", type=int, default=4)
args = ap.parse_args()
dev = torch.device("cuda", 0)
t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), device=dev)      # noqa: E731
e = lambda *s, dt=torch.float64: torch.empty(s, dtype=dt, device=dev)      # noqa: E731
B, K = args.batch, args.steps
rng = np.random.default_rng(1)
stream = torch.cuda.current_stream().cuda_stream


def alternating(variants, rounds, per_round):
    """{name: median seconds per launch}: rounds of `per_round` launches of each variant in turn, device events around each round"""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per_round):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e-3 / per_round)
    return {k: float(np.median(v)) for k, v in out.items()}


print(f"# tools/gpu_lqr_tv_rate.py --batch {B} --steps {K} --rounds {args.rounds} --twin {args.twin} on {torch.cuda.get_device_name(0)}")
print("## designs: B trajectories of K knots, resident inputs, median of alternating rounds")
for name in ("cstr_lqr", "oscillating_masses_lqr"):
    rate = name != "cstr_lqr"
    ex, plant, lqr = lc.example(name, hostemu=False, n_horizon=None, rate=rate)
    sim = lc.plant_on(ex.build_simulator(plant, setup=False), hostemu=False)
    nx, nu, n = plant.n_x, plant.n_u, lqr.n_design
    if name == "cstr_lqr":
        U = np.tile(ct.input_sequence(K)[:, None, :], (1, B, 1)) * (1.0 + 0.05 * rng.uniform(-1, 1, (K, B, nu)))
        X = sim.simulate_batch(ct.X0[None, :] + ct.START_SPREAD * rng.uniform(0, 1, (B, nx)), U)["x"][:K]
    else:
        U = rng.uniform(-1, 1, (K, B, nu))
        X = sim.simulate_batch(ex.X0[None, :] * (1.0 + 0.3 * rng.uniform(-1, 1, (B, nx))), U)["x"][:K]
    Q, R, dR = lc.example_weights(ex)
    Qd, Rd, Pd = tc.design_weights(np.asarray(Q, float), np.asarray(R, float), np.asarray(dR, float), rate)
    dX, dU, dQ, dR_ = t(X), t(U), t(Qd), t(Rd)
    Aj, Bj, M, Kt, P0 = e(K, B, nx, nx), e(K, B, nx, nu), e(K, nu, nx, B), e(K, B, nu, n), e(B, n, n)
    st, ps = e(B, dt=torch.int32), e(K, B, dt=torch.int32)
    Kf, Pf, stf = e(K * B, nu, n), e(K * B, n, n), e(K * B, dt=torch.int32)
    out = dict(K_traj=Kt.data_ptr()) if rate else dict(law_M=M.data_ptr(), ld=B)
    common = dict(pair_status=ps.data_ptr(), status=st.data_ptr(), shared_mask=7, stream=stream)
    along = lambda **kw: lqr.gains_along_device(plant, B, K, dX.data_ptr(), dU.data_ptr(), Aj.data_ptr(), Bj.data_ptr(), dQ.data_ptr(),      # noqa: E731
                                                dR_.data_ptr(), dQ.data_ptr(), P0.data_ptr(), **out, **common, **kw)
    variants = {
        "gains_along_device (pairs + recursion)": lambda: along(),
        "pairs launch alone": lambda: along(recursion=False),
        "recursion launch alone": lambda: lqr.gains_tv_batch_device(B, K, Aj.data_ptr(), Bj.data_ptr(), dQ.data_ptr(), dR_.data_ptr(), dQ.data_ptr(),
                                                                    P0.data_ptr(), **out, **common),
        "gains_at_device on the B K knots (frozen schedule, infinite horizon)":
            lambda: lqr.gains_at_device(plant, B * K, dX.data_ptr(), dU.data_ptr(), dQ.data_ptr(), dR_.data_ptr(), Kf.data_ptr(), Pf.data_ptr(),
                                        status=stf.data_ptr(), shared_mask=7, stream=stream),
    }
    sec = alternating(variants, args.rounds, 3)
    torch.cuda.synchronize()
    bad = int(np.count_nonzero(st.cpu().numpy())) + int(np.count_nonzero(ps.cpu().numpy() & 0xFF))
    t0 = time.perf_counter()
    for b in range(args.twin):
        pairs = [tc.twin_pair(plant, X[k, b], U[k, b], np.zeros(0), np.zeros(0), getattr(ex, "T_STEP", None)) for k in range(K)]
        tc.twin_tv(np.stack([q[0] for q in pairs]), np.stack([q[1] for q in pairs]), Qd, Rd, Pd, rate)
    twin = args.twin / (time.perf_counter() - t0)
    for label, s in sec.items():
        print(f"| {name} ({'rate' if rate else 'standard'} mode, N = {n}) | {label} | B = {B}, K = {K} | {s * 1e6:.1f} us per launch | "
              f"{B / s:.3e} trajectories/s | {B * K / s:.3e} knots/s |", flush=True)
    print(f"| {name} | numpy twin on one core (Jacobians, zero-order hold, recursion) | {args.twin} trajectories | {twin:.3e} trajectories/s | "
          f"gains_along_device x {B / sec['gains_along_device (pairs + recursion)'] / twin:.0f} | status words set: {bad} |", flush=True)

print("## the loop: examples/cstr_tracking.py, B perturbed starts, wall clock with the copies, median of alternating rounds")
with warnings.catch_warnings():
    warnings.simplefilter("ignore", UserWarning)
    lqr = ct.build_lqr()
model = ct.build_model()
sim = ct.build_simulator(model)
X_ref, U_ref = ct.record(sim, K)
X0 = ct.starts(B)
loop = BatchClosedLoopTVLQR(lqr, sim, X0, X_ref, U_ref)
Ktv = np.ascontiguousarray(loop.M.cpu().numpy().transpose(0, 3, 1, 2)[:, :1])      # (one reference: the gains are the same for every loop)
times = {"run(K, fused=True)": [], "K calls of step()": []}
for _ in range(args.rounds):
    for label in times:
        lp = BatchClosedLoopTVLQR(lqr, sim, X0, X_ref, U_ref, K_traj=Ktv)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lp.run(K, fused=label.startswith("run"))
        times[label].append(time.perf_counter() - t0)
for label, v in times.items():
    s = float(np.median(v))
    print(f"| BatchClosedLoopTVLQR.{label} | B = {B}, K = {K} | {s * 1e3:.2f} ms | {B * K / s:.3e} loop steps/s |", flush=True)
# tracking: the time-varying gains against the frozen schedule (gains_at at every knot, infinite horizon), same starts
g = lqr.gains_at(model, X_ref[:K, 0], U_ref[:, 0])
assert not g["status"].any()
Kfz = g["K"][:, None]
rec_tv = BatchClosedLoopTVLQR(lqr, sim, X0, X_ref, U_ref, K_traj=Ktv).run()
rec_fz = BatchClosedLoopTVLQR(lqr, sim, X0, X_ref, U_ref, K_traj=Kfz).run()
rec_ol = sim.simulate_batch(X0, U_ref[:, 0])
scale = np.array([1.0, 1.0, 100.0, 100.0])
for label, x in (("time-varying gains (gains_along)", rec_tv["x"]), ("frozen schedule (gains_at at every knot)", rec_fz["x"]),
                 ("U_ref replayed open loop", rec_ol["x"])):
    dv = np.linalg.norm((x - X_ref) / scale, axis=2)[:, 1:]                    # [K + 1][B - 1]: start 0 is the reference's own
    print(f"| tracking error, {label} | B = {B} starts | final: median {np.median(dv[-1]):.3e}, max {dv[-1].max():.3e} | "
          f"sum over the steps: median {np.median(dv.sum(axis=0)):.3e}, max {dv.sum(axis=0).max():.3e} |", flush=True)
