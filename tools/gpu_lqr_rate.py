"""Rate of the batched LQR design (do_mpc_amd/lqr.py, csrc/dompc_lqr.hip) on resident inputs: designs per second at B = 16 384 for the
two shipped examples (their own mode and horizon, the pair perturbed per member), for N = 16 (n_x = 16, n_u = 4, random systems of
family (a) of the tests, infinite horizon) and for gains_at on the CSTR model (Jacobians, zero-order hold and design in one launch),
with the doubling steps the launch took.  Beside each figure: the twin's rate (scipy.linalg.solve_discrete_are or the reference's
recursion, plus scipy.signal.cont2discrete and the Jacobians for gains_at) on ONE core of the same box, over `--twin` members.
Device events around at least `--seconds` of launches after a warm-up.
usage: python tools/gpu_lqr_rate.py [--batch 16384] [--seconds 1.0] [--twin 64] > profiles/lqr_rate.txt"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import lqr_common as lc

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--seconds", type=float, default=1.0)
ap.add_argument("--twin", type=int, default=64)
args = ap.parse_args()
dev = torch.device("cuda", 0)
t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), device=dev)      # noqa: E731
B = args.batch
rng = np.random.default_rng(1)


def timed(launch, seconds, warm=3):
    """-> (seconds per launch, launches): device events around rounds of launches until `seconds` of them have been measured"""
    for _ in range(warm):
        launch()
    torch.cuda.synchronize()
    total, n, per_round = 0.0, 0, 1
    while total < seconds:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per_round):
            launch()
        e1.record()
        torch.cuda.synchronize()
        dt = e0.elapsed_time(e1) * 1e-3
        total += dt
        n += per_round
        per_round = max(1, min(1000, int(0.25 * seconds / max(dt / per_round, 1e-7))))
    return total / n, n


def report(label, sec, n, st, twin_rate):
    it = st >> 8
    print(f"| {label} | B = {B} | {sec * 1e6:.1f} us per launch over {n} launches | {B / sec:.3e} designs/s | steps per design: mean "
          f"{it.mean():.1f}, max {it.max()} | status bits set: {int(np.count_nonzero(st & 0xFF))} of {B} | twin on one core: {twin_rate:.3e} designs/s "
          f"-> x {B / sec / twin_rate:.0f} |", flush=True)


def twin_rate(fn, n):
    t0 = time.perf_counter()
    for b in range(n):
        fn(b)
    return n / (time.perf_counter() - t0)


print(f"# tools/gpu_lqr_rate.py --batch {B} --seconds {args.seconds} --twin {args.twin} on {torch.cuda.get_device_name(0)}")
st = torch.zeros(B, dtype=torch.int32, device=dev)
stream = torch.cuda.current_stream().cuda_stream
for name in ("oscillating_masses_lqr", "cstr_lqr"):
    ex, plant, lqr = lc.example(name, hostemu=False)
    Q, R, dR = lc.example_weights(ex)
    A0, B0 = lqr.model.sys_A, lqr.model.sys_B
    A = A0[None] * (1.0 + 0.01 * rng.uniform(-1, 1, (B,) + A0.shape))
    Bm = B0[None] * (1.0 + 0.01 * rng.uniform(-1, 1, (B,) + B0.shape))
    nx, nu, n = lqr.model.n_x, lqr.model.n_u, lqr.n_design
    Qd = np.block([[Q, np.zeros((nx, nu))], [np.zeros((nu, nx)), R]])
    dA, dB, dQ, dR_ = t(A), t(Bm), t(Qd), t(dR)
    K, P = torch.empty((B, nu, n), dtype=torch.float64, device=dev), torch.empty((B, n, n), dtype=torch.float64, device=dev)
    launch = lambda: lqr.gains_batch_device(B, dA.data_ptr(), dB.data_ptr(), dQ.data_ptr(), dR_.data_ptr(), K.data_ptr(), P.data_ptr(),      # noqa: E731
                                            P_term=dQ.data_ptr(), status=st.data_ptr(), shared_mask=1 | 2 | 4, stream=stream)
    sec, cnt = timed(launch, args.seconds)
    nh = lqr.settings.n_horizon
    tr = twin_rate(lambda b: lc.twin_design(A[b], Bm[b], Q, R, n_horizon=nh, rate=True, delR=dR), args.twin)
    report(f"{name} (N = {n}, rate mode, {'infinite horizon' if nh is None else f'n_horizon = {nh}'})", sec, cnt, st.cpu().numpy(), tr)
mem = []
while len(mem) < B:
    Ac, Bc, dt = rng.standard_normal((16, 16)) / 4.0, rng.standard_normal((16, 4)), float(rng.uniform(0.1, 0.5))
    Ad, Bd = lc.twin_zoh(Ac, Bc, dt) if len(mem) < 256 else mem[len(mem) % 256][:2]      # (256 distinct systems, repeated)
    mem.append((Ad, Bd, np.diag(10.0 ** rng.uniform(-1, 1, 16)), np.diag(10.0 ** rng.uniform(-1, 1, 4))))
A, Bm, Q, R = (np.stack([m[i] for m in mem]) for i in range(4))
lqr = lc.model_free_lqr(16, 4, hostemu=False)
dA, dB, dQ, dR_ = t(A), t(Bm), t(Q), t(R)
K, P = torch.empty((B, 4, 16), dtype=torch.float64, device=dev), torch.empty((B, 16, 16), dtype=torch.float64, device=dev)
launch = lambda: lqr.gains_batch_device(B, dA.data_ptr(), dB.data_ptr(), dQ.data_ptr(), dR_.data_ptr(), K.data_ptr(), P.data_ptr(),      # noqa: E731
                                        status=st.data_ptr(), stream=stream)
sec, cnt = timed(launch, args.seconds)
report("random systems (N = 16, n_u = 4, standard mode, infinite horizon)", sec, cnt, st.cpu().numpy(),
       twin_rate(lambda b: lc.twin_design(A[b], Bm[b], Q[b], R[b]), args.twin))
ex, plant, lqr = lc.example("cstr_lqr", hostemu=False)
X, U = lc.family_b_points(ex, B)
Q, R, dR = lc.example_weights(ex)
Qd = np.block([[Q, np.zeros((4, 2))], [np.zeros((2, 4)), R]])
dX, dU, dQ, dR_ = t(X), t(U), t(Qd), t(dR)
K, P = torch.empty((B, 2, 6), dtype=torch.float64, device=dev), torch.empty((B, 6, 6), dtype=torch.float64, device=dev)
launch = lambda: lqr.gains_at_device(plant, B, dX.data_ptr(), dU.data_ptr(), dQ.data_ptr(), dR_.data_ptr(), K.data_ptr(), P.data_ptr(),      # noqa: E731
                                     P_term=dQ.data_ptr(), status=st.data_ptr(), shared_mask=1 | 2 | 4, stream=stream)
sec, cnt = timed(launch, args.seconds)


def twin_at(b):
    Ac, Bc = lc.twin_jacobians(plant, X[b], U[b])
    Ad, Bd = lc.twin_zoh(Ac, Bc, ex.T_STEP)
    return lc.twin_design(Ad, Bd, Q, R, n_horizon=lqr.settings.n_horizon, rate=True, delR=dR)


report("gains_at on the CSTR model (Jacobians + zero-order hold + design, N = 6, n_horizon = 10)", sec, cnt, st.cpu().numpy(), twin_rate(twin_at, args.twin))
