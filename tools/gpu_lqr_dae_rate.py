"""Rate of the batched LQR design for models with algebraic states (LQR.gains_at on a DAE model: Newton on g = 0, the index-1
reduction, zero-order hold and design in ONE launch of csrc/dompc_lqr.hip) on resident inputs: designs per second at B = 16 384 for the
batch-reactor DAE model (n_x = 3, n_u = 1, n_z = 1) and for the n_z = 16 case of the tests (n_x = 2, n_u = 1), and - the yardstick of
the same run - for gains_at on the ODE model of the CSTR example (tools/gpu_lqr_rate.py's last line).  Device events around at least
`--seconds` of launches after a warm-up.
usage: python tools/gpu_lqr_dae_rate.py [--batch 16384] [--seconds 1.0] > profiles/lqr_dae_rate.txt"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import lqr_common as lc
import lqr_dae_common as dc

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--seconds", type=float, default=1.0)
args = ap.parse_args()
dev = torch.device("cuda", 0)
t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), device=dev)      # noqa: E731
B = args.batch


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


def report(label, sec, n, st):
    it, newton = (st >> 8) & 0xFFFF, st >> 24
    print(f"| {label} | B = {B} | {sec * 1e6:.1f} us per launch over {n} launches | {B / sec:.3e} designs/s | steps per design: mean "
          f"{it.mean():.1f}, max {it.max()} | Newton updates: mean {newton.mean():.1f}, max {newton.max()} | status bits set: "
          f"{int(np.count_nonzero(st & 0xFF))} of {B} |", flush=True)


print(f"# tools/gpu_lqr_dae_rate.py --batch {B} --seconds {args.seconds} on {torch.cuda.get_device_name(0)}")
st = torch.zeros(B, dtype=torch.int32, device=dev)
stream = torch.cuda.current_stream().cuda_stream
for name, label in (("batch_reactor", "gains_at on the batch-reactor DAE model (n_x = 3, n_u = 1, n_z = 1; Newton + reduction + zero-order hold + design, infinite horizon)"),
                    ("nz16", "gains_at on the n_z = 16 model of the tests (n_x = 2, n_u = 1; Newton + reduction + zero-order hold + design, infinite horizon)")):
    model, lqr = dc.design(name, hostemu=False)
    X, U = dc.points(model, B, scale=2.0 if name == "batch_reactor" else 1.0)
    nx, nu, nz = model.n_x, model.n_u, model.n_z
    dX, dU, dZ, dQ, dR = t(X), t(U), t(np.zeros((B, nz))), t(np.eye(nx)), t(np.eye(nu))
    K, P = torch.empty((B, nu, nx), dtype=torch.float64, device=dev), torch.empty((B, nx, nx), dtype=torch.float64, device=dev)
    Zo = torch.empty((B, nz), dtype=torch.float64, device=dev)
    launch = lambda: lqr.gains_at_device(model, B, dX.data_ptr(), dU.data_ptr(), dQ.data_ptr(), dR.data_ptr(), K.data_ptr(), P.data_ptr(),      # noqa: E731
                                         status=st.data_ptr(), shared_mask=1 | 2, stream=stream, z=dZ.data_ptr(), z_out=Zo.data_ptr())
    sec, cnt = timed(launch, args.seconds)
    report(label, sec, cnt, st.cpu().numpy())
ex, plant, lqr = lc.example("cstr_lqr", hostemu=False)
X, U = lc.family_b_points(ex, B)
Q, R, dR = lc.example_weights(ex)
Qd = np.block([[Q, np.zeros((4, 2))], [np.zeros((2, 4)), R]])
dX, dU, dQ, dR_ = t(X), t(U), t(Qd), t(dR)
K, P = torch.empty((B, 2, 6), dtype=torch.float64, device=dev), torch.empty((B, 6, 6), dtype=torch.float64, device=dev)
launch = lambda: lqr.gains_at_device(plant, B, dX.data_ptr(), dU.data_ptr(), dQ.data_ptr(), dR_.data_ptr(), K.data_ptr(), P.data_ptr(),      # noqa: E731
                                     P_term=dQ.data_ptr(), status=st.data_ptr(), shared_mask=1 | 2 | 4, stream=stream)
sec, cnt = timed(launch, args.seconds)
report("yardstick: gains_at on the ODE model of the CSTR (Jacobians + zero-order hold + design, N = 6, n_horizon = 10)", sec, cnt, st.cpu().numpy())
