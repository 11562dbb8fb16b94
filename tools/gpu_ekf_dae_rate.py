"""Rate of the batched extended Kalman filter for models with algebraic states (do_mpc_amd/ekf.py with settings.dae_reduction: Newton
on g = 0 and the reduction A = f_x - f_z g_z^-1 g_x inside the launch of csrc/dompc_ekf.hip) on resident inputs: filter steps per second
at B = 16 384 for models 1, 4 and 5 of tests/ekf_dae_common.py (the oscillating masses with their successor state as algebraic state,
the double inverted pendulum, the batch reactor) and - in the same process, alternating with them - for the ODE filters of models 1
and 5 with z eliminated by hand, which is what the reduction costs.  Device events around at least `--seconds` of launches after a
warm-up; x, P and z are updated in place, so the filters run on with the same measurement and settle - the status words at the end
say whether every filter was still updating.  No bar was fixed in advance.
usage: python tools/gpu_ekf_dae_rate.py [--batch 16384] [--seconds 1.0] > profiles/ekf_dae_rate.txt"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import ekf_common as ec
import ekf_dae_common as dc

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--seconds", type=float, default=1.0)
args = ap.parse_args()
dev = torch.device("cuda", 0)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)      # noqa: E731
# name -> (centre of the states, spread, inputs)
START = {"masses": (np.zeros(4), 0.3, [0.1]), "masses_eliminated": (np.zeros(4), 0.3, [0.1]),
         "dip": (np.array([0.1, 0.3, -0.2, 0.05, -0.1, 0.1]), 0.02, [0.5]),
         "batch_reactor": (np.array([1.0, 0.5, 0.2]), 0.1, [0.3]), "batch_reactor_eliminated": (np.array([1.0, 0.5, 0.2]), 0.1, [0.3])}


class FilterRun:
    def __init__(self, name, B):
        ekf = self.ekf = dc.make_filter(name, hostemu=False)
        m = self.m = ekf.model
        centre, spread, u = START[name]
        rng = np.random.default_rng(1)
        nx, ny, nz = m.n_x, m.n_y, m.n_z
        X = centre + spread * rng.uniform(-1, 1, (B, nx))
        G = rng.uniform(-1, 1, (B, nx, nx))
        self.B = B
        self.x, self.P = t(X), t(0.1 * np.eye(nx)[None] + 0.02 * G @ G.transpose(0, 2, 1))
        p, tvp = ec.p_tvp(ekf)
        self.u = t(np.tile(u, (B, 1)))
        self.Q, self.R = t(1e-3 * np.eye(nx)), t(1e-2 * np.eye(ny))
        self.p, self.tvp = t(p if m.n_p else np.zeros(1)), t(tvp if m.n_tvp else np.zeros(1))
        self.st = torch.zeros(B, dtype=torch.int32, device=dev)
        self.z = t(np.zeros((B, max(nz, 1))))
        self.nw = torch.zeros(B, dtype=torch.int32, device=dev)
        # measurements near the start: the states themselves (model 1: x_0, x_2 and, for the successor of x_1, x_1), with noise
        yv = X[:, [0, 2, 1]] if name.startswith("masses") else X
        self.y = t(yv + 0.01 * rng.standard_normal((B, ny)))

    def launch(self):
        kw = {"z": self.z.data_ptr(), "newton": self.nw.data_ptr()} if self.m.n_z else {}
        self.ekf.step_batch_device(self.B, self.x.data_ptr(), self.P.data_ptr(), self.y.data_ptr(), self.u.data_ptr(), self.tvp.data_ptr(),
                                   self.p.data_ptr(), self.Q.data_ptr(), self.R.data_ptr(), status=self.st.data_ptr(), shared_mask=2 | 4 | 8 | 16,
                                   stream=torch.cuda.current_stream().cuda_stream, **kw)


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


def report(name, run, sec, n):
    st = run.st.cpu().numpy()
    nw = run.nw.cpu().numpy()
    print(f"| {name} (nx {run.m.n_x}, nz {run.m.n_z}, ny {run.m.n_y}, {run.m.model_type}) | B = {run.B} | {sec * 1e6:.1f} us per launch over {n} launches | "
          f"{run.B / sec:.3e} filter steps/s | integration steps per filter in the last launch: mean {np.mean(st >> 8):.1f}, max {np.max(st >> 8)} | "
          f"Newton updates per filter in the last launch: mean {np.mean(nw):.1f}, max {np.max(nw)} | status bits set: "
          f"{int(np.count_nonzero(st & 0xFF))} of {run.B} |", flush=True)
    return run.B / sec


print(f"# tools/gpu_ekf_dae_rate.py --batch {args.batch} --seconds {args.seconds} on {torch.cuda.get_device_name(0)}")
for dae, ode in (("masses", "masses_eliminated"), ("batch_reactor", "batch_reactor_eliminated"), ("dip", None)):
    runs = {k: FilterRun(k, args.batch) for k in (dae, ode) if k}
    rates = {k: [] for k in runs}
    for rnd in range(2):                        # alternating: with z, eliminated, with z, eliminated
        for k, run in runs.items():
            sec, n = timed(run.launch, args.seconds)
            rates[k].append(report(f"{k}, round {rnd + 1}", run, sec, n))
    if ode:
        ratio = [a / b for a, b in zip(rates[dae], rates[ode])]
        print(f"| {dae} / {ode}: filter steps/s with the algebraic states over filter steps/s of the eliminated ODE model | round 1: {ratio[0]:.3f} | "
              f"round 2: {ratio[1]:.3f} |", flush=True)
