"""Rate of the batched extended Kalman filter (do_mpc_amd/ekf.py, csrc/dompc_ekf.hip) on resident inputs: filter steps per second at
B = 16 384 for triple_tank, oscillating_masses (estimation=True) and rotating_masses, the bytes a step has to move over the kernel time
as a share of the HBM peak (a WHOLE-KERNEL figure: it says how far the kernel is from the memory roof, not where its time goes), and -
alternating with the rotating-masses filter in the same process - the batched moving horizon estimator on the same model
(BatchClosedLoopMHE's estimator launch, mhe.S.solve_batch_device), the estimator a user had before.
Device events around at least `--seconds` of launches after a warm-up; x and P are updated in place, so the filters run on with the
same measurement and settle - the status words at the end say whether every filter was still updating.
usage: python tools/gpu_ekf_rate.py [--batch 16384] [--mhe-batch 4096] [--seconds 1.0] > profiles/ekf_rate.txt"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from do_mpc_amd.ekf import EKF
from do_mpc_amd.examples import CASES

HBM_PEAK = 8.0e12          # bytes/s
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--mhe-batch", type=int, default=4096)
ap.add_argument("--seconds", type=float, default=1.0)
args = ap.parse_args()
dev = torch.device("cuda", 0)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)      # noqa: E731
SETTINGS = {"triple_tank": ({}, 1.0, {"p1": 2.0}, {"tvp1": 0.5}, 2.0, 1e-4), "oscillating_masses": ({"estimation": True}, 0.5, {}, {}, 0.0, 0.3),
            "rotating_masses": ({}, 0.1, {"Theta_1": 2.25e-4, "Theta_2": 2.25e-4, "Theta_3": 2.25e-4, "P_p": 1.0}, {}, 0.0, 0.3)}


class FilterRun:
    def __init__(self, name, B):
        kw, t_step, pv, tv, x_off, u_scale = SETTINGS[name]
        m = self.m = CASES[name].build_model(**kw)
        ekf = self.ekf = EKF(m)
        ekf.settings.t_step = t_step
        if m.n_p:
            pt = ekf.get_p_template()
            for k, v in pv.items():
                pt[k] = v
            ekf.set_p_fun(lambda _t: pt)
        if m.n_tvp:
            tt = ekf.get_tvp_template()
            for k, v in tv.items():
                tt[k] = v
            ekf.set_tvp_fun(lambda _t: tt)
        ekf.setup()
        rng = np.random.default_rng(1)
        nx, ny, nu = m.n_x, m.n_y, m.n_u
        X = x_off + 0.3 * rng.uniform(-1, 1, (B, nx))
        G = rng.uniform(-1, 1, (B, nx, nx))
        self.B = B
        self.x, self.P = t(X), t(0.1 * np.eye(nx)[None] + 0.02 * G @ G.transpose(0, 2, 1))
        yv = np.asarray(m._meas_fun.eval(X.T, np.zeros((nu, B)), np.zeros((0, B)), np.tile(ekf.tvp_fun(0).master[:, None], (1, B)),
                                         np.tile(ekf.p_fun(0).master[:, None], (1, B)), np.zeros((m.n_v, B)))[0], float).T
        self.y, self.u = t(yv + 0.01 * rng.standard_normal((B, ny))), t(u_scale * rng.uniform(0, 1, (B, nu)))
        self.Q, self.R = t(1e-3 * np.eye(nx)), t(1e-2 * np.eye(ny))
        self.p, self.tvp = t(ekf.p_fun(0).master if m.n_p else np.zeros(1)), t(ekf.tvp_fun(0).master if m.n_tvp else np.zeros(1))
        self.st = torch.zeros(B, dtype=torch.int32, device=dev)
        # what one step has to move: x and P in and out, y and u in, the status word out; tvp, p, Q and R are shared by the batch
        self.bytes = (2 * nx * nx + 2 * nx + ny + nu) * 8 + 4

    def launch(self):
        self.ekf.step_batch_device(self.B, self.x.data_ptr(), self.P.data_ptr(), self.y.data_ptr(), self.u.data_ptr(), self.tvp.data_ptr(),
                                   self.p.data_ptr(), self.Q.data_ptr(), self.R.data_ptr(), status=self.st.data_ptr(), shared_mask=2 | 4 | 8 | 16,
                                   stream=torch.cuda.current_stream().cuda_stream)


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
    print(f"| {name} (nx {run.m.n_x}, ny {run.m.n_y}, {run.m.model_type}) | B = {run.B} | {sec * 1e6:.1f} us per launch over {n} launches | "
          f"{run.B / sec:.3e} filter steps/s | {run.bytes} B per step -> {run.B * run.bytes / sec / 1e9:.1f} GB/s = "
          f"{100.0 * run.B * run.bytes / sec / HBM_PEAK:.2f} % of 8 TB/s (whole kernel) | integration steps per filter in the last launch: "
          f"mean {np.mean(st >> 8):.1f}, max {np.max(st >> 8)} | status bits set: {int(np.count_nonzero(st & 0xFF))} of {run.B} |", flush=True)


def mhe_run(B):
    """the estimator launch of BatchClosedLoopMHE on rotating_masses: B cold estimation problems (horizon 10, one estimated parameter) from
    random previous estimates and measurement windows"""
    ex = CASES["rotating_masses"]
    mhe = ex.build_mhe(ex.build_model(), max_batch=B, nlpsol_opts={"ipopt.max_iter": 200})
    from do_mpc_amd.solver import STATS_DTYPE
    rng = np.random.default_rng(2)
    nx, npe = mhe.model.n_x, mhe.n_p_est
    op = np.zeros((B, mhe.n_opt_p))
    x_est = 0.1 * rng.uniform(-1, 1, (B, nx))
    op[:, :nx] = x_est
    op[:, nx:nx + npe] = 1e-4
    op[:, mhe._po_pset:mhe._po_tvp] = mhe.p_fun(0.0).master
    op[:, mhe._po_tvp:mhe._po_y] = mhe.tvp_fun(0.0).master
    op[:, mhe._po_y:] = 0.1 * rng.uniform(-1, 1, op[:, mhe._po_y:].shape)
    ge = np.zeros((B, mhe.n_opt_x))
    ge[:, :mhe._o_z].reshape(B, -1, nx)[:] = (x_est / mhe._x_scaling.master)[:, None, :]
    ge[:, mhe._o_p:] = 1e-4 / mhe._p_est_scaling.master
    em, es = mhe._mpc, mhe._ps
    Pe, Ge = t(mhe._p_to_chain(op)), t(mhe._to_chain(ge))
    lbx, ubx, lbg, ubg = t(em._lb_opt_x.master), t(em._ub_opt_x.master), t(em._nlp_cons_lb), t(em._nlp_cons_ub)
    sol = torch.empty((B, es.n_opt_x), dtype=torch.float64, device=dev)
    f = torch.empty(B, dtype=torch.float64, device=dev)
    stats = torch.zeros(B * STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)

    def launch():
        mhe.S.solve_batch_device(B, Ge.data_ptr(), lbx.data_ptr(), ubx.data_ptr(), lbg.data_ptr(), ubg.data_ptr(), Pe.data_ptr(), sol.data_ptr(),
                                 0, 0, 0, f.data_ptr(), stats.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    return launch, lambda: np.frombuffer(stats.cpu().numpy().tobytes(), dtype=STATS_DTYPE).copy()


print(f"# tools/gpu_ekf_rate.py --batch {args.batch} --mhe-batch {args.mhe_batch} --seconds {args.seconds} on {torch.cuda.get_device_name(0)}")
for name in ("triple_tank", "oscillating_masses"):
    run = FilterRun(name, args.batch)
    sec, n = timed(run.launch, args.seconds)
    report(name, run, sec, n)
run = FilterRun("rotating_masses", args.batch)
try:
    mhe_launch, mhe_stats = mhe_run(args.mhe_batch)
except Exception as e:                      # noqa: BLE001
    mhe_launch = None
    print(f"| rotating_masses MHE | not measured ({type(e).__name__}: {e}) |")
for rnd in range(2):                        # alternating: filter, estimator, filter, estimator
    sec, n = timed(run.launch, args.seconds)
    report(f"rotating_masses, round {rnd + 1}", run, sec, n)
    if mhe_launch is not None:
        msec, mn = timed(mhe_launch, args.seconds, warm=1)
        s = mhe_stats()
        print(f"| rotating_masses MHE (horizon 10, 1 estimated parameter, cold solves), round {rnd + 1} | B = {args.mhe_batch} | "
              f"{msec * 1e3:.2f} ms per launch over {mn} launches | {args.mhe_batch / msec:.3e} estimator steps/s | "
              f"{int(s['success'].sum())} of {args.mhe_batch} converged, {s['iter_count'].mean():.1f} iterations on average | "
              f"filter steps per estimator step at equal time: {(run.B / sec) / (args.mhe_batch / msec):.0f} |", flush=True)
