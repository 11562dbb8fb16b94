"""Time of the batched sensitivities (DoMPCDifferentiator.differentiate_batch_device: du0/dx0 and du0/du_prev for every member of a
batch) next to the cold solve of the same batch and to the route that existed before, a loop of differentiate() over single members.

    python tools/gpu_sens_rate.py [--batch 16384] [--members 32] [--out profiles/sens_rate.txt]

batch_reactor and industrial_poly, inputs resident on the device, one process.  Per case: the cold solve (one warm-up launch, then the
mean of `--reps` launches between device synchronisations), the sensitivity call (same), and differentiate() for `--members` members
copied one by one into the controller's attributes (wall time per member, scaled to the batch)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from do_mpc_amd.differentiator import DoMPCDifferentiator  # noqa: E402
from do_mpc_amd.examples import CASES  # noqa: E402
from do_mpc_amd.solver import STATS_DTYPE  # noqa: E402


def x0_batch(name, B):
    if name == "industrial_poly":
        import bench
        return bench.synthetic_x0_batch(B)
    x0 = np.asarray(CASES[name].X0, float)
    return x0 * (1.0 + 0.02 * np.random.default_rng(99).uniform(-1, 1, size=(B, x0.size)))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def run(name, B, members, reps):
    ex = CASES[name]
    mpc = ex.build_mpc(ex.build_model(), max_batch=B)
    ps = mpc.structure
    dev = torch.device("cuda", 0)
    X0 = x0_batch(name, B)
    P = np.tile(mpc.opt_p_num.master, (B, 1))
    P[:, :ps.nx] = X0
    P[:, ps.p_off_tvp:ps.p_off_p] = mpc.tvp_fun(0.0).master
    P[:, ps.p_off_p:ps.p_off_uprev] = mpc.p_fun(0.0).master
    P[:, ps.p_off_uprev:] = 0.0
    Xi = np.zeros((B, ps.n_opt_x))
    Xi[:, :ps.off_z].reshape(B, -1, ps.nx)[:] = (X0 / mpc._x_scaling.master)[:, None, :]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)      # noqa: E731
    t = {"Xi": up(Xi), "P": up(P), "lbx": up(mpc._lb_opt_x.master), "ubx": up(mpc._ub_opt_x.master), "lbg": up(mpc._nlp_cons_lb),
         "ubg": up(mpc._nlp_cons_ub)}
    for k, n in (("X", ps.n_opt_x), ("G", ps.n_g), ("LX", ps.n_opt_x), ("LG", ps.n_g)):
        t[k] = torch.empty((B, n), dtype=torch.float64, device=dev)
    t["F"] = torch.empty(B, dtype=torch.float64, device=dev)
    t["Stats"] = torch.zeros(B * STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def solve():
        mpc.S.solve_batch_device(B, t["Xi"].data_ptr(), t["lbx"].data_ptr(), t["ubx"].data_ptr(), t["lbg"].data_ptr(), t["ubg"].data_ptr(),
                                 t["P"].data_ptr(), t["X"].data_ptr(), t["G"].data_ptr(), t["LX"].data_ptr(), t["LG"].data_ptr(),
                                 t["F"].data_ptr(), t["Stats"].data_ptr(), stream=stream)

    t_solve = timed(solve, reps)
    nd = DoMPCDifferentiator(mpc, check_SC=False)
    out = {}

    def sens():
        out.update(nd.differentiate_batch_device(t["X"], t["LG"], t["Stats"], t["P"], out=out or None))

    t_sens = timed(sens, reps)
    ok = out["ok"].cpu().numpy()
    stats = np.frombuffer(t["Stats"].cpu().numpy().tobytes(), dtype=STATS_DTYPE)
    # the route that existed before: one member at a time through the controller's attributes
    r = {k: t[v][:members].cpu().numpy() for k, v in (("x", "X"), ("g", "G"), ("lam_x", "LX"), ("lam_g", "LG"), ("p", "P"))}
    S_batch = out["dxdp"][:members].cpu().numpy()
    sel = mpc._opt_x_layout.resolve(("_u", 0, 0)).ravel()
    lay = mpc._opt_p_layout
    col = np.concatenate([lay.resolve(("_x0",)).ravel(), lay.resolve(("_u_prev",)).ravel()])
    dt, n, dev_max = 0.0, 0, 0.0
    for q in range(members):
        if not (stats["success"][q] and ok[q]):
            continue
        t0 = time.perf_counter()
        mpc.opt_x_num.master[:] = r["x"][q]
        mpc.opt_p_num.master[:] = r["p"][q]
        mpc.lam_g_num, mpc.lam_x_num, mpc.opt_g_num = r["lam_g"][q], r["lam_x"][q], r["g"][q]
        mpc.solver_stats = mpc.S._stats_dict(stats[q])
        dxdp, _ = nd.differentiate()
        if n or q:                          # (the first call allocates staging buffers: not counted when there is another one)
            dt += time.perf_counter() - t0
            n += 1
        ref = np.asarray(dxdp)[np.ix_(sel, col)]
        dev_max = max(dev_max, float(np.max(np.abs(ref - S_batch[q])) / max(1.0, np.max(np.abs(ref)))))
    t_loop = dt / max(n, 1) * B
    R = 1 + col.size
    lines = [f"{name}: B = {B}, n_opt_x = {ps.n_opt_x}, n_g = {ps.n_g}, n_opt_p = {ps.n_opt_p}, directions per point = {R} "
             f"(1 + n_x + n_u), solves succeeded {int(stats['success'].sum())} / {B}, sensitivities ok {int(ok.sum())} / {B}, "
             f"mean IPM iterations {float(np.mean(stats['iter_count'])):.1f}",
             f"  cold solve of the batch                      {t_solve * 1e3:10.1f} ms",
             f"  differentiate_batch_device                   {t_sens * 1e3:10.1f} ms   ({t_sens / B / R * 1e6:.2f} us per direction, "
             f"{t_solve / B / max(float(np.mean(stats['iter_count'])), 1.0) * 1e6:.2f} us per IPM iteration of the solve)",
             f"  loop of differentiate() ({n} members timed)   {t_loop * 1e3:10.1f} ms   scaled to the batch ({dt / max(n, 1) * 1e3:.2f} ms per member)",
             f"  sensitivities / cold solve                   {t_sens / t_solve:10.3f}",
             f"  loop of differentiate() / sensitivities      {t_loop / t_sens:10.1f}",
             f"  max |batch - differentiate()| / max(1, |ref|) over the timed members: {dev_max:.1e}"]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--members", type=int, default=32)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"tools/gpu_sens_rate.py --batch {a.batch} --members {a.members} --reps {a.reps} on {torch.cuda.get_device_name(0)}", ""]
    for name in ("batch_reactor", "industrial_poly"):
        lines += run(name, a.batch, a.members, a.reps) + [""]
        print("\n".join(lines[-9:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines))


if __name__ == "__main__":
    main()
