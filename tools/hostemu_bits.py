"""Bit-for-bit comparison of two source trees on the TEST-ONLY host emulation of the kernels (tests/hostemu.py).

    python tools/hostemu_bits.py record out.npz      in each of the two checkouts (e.g. two git worktrees), then
    python tools/hostemu_bits.py compare a.npz b.npz

`record` runs a fixed list of solves and stores x, g, lam_x, lam_g, f and every statistic of every solver call;
`compare` asks np.array_equal of every stored array and prints which paths of the line search the sample went
through (second-order corrections, rejected trial points, watchdogs, failed line searches).  A change of the
driver or of the vector passes that claims to keep every output bit is checked with this before a GPU is used.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LOG = []


def _install_recorder():
    """every result that leaves the solver object, in call order"""
    from do_mpc_amd.solver import HipIpmSolver
    call, batch = HipIpmSolver.__call__, HipIpmSolver.solve_batch

    def rec_call(self, *a, **kw):
        r = call(self, *a, **kw)
        st = self._stats
        LOG.append(dict(x=r["x"].copy(), g=r["g"].copy(), lam_x=r["lam_x"].copy(), lam_g=r["lam_g"].copy(), f=np.array([r["f"]]),
                        stats=np.array([[float(st[k]) for k in sorted(st) if isinstance(st[k], (bool, int, float, np.number)) and not k.startswith("t_")]]),
                        counts=np.array([[st["iter_count"], st["n_trials"], st["n_soc"], st["n_watchdog"], st["n_ls_fail"]]])))
        return r

    def rec_batch(self, *a, **kw):
        r = batch(self, *a, **kw)
        st = r["stats"]
        names = [n for n in st.dtype.names if not n.startswith("t_")]
        LOG.append(dict(x=r["x"].copy(), g=r["g"].copy(), lam_x=r["lam_x"].copy(), lam_g=r["lam_g"].copy(), f=r["f"].copy(),
                        stats=np.stack([st[n].astype(np.float64) for n in names], axis=1),
                        counts=np.stack([st[n] for n in ("iter_count", "n_trials", "n_soc", "n_watchdog", "n_ls_fail")], axis=1)))
        return r

    HipIpmSolver.__call__, HipIpmSolver.solve_batch = rec_call, rec_batch


def record(out):
    import hostemu
    import parity_common as pc
    import bench
    from do_mpc_amd.examples import CASES, rotating_masses
    _install_recorder()
    marks = []

    def make_mpc(name, **kw):
        with hostemu.patched():
            return CASES[name].build_mpc(CASES[name].build_model(), **kw)

    def cold(name, x0=None, **kw):
        mpc = make_mpc(name, **kw)
        x0 = CASES[name].X0 if x0 is None else x0
        mpc.x0 = x0
        mpc.set_initial_guess()
        mpc.make_step(x0)
        return mpc

    def replay(name, steps):
        g = pc.golden(name)
        mpc = make_mpc(name)
        mpc.x0 = CASES[name].X0
        mpc.set_initial_guess()
        for k in range(steps):
            mpc.make_step(g["mpc._x"][k])
            mpc.u0 = g["mpc._u"][k]

    def case(label, fn):
        n0 = len(LOG)
        fn()
        marks.extend([label] * (len(LOG) - n0))
        print(f"{label}: {len(LOG) - n0} solver calls", flush=True)

    case("bench batch, first 32 members", lambda: make_mpc("industrial_poly", max_batch=32).make_step_batch(bench.synthetic_x0_batch(16384)[:32]))
    case("industrial_poly watchdog trigger 1", lambda: cold("industrial_poly", pc.golden("industrial_poly")["mpc._x"][0],
                                                            nlpsol_opts={"ipopt.watchdog_shortened_iter_trigger": 1}))
    case("CSTR replay", lambda: replay("CSTR", 3))
    case("batch_reactor replay", lambda: replay("batch_reactor", 3))
    for label, over, x0 in pc.SINGLE_SLACK_CASES:
        case("single slack " + label, lambda: cold("CSTR", x0, nl_cons_single_slack=True, **over))
    for name, over, x0 in pc.NL_COLLOC_CASES:
        case("rows at collocation points " + name, lambda: cold(name, x0, **over))
    case("oscillating_masses_dae replay", lambda: replay("oscillating_masses_dae", 3))
    case("dip replay", lambda: replay("dip", 2))
    case("kinematic_bicycle", lambda: cold("kinematic_bicycle"))
    case("kite, full horizon", lambda: cold("kite", n_horizon=80))

    def mhe_run():
        with hostemu.patched():
            mhe = rotating_masses.build_mhe(rotating_masses.build_model())
        pc.check_mhe_golden_replay(lambda **kw: mhe, steps=5)
        mpc = mhe._mpc
        P, X0 = pc.mhe_straggler_problem(mhe)
        mhe.S.solve_batch(X0, mpc._lb_opt_x.master, mpc._ub_opt_x.master, mpc._nlp_cons_lb, mpc._nlp_cons_ub, P)
    case("estimator replay + straggler", mhe_run)

    flat = {}
    for i, e in enumerate(LOG):
        for k, v in e.items():
            flat[f"{i:03d}/{k}"] = np.asarray(v)
    flat["labels"] = np.array(marks)
    np.savez_compressed(out, **flat)
    print("stored", len(LOG), "solver calls in", out)


def compare(a, b):
    A, B = np.load(a), np.load(b)
    keys = sorted(k for k in A.files if k != "labels")
    assert keys == sorted(k for k in B.files if k != "labels"), "different lists of solver calls"
    bad = 0
    cnt = np.zeros(5, dtype=np.int64)
    paths = dict(solves=0, soc=0, rejected_trial=0, watchdog=0, ls_fail=0)
    for k in keys:
        same = A[k].shape == B[k].shape and np.array_equal(A[k], B[k], equal_nan=True)
        if not same:
            bad += 1
            print("DIFFERENT", k, A["labels"][int(k[:3])])
        if k.endswith("/counts"):
            c = A[k]
            cnt += c.sum(axis=0)
            paths["solves"] += c.shape[0]
            paths["soc"] += int((c[:, 2] > 0).sum())
            paths["rejected_trial"] += int((c[:, 1] > c[:, 0]).sum())
            paths["watchdog"] += int((c[:, 3] > 0).sum())
            paths["ls_fail"] += int((c[:, 4] > 0).sum())
    print(f"{len(keys)} arrays of {len(keys) // 7} solver calls compared, {bad} different")
    print("iterations %d, trial points %d, second-order corrections %d, watchdogs %d, failed line searches %d" % tuple(cnt))
    print("solves: %(solves)d; with a second-order correction %(soc)d, with a rejected trial point %(rejected_trial)d, "
          "with a watchdog %(watchdog)d, with a failed line search %(ls_fail)d" % paths)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "record":
        record(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
