"""Bit-for-bit comparison of two source trees on the TEST-ONLY host emulation of the plant integrator, of the extended Kalman
filter and of the LQR design - the counterpart of tools/hostemu_bits.py (solver) for the other three runtimes.

    python tools/hostemu_plant_ekf_bits.py record out.npz      in each of the two checkouts, then
    python tools/hostemu_plant_ekf_bits.py compare a.npz b.npz

`record`: seeded batches through Simulator.make_step_batch (one ODE plant, one DAE plant; two consecutive calls with carry_z) and
EKF.step_batch (one discrete, one continuous model; shared and per-filter Q / R), each with B = 9 and with a batch that grows after a
smaller one (B = 3, 9, 3: the staging buffers are regrown and then reused); x, y / P, status and step counts of every call are stored.
LQR: a standard design and a finite-horizon one (n_horizon passes) through gains_batch, a design in inputRatePenalization mode
through gains_at on the CSTR (Jacobians, zero-order hold), with the same batches; K, P, the discrete pair, status and step counts are
stored.  `compare` asks np.array_equal of every stored array.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def record(out):
    import ekf_common as ec
    import simulator_common as sc
    from do_mpc_amd.examples import CASES
    flat = {}

    def store(label, r, second):
        for k in ("x", second, "status", "n_steps"):
            flat[f"{label}/{k}"] = np.asarray(r[k]).copy()

    for name in ("CSTR", "dip"):                                # ODE plant, DAE plant
        m = CASES[name].build_model()
        rng = np.random.default_rng(5)
        X = CASES[name].X0[None, :] * (1.0 + 0.01 * rng.uniform(-1, 1, size=(9, m.n_x)))
        U = np.array(sc.U_TEST[name])[None, :] * (1.0 + 0.2 * rng.uniform(-1, 1, size=(9, m.n_u)))
        sim = sc.make_simulator(name, model=m)
        r = sim.make_step_batch(X, U)
        store(f"plant {name} B=9 call 1", r, "y")
        store(f"plant {name} B=9 call 2 (carry_z)", sim.make_step_batch(r["x"], U, carry_z=True), "y")
        sim = sc.make_simulator(name, model=m)                  # a fresh handle: B = 3, then 9, then 3
        for i, B in enumerate((3, 9, 3)):
            r = sim.make_step_batch(X[:B], U[:B], carry_z=i > 0)
            store(f"plant {name} growth call {i} B={B}", r, "y")
            X = np.concatenate([r["x"], X[B:]])
        print(f"plant {name}: recorded", flush=True)

    for name in ("oscillating_masses", "CSTR"):                 # discrete model, continuous model
        m = CASES[name].build_model(**ec.MODEL_KW.get(name, {}))
        X, Pc, Y, U, Q, R = ec.random_filters(m, 9, offset=CASES[name].X0 if name == "CSTR" else 0.0)
        for shared in (True, False):
            Qs, Rs = (Q[0], R[0]) if shared else (Q, R)
            tag = "shared Q/R" if shared else "per-filter Q/R"
            ekf = ec.make_ekf(name, hostemu=True, model=m)
            store(f"filter {name} {tag} B=9", ekf.step_batch(X, Pc, Y, U, Qs, Rs), "P")
            ekf = ec.make_ekf(name, hostemu=True, model=m)      # a fresh handle: B = 3, then 9, then 3
            for i, B in enumerate((3, 9, 3)):
                r = ekf.step_batch(X[:B], Pc[:B], Y[:B], U[:B], Qs if shared else Qs[:B], Rs if shared else Rs[:B])
                store(f"filter {name} {tag} growth call {i} B={B}", r, "P")
        print(f"filter {name}: recorded", flush=True)
    record_lqr(flat)
    np.savez_compressed(out, **flat)
    print("stored", len(flat), "arrays in", out)


def record_lqr(flat):
    import lqr_common as lc
    rng = np.random.default_rng(11)
    n, nu = 6, 2
    A = np.empty((9, n, n)); Bm = np.empty((9, n, nu))
    for b in range(9):
        A[b], Bm[b] = lc.twin_zoh(rng.standard_normal((n, n)) / np.sqrt(n), rng.standard_normal((n, nu)), float(rng.uniform(0.1, 0.5)))
    Q = np.diag(10.0 ** rng.uniform(-1, 1, n))
    R = np.diag(10.0 ** rng.uniform(-1, 1, nu))
    ex, plant, _ = lc.example("cstr_lqr", True, n_horizon=None)
    X, U = lc.family_b_points(ex, 9)
    designs = {                                                 # label -> (fresh controller, call on the first B members)
        "standard": (lambda: lc.model_free_lqr(n, nu, True), lambda q, B: q.gains_batch(A[:B], Bm[:B], Q, R)),
        "n_horizon=7": (lambda: lc.model_free_lqr(n, nu, True, n_horizon=7), lambda q, B: q.gains_batch(A[:B], Bm[:B], Q, R, P=Q)),
        "rate gains_at": (lambda: lc.example("cstr_lqr", True, n_horizon=None)[2], lambda q, B: q.gains_at(plant, X[:B], U[:B])),
    }
    for label, (fresh, call) in designs.items():
        def store(tag, r, B):
            for k, v in (("K", r["K"]), ("P", r["P"]), ("A", r.get("A", A[:B])), ("B", r.get("B", Bm[:B])), ("status", r["status"]), ("iters", r["iters"])):
                flat[f"design {label} {tag}/{k}"] = np.asarray(v).copy()
        store("B=9", call(fresh(), 9), 9)
        q = fresh()                                             # a fresh handle: B = 3, then 9, then 3
        for i, B in enumerate((3, 9, 3)):
            store(f"growth call {i} B={B}", call(q, B), B)
        print(f"design {label}: recorded", flush=True)


def compare(a, b):
    A, B = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(B.files), "different lists of calls"
    bad = [k for k in sorted(A.files) if not (A[k].shape == B[k].shape and np.array_equal(A[k], B[k], equal_nan=True))]
    for k in bad:
        print("DIFFERENT", k)
    ok = [sum(int((Z[k] == 0).all()) for k in Z.files if k.endswith("/status")) for Z in (A, B)]
    print(f"{len(A.files)} arrays of {sum(k.endswith('/status') for k in A.files)} calls compared, {len(bad)} different; "
          f"calls with status 0 in every row: {ok[0]} / {ok[1]}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "record":
        record(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
