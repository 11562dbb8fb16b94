"""Bit-for-bit comparison of two source trees on the TEST-ONLY host emulation of the plant integrator and of the extended Kalman
filter - the counterpart of tools/hostemu_bits.py (solver) for the other two runtimes.

    python tools/hostemu_plant_ekf_bits.py record out.npz      in each of the two checkouts, then
    python tools/hostemu_plant_ekf_bits.py compare a.npz b.npz

`record`: seeded batches through Simulator.make_step_batch (one ODE plant, one DAE plant; two consecutive calls with carry_z) and
EKF.step_batch (one discrete, one continuous model; shared and per-filter Q / R), each with B = 9 and with a batch that grows after a
smaller one (B = 3, 9, 3: the staging buffers are regrown and then reused); x, y / P, status and step counts of every call are stored.
`compare` asks np.array_equal of every stored array.
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
    np.savez_compressed(out, **flat)
    print("stored", len(flat), "arrays in", out)


def compare(a, b):
    A, B = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(B.files), "different lists of calls"
    bad = [k for k in sorted(A.files) if not (A[k].shape == B[k].shape and np.array_equal(A[k], B[k], equal_nan=True))]
    for k in bad:
        print("DIFFERENT", k)
    ok = sum(int((A[k] == 0).all()) for k in A.files if k.endswith("/status"))
    print(f"{len(A.files)} arrays of {len(A.files) // 4} calls compared, {len(bad)} different; calls with status 0 in every row: {ok}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "record":
        record(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
