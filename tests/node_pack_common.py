"""The packed per-node index records (KArgs::node_pack, csrc/dompc_kargs.h) against the table look-ups they replace - cases and the
comparison shared by the host-emulation (CPU CI) and the HIP (-m gpu) test modules.

The build with -DDOMPC_NODE_PACK=0 keeps the look-ups in node_x_off, node_u_off, node_in_edge, node_parent, node_child_start, ... compiled
in; the default build reads one record per node.  Both form the same integers, so every output of a solve has the same bits."""
import numpy as np

import quad_common  # noqa: F401  (the five-edge CSTR is the case of tests/quad_common.py)
import riccati_shape_common as rs
from do_mpc_amd.examples import CASES
from do_mpc_amd.solver import HipIpmSolver

COMPARISON_DEFS = "DOMPC_NODE_PACK=0"

# (id, example, build_mpc keywords)
CASES_CPU = [(mid, rs.name_of(mid), {}) for mid in rs.IDS] + [
    ("CSTR_five_edges", "CSTR", dict(n_horizon=5, n_robust=0)),
    # branches at the root only: the chain levels start at stage 1, nodes that are not the first child of their parent
    ("industrial_poly_N3_robust1", "industrial_poly", dict(n_horizon=3, n_robust=1)),
    # two branching levels: the level-by-level node updates below the root read the records too
    ("industrial_poly_N3_robust2", "industrial_poly", dict(n_horizon=3, n_robust=2)),
]
IDS_CPU = [c[0] for c in CASES_CPU]
OUTPUTS = ("x", "g", "lam_g", "lam_x", "f")


def statistics(st):
    """every numeric statistic of a solve except the timers, by name"""
    return {k: float(st[k]) for k in sorted(st) if isinstance(st[k], (bool, int, float, np.number)) and not k.startswith("t_")}


def cold_solve(make_mpc, name, kw, monkeypatch, defs):
    """outputs and statistics of one cold make_step of `name` from the example's X0 with the kernels built with the switches `defs`"""
    got = {}
    call = HipIpmSolver.__call__

    def rec(self, *a, **k):
        r = call(self, *a, **k)
        got.update({key: np.array(r[key], dtype=np.float64, copy=True) for key in OUTPUTS})
        got["stats"] = statistics(self._stats)
        return r

    if defs:
        monkeypatch.setenv("DOMPC_DEFS", defs)
    else:
        monkeypatch.delenv("DOMPC_DEFS", raising=False)
    monkeypatch.setattr(HipIpmSolver, "__call__", rec)
    try:
        mpc = make_mpc(name, **kw)
        x0 = CASES[name].X0
        mpc.x0 = x0
        mpc.set_initial_guess()
        mpc.make_step(x0)
    finally:
        monkeypatch.undo()
    assert got, "the solver was not called"
    return mpc, got


def assert_same_bits(a, b, what):
    for key in OUTPUTS:
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key], equal_nan=True), (what, key)
    assert a["stats"] == b["stats"], (what, {k: (a["stats"][k], b["stats"].get(k)) for k in a["stats"] if a["stats"][k] != b["stats"].get(k)})


# ---- the device: the same cases plus the shipped CSTR, one problem alone and a batch that takes the one-wavefront launch shape
CASES_GPU = CASES_CPU + [("CSTR", "CSTR", {})]
IDS_GPU = [c[0] for c in CASES_GPU]
BATCH = 4096
WS_FILL = "255"          # DOMPC_WS_FILL: every byte of the workspace 0xff - a double read before it is written is a NaN


def batch_states(name, B=BATCH, seed=3):
    """B initial states around the example's X0 (1 +- 1 %); fixed, not modified by the tests"""
    x0 = np.asarray(CASES[name].X0, float).ravel()
    X0 = x0 * (1.0 + 0.01 * np.random.default_rng(seed).uniform(-1.0, 1.0, size=(B, x0.size)))
    X0[0] = x0
    X0.setflags(write=False)
    return X0


def batch_solve(make_mpc, name, kw, monkeypatch, defs, fill=False, B=BATCH, **call_kw):
    """(mpc, outputs and statistics) of one make_step_batch over batch_states(name, B) with the kernels built with the switches `defs`;
    fill: the workspace of the handle is pre-filled with WS_FILL"""
    if defs:
        monkeypatch.setenv("DOMPC_DEFS", defs)
    else:
        monkeypatch.delenv("DOMPC_DEFS", raising=False)
    if fill:
        monkeypatch.setenv("DOMPC_WS_FILL", WS_FILL)
    try:
        mpc = make_mpc(name, max_batch=B, **kw)
    finally:
        monkeypatch.undo()
    r = mpc.make_step_batch(batch_states(name, B), **call_kw)
    st = r["stats"]
    got = {key: np.array(r[key], dtype=np.float64, copy=True) for key in OUTPUTS}
    got["stats"] = {n: st[n].astype(np.float64).tolist() for n in st.dtype.names if not n.startswith("t_")}
    for key in ("du0dx0", "du0du_prev", "dxdp", "residual_step", "ok"):
        if key in r:
            got[key] = np.array(r[key], dtype=np.float64, copy=True)
    return mpc, got


def assert_finite(a, what):
    for key in OUTPUTS:
        assert np.all(np.isfinite(a[key])), (what, key)
