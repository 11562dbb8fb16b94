"""The four-edges-per-wavefront sweep and forward pass (csrc/dompc_quad.h) on problems in which SOME quads fail the pivot test of the
register elimination and take the wavefront-per-edge fallback while the quads around them do not.  No shipped workload reaches that code
(tests/quad_common.py makes the inputs, tests/test_quad_fallback_inputs.py checks them on the CPU), the kernels have no host-emulation
twin, and the -DDOMPC_GJ_U=1e9 build of test_pivoting_fallback_of_the_factorisation sends EVERY quad through the fallback: what happens
around ONE fallback - the LDS-DMA in flight, the bank the next quad is requested into, the edge pack re-read behind the call, the verdict
the forward pass reaches on its own - is checked here only."""
import functools

import numpy as np
import pytest

import parity_common as pc
import quad_common as qc
from do_mpc_amd.examples import CASES
from oracle import ipm

pytestmark = pytest.mark.gpu

FIVE_EDGES = dict(n_horizon=5, n_robust=0)      # CSTR: two quads, the last one with one live row and three idle rows that repeat it
SAME_QUANTITY = 1e-9                            # "same quantity, other elimination order" (test_pivoting_fallback_of_the_factorisation)
ADJ_MU = 10.0                                   # DOMPC_ADJ_MU (csrc/dompc_edge.h): the adjoint forward pass runs from mu <= ADJ_MU tol on


def make_mpc(name, **kw):
    ex = CASES[name]
    return ex.build_mpc(ex.build_model(), **kw)


class DevArr:
    def __init__(self, a):
        import torch
        self.t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
        self.ptr = self.t.data_ptr()

    def host(self):
        import torch
        torch.cuda.synchronize()
        return self.t.cpu().numpy()


def _sweep(mpc, X, LAM, P):
    """(g, records) of one dompc_sweep_batch_device call over the rows of X"""
    ps, B = mpc.structure, X.shape[0]
    dX, dL, dP = DevArr(X), DevArr(LAM), DevArr(P)
    dG, dB = DevArr(np.zeros((B, ps.n_g))), DevArr(np.zeros((B, ps.n_edges, mpc.S.sweep_block_doubles)))
    mpc.S.sweep_batch_device(B, dX.ptr, dL.ptr, dP.ptr, dG.ptr, dB.ptr)
    return dG.host(), dB.host()


@functools.lru_cache(maxsize=None)
def _sweep_inputs(name, five):
    """the patterns of quad_common.patterns() as the rows of one batch, `last` and `none` again behind them - and for a problem whose last quad
    is partial `none` once more in the middle: (nlp, names, edges per row, X, LAM, P)"""
    over = FIVE_EDGES if five else {}
    ps = qc.structure_of(name, **over)
    nlp = pc.oracle_nlp(name, **over)
    ex = CASES[name]
    x, p = nlp.initial_guess(ex.X0), nlp.opt_p(ex.X0, np.zeros(nlp.nu))
    pats = qc.patterns(ps.n_edges, 4)
    names = list(pats) + (["none"] if ps.n_edges % 4 else []) + ["last", "none"]
    cache = {}
    X = np.stack([qc.craft(nlp, ps, x, p, pats[k], cache) for k in names])
    lam = np.random.default_rng(11).standard_normal(ps.n_g)
    for a in (X, lam):
        a.setflags(write=False)
    return nlp, names, [pats[k] for k in names], X, np.tile(lam, (len(names), 1)), np.tile(p, (len(names), 1))


def _parts(ps):
    nx, na = ps.nx, ps.nx + ps.nu
    cuts = np.cumsum([0, nx * na, nx, na * na, na])
    return [("[A B]", cuts[0], cuts[1]), ("c", cuts[1], cuts[2]), ("Q~", cuts[2], cuts[3]), ("q~", cuts[3], cuts[4])]


@pytest.mark.parametrize("name,five", [("industrial_poly", False), ("CSTR", False), ("CSTR", True)], ids=["industrial_poly", "CSTR", "CSTR_five_edges"])
def test_sweep_records_when_some_quads_fall_back(name, five, monkeypatch):
    """Every pattern of tests/quad_common.py as one iterate of ONE sweep launch (12 iterates of a 180-edge problem; 6 of the five-edge one),
    in the 256-thread launch shape (four wavefronts per problem) and with block_threads = 64 (one wavefront walks all quads: the longest
    prefetch chain behind a fallback), against
      1. the oracle: g, [A B] and c of every edge (dense float64 solve per edge, bounds of test_sweep_blocks_match_oracle_jacobian);
      2. the wavefront-per-edge build (-DDOMPC_QUAD=0) of the same model, whole record [A B | c | Q~ | q~ + r_y]: the four edges of a quad
         that is PREDICTED to fall back bit for bit - both builds run eval_edge_coop there, one wavefront per edge, and neither its group
         size (64 in both) nor what is staged for it enters its arithmetic - and every other edge to 1e-9 max(1, max |part|) per edge and
         part (the project's bound for the same quantity from another elimination order);
      3. the prediction: every quad predicted healthy differs from the per-edge build in at least one bit (pattern `none`: all of them) -
         a kernel that took the fallback everywhere would pass 2. trivially.
    Rows of the batch with the same iterate give the same bits, and so do the two launch shapes.
    The five-edge CSTR is the problem with a PARTIAL last quad: edge 4 and three idle rows that repeat it.  Until this test existed the
    idle rows took their model-output record from the bytes that stage_quad() copies from behind the last record of the problem, built
    columns from them and voted in the pivot test, so that the last quad fell back - or not - with the contents of memory the sweep does
    not own (first MI355X run: pattern `none` fell back in quad 1, predicted none), and the forward pass could reach another verdict than
    the sweep.  The idle rows now read the last edge's record.  What probes those bytes is the row order: `none` is the first, a middle
    and the last problem of the batch, `last` a middle one twice, each with its own workspace slot and its own neighbours behind the
    record; all copies must give the same bits and the predicted quads.
    Quads on the fallback per pattern, measured on MI355X = predicted.  industrial_poly and CSTR (180 edges): none 0, first 1 (quad 0),
    last 1 (quad 44), row0 .. row3 1 each (quad 22), consecutive 2 (22, 26), whole 1 (22), neighbours 2 (22, 23).  Five-edge CSTR: none 0,
    first 1 (quad 0), last 1 (quad 1).  The fallen-back quads have the per-edge build's bits, in both launch shapes.  Worst quad vs
    per-edge deviation over the healthy edges, relative to max(1, max |part|): industrial_poly 6.0e-13, CSTR 8.0e-15, five-edge CSTR
    1.7e-15."""
    over = FIVE_EDGES if five else {}
    nlp, names, edges, X, LAM, P = _sweep_inputs(name, five)
    B = len(names)
    quad256 = make_mpc(name, max_batch=16, **over)
    quad64 = make_mpc(name, max_batch=16, block_threads=64, **over)
    assert quad256.S.edges_per_wavefront == 4 and quad64.S.edges_per_wavefront == 4 and quad64.S.batch_object_state == 1
    monkeypatch.setenv("DOMPC_DEFS", "DOMPC_QUAD=0")
    per_edge = make_mpc(name, max_batch=16, **over)
    monkeypatch.delenv("DOMPC_DEFS")
    assert per_edge.S.edges_per_wavefront == 1 and per_edge.S.code_object_path != quad256.S.code_object_path
    ps = quad256.structure
    assert np.array_equal(ps.tables["edge_row0"], nlp.row0) and np.array_equal(ps.tables["edge_w_off"], nlp.col_blk)
    G, R = _sweep(quad256, X, LAM, P)
    G64, R64 = _sweep(quad64, X, LAM, P)
    Ge, Re = _sweep(per_edge, X, LAM, P)
    assert np.all(np.isfinite(R)) and np.all(np.isfinite(Re)) and np.all(np.isfinite(G))
    # ---- 1. the oracle
    for b in range(B):
        pc.assert_sweep_records_match_oracle(ps, nlp, X[b], P[b], G[b], R[b])
    # ---- 2. and 3. the wavefront-per-edge build, quad by quad
    nq = (ps.n_edges + 3) // 4
    worst = 0.0
    for b in range(B):
        predicted = qc.quads_of(edges[b])
        assert predicted == qc.predicted_fallback_quads(nlp, ps, X[b], P[b])
        same = [q for q in range(nq) if np.array_equal(R[b, 4 * q:4 * q + 4], Re[b, 4 * q:4 * q + 4])]
        print(f"{name} {over} {names[b]}: crafted edges {edges[b]}, quads that fell back (same bits as the per-edge build) {same}, predicted {predicted}")
        assert same == predicted, (names[b], same, predicted)
        for e in range(ps.n_edges):
            if e // 4 in predicted:
                continue
            for part, lo, hi in _parts(ps):
                dev = np.max(np.abs(R[b, e, lo:hi] - Re[b, e, lo:hi])) / max(1.0, np.max(np.abs(Re[b, e, lo:hi])))
                worst = max(worst, dev)
                assert dev <= SAME_QUANTITY, (names[b], e, part, dev)
        assert np.max(np.abs(G[b] - Ge[b])) <= SAME_QUANTITY * max(1.0, np.max(np.abs(Ge[b])))
    print(f"{name} {over}: worst quad vs per-edge deviation over the healthy edges, relative to max(1, max |part|): {worst:.2e}")
    # ---- the same iterate: the same bits, in whichever row and launch shape
    assert names[-2:] == ["last", "none"] and names.count("none") == (3 if ps.n_edges % 4 else 2) and names.count("last") == 2
    for j in range(B):
        i = names.index(names[j])
        assert np.array_equal(R[i], R[j]) and np.array_equal(G[i], G[j]), (names[j], i, j)
    assert np.array_equal(R, R64) and np.array_equal(G, G64)


@functools.lru_cache(maxsize=None)
def _newton_inputs(pattern):
    """industrial_poly: the oracle's iterate and multipliers after 6 iterations (interior), the iterate crafted by `pattern`, the oracle's
    relaxed box with infinite bounds on the crafted entries: (nlp, p, x, lam, lb, ub)"""
    name = "industrial_poly"
    ps = qc.structure_of(name)
    nlp = pc.oracle_nlp(name)
    assert nlp.ne == 0
    ex = CASES[name]
    p = nlp.opt_p(ex.X0, np.zeros(nlp.nu))
    r = _oracle_six_iterations()
    x0, lam = r["x"], r["lam_g"] * r["stats"]["obj_scaling"]
    edges = qc.patterns(ps.n_edges, 4)[pattern]
    x = qc.craft(nlp, ps, x0, p, edges)
    crafted = np.where(x != x0)[0]
    assert len(crafted) == len(edges)
    # the conditions of tests/test_quad_fallback_inputs.py at THIS iterate
    ratio, cond = qc.min_ratios(nlp, ps, x, p)
    assert all(ratio[e] < qc.FAIL_BELOW and cond[e] < qc.COND_BELOW for e in edges) and np.delete(ratio, edges).min() > qc.HEALTHY_ABOVE
    lb, ub = nlp.lbx.copy(), nlp.ubx.copy()
    hl, hu = np.isfinite(lb), np.isfinite(ub)
    lb[hl] -= 1e-8 * np.maximum(1, np.abs(lb[hl]))
    ub[hu] += 1e-8 * np.maximum(1, np.abs(ub[hu]))
    lb[crafted], ub[crafted] = -np.inf, np.inf
    return nlp, p, x, lam, lb, ub


@functools.lru_cache(maxsize=None)
def _oracle_six_iterations():
    nlp = pc.oracle_nlp("industrial_poly")
    X0 = CASES["industrial_poly"].X0
    return ipm.solve(nlp, nlp.initial_guess(X0), nlp.opt_p(X0, np.zeros(nlp.nu)), opts=dict(max_iter=6))


def _reference_with_inertia(mpc, pattern, mu):
    """newton_reference() at the smallest delta_w of (0, 0.05, 1.0) for which the KKT matrix is SHOWN to have the inertia (n, m, 0) - by the
    oracle's exact count (sparse LDL' without interchanges; where it cannot count, as at delta_w = 0 with the Hessian's zero rows, the
    inertia is not shown and the next value is tried): a NaN direction from the kernel is then the kernel's failure, not the input's"""
    nlp, p, x, lam, lb, ub = _newton_inputs(pattern)
    for delta in (0.0, 0.05, 1.0):
        ref = pc.newton_reference(mpc, nlp, x, lam, lb, ub, mu, delta, p)
        if ipm._n_negative_sparse(ref["H"], ref["A"], 0.0) == ref["A"].shape[0]:
            assert delta == 0.05                 # (the value the docstrings state: a drift to 1.0 would go unnoticed otherwise)
            return ref, delta
    raise AssertionError("no delta_w with the inertia (n, m, 0)")


def _mu_of(mpc, kind):
    mu = {"forms_inverses_again": 0.1, "adjoint_reads_stored_inverses": 0.5 * ADJ_MU * float(mpc.S.options.tol)}[kind]
    assert (mu <= ADJ_MU * float(mpc.S.options.tol)) == (kind == "adjoint_reads_stored_inverses")
    return mu


@pytest.mark.parametrize("kind", ["forms_inverses_again", "adjoint_reads_stored_inverses"])
@pytest.mark.parametrize("pattern", ["row2", "last", "consecutive"])
def test_newton_direction_with_a_mixed_quad(pattern, kind):
    """One Newton direction (sweep, backward pass, forward pass) of industrial_poly with one or two quads on the fallback, against a sparse
    LU of the same KKT system (assertions of check_newton_step: c, r_d, dx within STEP_TOL, linear residual below 1e-7).
    mu = 0.1: the sweep stores G_cc^-1 for the quads that fell back only (lu_store_rule), the four-edge forward pass forms the inverses
    again, has to reach the sweep's verdict for every quad by itself and reads the stored inverse where it falls back.
    mu = 5 tol: the adjoint variant of the forward pass - every edge reads a stored inverse, written by the quad path or by the fallback.
    delta_w = 0.05 in all six cases (at 0 the Hessian's zero rows keep the oracle's count from showing the inertia); passes on MI355X."""
    mpc = make_mpc("industrial_poly")
    assert mpc.S.edges_per_wavefront == 4
    nlp, p, x, lam, lb, ub = _newton_inputs(pattern)
    mu = _mu_of(mpc, kind)
    ref, delta = _reference_with_inertia(mpc, pattern, mu)
    print(f"{pattern} {kind}: mu = {mu:g}, delta_w = {delta:g}, max |dx| of the reference {np.max(np.abs(ref['dx'])):.4g}")
    pc.check_newton_step_at(mpc, nlp, x, lam, lb, ub, mu, delta, p, ref=ref)


@pytest.mark.parametrize("kind", ["forms_inverses_again", "adjoint_reads_stored_inverses"])
@pytest.mark.parametrize("pattern", ["row2", "last", "consecutive"])
def test_newton_direction_with_a_mixed_quad_equals_the_all_fallback_build(pattern, kind, monkeypatch):
    """... and against the build in which EVERY quad takes the fallback (-DDOMPC_GJ_U=1e9), the anchor for the parts of the records that have
    no oracle: the same direction to 1e-9 (relative to max(1, |dx|)), not the same bits (the healthy quads ran the register elimination).
    Measured on MI355X: 1.6e-12 at mu = 0.1, 9.5e-13 .. 1.1e-12 at mu = 5 tol."""
    nlp, p, x, lam, lb, ub = _newton_inputs(pattern)
    dx = []
    for defs in ("", "DOMPC_GJ_U=1e9"):
        monkeypatch.setenv("DOMPC_DEFS", defs)
        mpc = make_mpc("industrial_poly")
        mu = _mu_of(mpc, kind)
        ref, delta = _reference_with_inertia(mpc, pattern, mu)
        dx.append(mpc.S.debug_newton_step(x, lam, ref["zl"], ref["zu"], lb, ub, nlp.lbg, nlp.ubg, p, mu, delta)[0])
    assert np.all(np.isfinite(dx[0])) and np.all(np.isfinite(dx[1]))
    print(f"{pattern} {kind}: default build vs all-fallback build, relerr of dx {pc.relerr(dx[0], dx[1]):.2e}")
    assert pc.relerr(dx[0], dx[1]) < SAME_QUANTITY
    assert not np.array_equal(dx[0], dx[1])
