"""Inputs on which the four-edges-per-wavefront sweep (csrc/dompc_quad.h) takes its pivoting fallback for SOME quads only: numpy / scipy
restatements and searches, no GPU.

The register elimination of a quad runs in the natural pivot order and tests every pivot, |a_kk| >= GJ_U max |a_rk| over the rows of the
same group of four below it (GJ_U = 0.01); one failing pivot on one of its four edges sends the whole quad through the wavefront-per-edge
path (phase_edge_fallback).  No shipped workload ever fails the test (smallest ratio over the 180 edges at the initial guess: 4.28 for
industrial_poly, 3.71 for CSTR), so the inputs are made: ONE collocation unknown of an edge is moved to the value at which one pivot of
that edge's block G_cc passes through zero in the natural order.  The block itself stays well conditioned (partial pivoting has an easy
job) and every other edge of the problem is untouched - G_cc of an edge depends on the collocation unknowns of that edge only.

tests/test_quad_fallback_inputs.py holds the conditions on these inputs (CPU), tests/test_gpu_quad_fallback.py runs them."""
import numpy as np
from scipy.optimize import brentq

GJ_U = 0.01                   # DOMPC_GJ_U of the shipped build (csrc/dompc_factor.h)
FAIL_BELOW = 1e-4             # ratio of the crafted pivot: two orders of magnitude below the threshold ...
KEEP_ABOVE = 0.1              # ... every other pivot of the crafted edge one order above it
COND_BELOW = 1e4              # cond(G_cc) of a crafted edge
HEALTHY_ABOVE = 1.0           # smallest ratio of every edge that is not crafted: two orders above the threshold
OFF_ROOT = 1.0 + 1e-7         # the crafted value: the root of the pivot, moved off by this factor (a pivot that is small, not zero)


def structure_of(name, **over):
    """ProblemStructure of an example's controller without a solver behind it (no GPU, nothing compiled)"""
    from do_mpc_amd import controller
    from do_mpc_amd.examples import CASES

    class NoSolver:
        def __init__(self, *a, **k):
            pass
    orig = controller.HipIpmSolver
    controller.HipIpmSolver = NoSolver
    try:
        ex = CASES[name]
        return ex.build_mpc(ex.build_model(), **over).structure
    finally:
        controller.HipIpmSolver = orig


def pivot_ratios(G_cc):
    """The pivot test of eval_edge_quad / qd_fw_eliminate restated: unblocked Gauss-Jordan in the natural order, per pivot k the ratio
    |a_kk| / max |a_rk| over r = k+1 .. 4 (k / 4 + 1) - 1 (inf where that range is empty or zero).  Returns (ratios, pivots)."""
    A = np.array(G_cc, dtype=np.float64)
    R = A.shape[0]
    ratios, pivots = np.empty(R), np.empty(R)
    for k in range(R):
        hi = min(4 * (k // 4 + 1), R)
        m = np.max(np.abs(A[k + 1:hi, k])) if hi > k + 1 else 0.0
        pivots[k] = A[k, k]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratios[k] = abs(A[k, k]) / m if m > 0 else np.inf
            row = A[k] / A[k, k]
            col = A[:, k].copy()
            col[k] = 0.0
            A -= np.outer(col, row)
            A[k] = row
    return ratios, pivots


def edge_blocks(nlp, ps, x, p):
    """G_cc of every edge from the oracle's Jacobian: rows edge_row0[e] .. + deg nx, columns edge_w_off[e] .. + deg nx"""
    R = ps.deg * ps.nx
    J = nlp.jac(x, p).tocsr()
    out = []
    for e in range(ps.n_edges):
        r0, w0 = ps.tables["edge_row0"][e], ps.tables["edge_w_off"][e]
        out.append(J[r0:r0 + R][:, w0:w0 + R].toarray())
    return out


def min_ratios(nlp, ps, x, p):
    """(smallest pivot ratio, cond(G_cc)) of every edge"""
    G = edge_blocks(nlp, ps, x, p)
    return np.array([pivot_ratios(g)[0].min() for g in G]), np.array([np.linalg.cond(g) for g in G])


def predicted_fallback_quads(nlp, ps, x, p):
    """the quads (of four consecutive edges) in which at least one edge fails the kernel's pivot test at this iterate"""
    r, _ = min_ratios(nlp, ps, x, p)
    return sorted({int(e) // 4 for e in np.where(~(r >= GJ_U))[0]})


def _trial_blocks(nlp, ps, x, p, e, iv, values):
    """G_cc of edge e with its unknown iv set to each of `values`: (len(values), R, R).  The block of an edge is [s == jj] J_jj - C[s+1][jj+1] I
    with the dynamics Jacobians at the edge's own collocation points, so the oracle's Jacobian function is evaluated at those points only
    (oracle/nlp.py: jac) - a whole nlp.jac per trial value would make the search take minutes."""
    nx, nu, deg = ps.nx, ps.nu, ps.deg
    w0 = ps.tables["edge_w_off"][e]
    oe = int(np.where(nlp.col_blk == w0)[0][0])            # (the oracle's number of this edge)
    assert nlp.row0[oe] == ps.tables["edge_row0"][e] and nlp.ni == 1
    n = len(values)
    W = np.tile(x[w0:w0 + deg * nx].reshape(deg, nx), (n, 1, 1))
    W[:, iv // nx, iv % nx] = values
    U = x[nlp.col_u[oe] + np.arange(nu)]
    P = nlp._pvals(p)[oe]
    xs = W.reshape(n * deg, nx)
    cols = [xs[:, i] for i in range(nx)] + [np.full(n * deg, U[i]) for i in range(nu)] + [np.full(n * deg, P[i]) for i in range(nlp.nq)]
    with np.errstate(all="ignore"):                        # (a scan may step on a pole of the model, e.g. a temperature of zero: not finite, skipped)
        J = np.asarray(nlp.JF(cols, n * deg)).T.reshape(n, deg, nx, nx + nu)[..., :nx]
    G = np.zeros((n, deg, nx, deg, nx))
    for jj in range(deg):
        G[:, jj, :, jj, :] = J[:, jj]
        for s in range(deg):
            G[:, jj, np.arange(nx), s, np.arange(nx)] -= nlp.C[s + 1, jj + 1]
    return G.reshape(n, deg * nx, deg * nx)


def craft_edge(nlp, ps, x, p, e, which=0, span=40.0, grid=81):
    """(index into x, value, pivot): one collocation unknown of edge e and the value that makes one natural-order pivot of its G_cc
    (nearly) vanish while the block stays well conditioned.  Every unknown is scanned over x_i +- span max(1, |x_i|); at the first change
    of sign of a pivot Brent's method finds the root, which is moved off by OFF_ROOT.  Of the candidates that meet the three conditions
    of the module, in the order (unknown, pivot), number `which` is taken - the last one if there are fewer - so that the crafted edges
    of a problem do not all fail at the same pivot (tests/test_quad_fallback_inputs.py pins the outcome)."""
    R = ps.deg * ps.nx
    found = []
    w0 = ps.tables["edge_w_off"][e]
    for iv in range(R):
        i = w0 + iv
        vals = x[i] + np.linspace(-span, span, grid) * max(1.0, abs(x[i]))
        P = np.array([pivot_ratios(g)[1] for g in _trial_blocks(nlp, ps, x, p, e, iv, vals)])
        for k in range(R):
            flips = np.where(np.isfinite(P[:-1, k]) & np.isfinite(P[1:, k]) & (P[:-1, k] * P[1:, k] < 0))[0]
            if len(flips) == 0:
                continue
            q = flips[0]
            f = lambda v, iv=iv, k=k: pivot_ratios(_trial_blocks(nlp, ps, x, p, e, iv, [v])[0])[1][k]      # noqa: E731
            try:
                v = brentq(f, vals[q], vals[q + 1], xtol=1e-15, rtol=1e-15) * OFF_ROOT
            except (ValueError, RuntimeError):
                continue
            g = _trial_blocks(nlp, ps, x, p, e, iv, [v])[0]
            r, _ = pivot_ratios(g)
            if np.all(np.isfinite(g)) and r[k] < FAIL_BELOW and np.linalg.cond(g) < COND_BELOW and np.delete(r, k).min() > KEEP_ABOVE:
                found.append((int(i), float(v), k))
                if len(found) > which:
                    return found[-1]
    if found:
        return found[-1]
    raise AssertionError(f"no collocation unknown of edge {e} makes a pivot vanish under the conditions of tests/quad_common.py")


def craft(nlp, ps, x, p, edges, cache=None):
    """the iterate x with one unknown of each edge in `edges` changed (craft_edge); `cache`: a dict shared by the calls at one (x, p)"""
    cache = {} if cache is None else cache
    xc = np.array(x, dtype=np.float64)
    for e in edges:
        if e not in cache:
            cache[e] = craft_edge(nlp, ps, x, p, e, which=e % 3)
        i, v, _ = cache[e]
        xc[i] = v
    return xc


def patterns(n_edges, ng=4):
    """{name: edges to craft}.  Quads are dealt to the `ng` wavefronts of a problem round-robin (ng = 4: 256-thread workgroup, ng = 1:
    block_threads = 64), so wavefront q % ng handles quads q, q + ng, ...: `consecutive` makes ONE wavefront fall back twice in a row,
    `neighbours` two wavefronts side by side (with one wavefront per problem `neighbours` IS the consecutive case).  Problems with fewer than
    five quads get the patterns that exist for them."""
    nq = (n_edges + 3) // 4
    big = nq >= 2 * ng + 3
    out = {"none": [], "first": [1 if big else 0], "last": [min(4 * (nq - 1) + 2, n_edges - 1)]}
    if big:
        q = nq // 2
        for g in range(4):
            out[f"row{g}"] = [4 * q + g]
        out["consecutive"] = [4 * q + 1, 4 * (q + ng) + 2]
        out["whole"] = [4 * q + g for g in range(4)]
        out["neighbours"] = [4 * q + 3, 4 * (q + 1)]
    return out


def quads_of(edges):
    return sorted({e // 4 for e in edges})
