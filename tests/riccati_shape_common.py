"""The backward Riccati pass at the shapes no shipped model reaches - checks shared by the host-emulation (CPU CI) and the HIP (-m gpu)
test modules.

The matrix-core recursion (csrc/dompc_riccati16.h) keeps a node's quadratic over z = (x, u_prev, u, eps) in one 16 x 16 tile with the
vectors in row / column NA; its index arithmetic (HR = NA / 4, HG = NA % 4, the k-block counts KB_A, KB_H, KB_Y, the decision entries
NA .. NA + NV - 1, the slack columns, yz()) has cases the shipped models (NA = 5, 6, 10, 13) never select.  The synthetic family of
do_mpc_amd/examples/shape_family.py selects them (MEMBERS below), plus the two sizes one past the limits, which must take the generic
recursion.  The host emulation always runs the generic recursion: there these checks validate the family, its lowering, the oracle case
(oracle/models.py: case_shape_family) and the sparse reference with nl_cons rows (parity_common.newton_reference) before a GPU is used.
[NO REFERENCE FIXTURE: the family does not exist in the reference; oracle-or-equivalence checks, not reproductions]
"""
import numpy as np

import differentiator_common as dc
import parity_common as pc
from do_mpc_amd.examples import CASES
from oracle import ipm

# id -> (nx, nu, n_soft, n_hard, NA, NV, NYT, NE, recursion the device runs: 1 = matrix-core tile, 0 = generic)
MEMBERS = {
    "s1": (1, 1, 0, 0, 2, 1, 3, 0, 1),        # smallest tile, KB_H = 1
    "s2": (3, 1, 0, 0, 4, 1, 5, 0, 1),        # HG = 0, KB_H = 2 > KB_A = 1
    "s3": (5, 2, 1, 1, 7, 3, 10, 2, 1),       # decision entries 7, 8, 9 straddle registers 1 and 2; a hard and a soft row
    "s4": (6, 2, 2, 2, 8, 4, 12, 4, 1),       # NV = 4, NE = 4, NS = 2, HG = 0
    "s5": (8, 4, 0, 0, 12, 4, 16, 0, 1),      # NU = 4, HG = 0, HR = 3, full tile
    "s6": (10, 2, 2, 1, 12, 4, 16, 3, 1),     # slacks in tile columns 14 and 15
    "s7": (14, 1, 0, 0, 15, 1, 16, 0, 1),     # NA = 15 (the limit), HR = HG = 3; wavefront-per-edge sweep
    "s8": (9, 4, 0, 0, 13, 4, 17, 0, 0),      # one past NYT <= 16
    "s9": (4, 2, 1, 4, 6, 3, 9, 5, 0),        # one past NE <= 4
}
IDS = sorted(MEMBERS)
DELTAS = (0.0, 0.05)

# Newton direction against the sparse KKT solve: max |dx - dx_ref| / max |dx_ref| at the oracle's iterate 6 from the family's X0.
# HOST_DX: the deviation of the HOST EMULATION from the sparse reference (same algebra, other code: the rounding level of the algorithm
# at that iterate), measured, per (member, delta_w); the bound of the GPU test is 100 x that value (the matrix-core products sum in
# another order), at most parity_common.STEP_TOL.  Source: profiles/riccati_shapes.txt (which also holds what the GPU measured - no
# bound comes from there).
HOST_DX = {
    ("s1", 0.0): 1.16e-12, ("s1", 0.05): 1.16e-12,
    ("s2", 0.0): 2.90e-11, ("s2", 0.05): 2.90e-11,
    ("s3", 0.0): 1.24e-16, ("s3", 0.05): 3.40e-14,
    ("s4", 0.0): 2.07e-17, ("s4", 0.05): 3.06e-14,
    ("s5", 0.0): 4.80e-14, ("s5", 0.05): 6.16e-14,
    ("s6", 0.0): 1.75e-16, ("s6", 0.05): 2.52e-13,
    ("s7", 0.0): 1.46e-08, ("s7", 0.05): 1.46e-08,
    ("s8", 0.0): 1.41e-13, ("s8", 0.05): 7.81e-14,
    ("s9", 0.0): 2.07e-17, ("s9", 0.05): 3.39e-14,
}


def name_of(mid):
    return "shape_family:" + mid


def gpu_dx_bound(mid, delta):
    return min(100.0 * HOST_DX[(mid, delta)], pc.STEP_TOL)


def check_shape(mpc, mid):
    """the lowered problem has the sizes of the table"""
    nx, nu, n_soft, n_hard, na, nv, nyt, ne, _ = MEMBERS[mid]
    ps = mpc.structure
    assert (ps.nx, ps.nu, ps.ns, ps.ne) == (nx, nu, n_soft, n_soft + n_hard)
    assert (ps.nx + ps.nu, ps.nu + ps.ns, ps.nx + 2 * ps.nu + ps.ns, ps.ne) == (na, nv, nyt, ne)
    assert (ps.N, ps.S, ps.M) == (4, 3, 3)            # horizon 4, a root with three children and three chains, Radau degree 2


_cold = {}


def oracle_cold_solve(mid):
    """(nlp, p, result) of the oracle's cold solve from the family's X0 - computed once, not modified by the tests"""
    if mid not in _cold:
        nlp = pc.oracle_nlp(name_of(mid))
        x0 = CASES[name_of(mid)].X0
        p = nlp.opt_p(x0, np.zeros(nlp.nu))
        _cold[mid] = (nlp, p, ipm.solve(nlp, nlp.initial_guess(x0), p))
    return _cold[mid]


def active_set(nlp, x, lam_g, p):
    """(input bounds active, soft rows active, hard rows active) at a solution: a bound counts when the variable is within 1e-6 of it,
    a row when its value (minus its slack) is within 1e-6 of ub and its multiplier is above 1e-3"""
    U = x[nlp.off_u:nlp.off_eps].reshape(-1, nlp.nu)
    lo, hi = np.asarray(nlp.case["u_lb"]) / nlp.su, np.asarray(nlp.case["u_ub"]) / nlp.su
    n_u = int(np.sum((np.abs(U - lo) < 1e-6) | (np.abs(U - hi) < 1e-6)))
    if nlp.ne == 0:
        return n_u, 0, 0
    rows = nlp.row0[:, None] + nlp.rows_per_edge - nlp.ne + np.arange(nlp.ne)[None, :]
    act = (np.abs(nlp.g(x, p)[rows] - nlp.ubg[rows]) < 1e-6) & (lam_g[rows] > 1e-3)
    soft = np.zeros(nlp.ne, bool)
    soft[nlp.soft] = True
    return n_u, int(act[:, soft].sum()), int(act[:, ~soft].sum())


def check_active_set_condition(mid, counts):
    n_u, n_soft, n_hard = counts
    assert n_u >= 1, (mid, counts)
    if MEMBERS[mid][7] > 0:
        assert n_soft >= 1 and n_hard >= 1, (mid, counts)


def check_oracle_active_set(mid):
    """The condition on the family's inputs, with the oracle alone: its cold solve converges without a failed line search (the oracle has
    no restoration phase: n_ls_fail counts where IPOPT would enter it) and ends with an input bound active and, for members with
    nl_cons rows, a soft and a hard row active."""
    nlp, p, r = oracle_cold_solve(mid)
    assert r["stats"]["success"] and r["stats"]["n_ls_fail"] == 0, r["stats"]["return_status"]
    check_active_set_condition(mid, active_set(nlp, r["x"], r["lam_g"], p))


def check_newton_direction(make_mpc, mid, delta, step_tol, report=None):
    """parity_common.check_newton_step on a member: c, rd and the residual of the full system with its bounds, dx with `step_tol`"""
    report = {} if report is None else report
    try:
        mpc = pc.check_newton_step(make_mpc, name_of(mid), delta=delta, step_tol=step_tol, report=report)
    finally:
        print("riccati_shapes newton %s delta_w=%g dx=%.3e (bound %.3e) c=%.1e rd=%.1e residual=%.1e dlam=%.1e" % (
            mid, delta, report.get("dx", np.nan), step_tol, report.get("c", np.nan), report.get("rd", np.nan), report.get("res", np.nan),
            report.get("dlam", np.nan)))
    check_shape(mpc, mid)
    return report


def check_cold_solve(make_mpc, mid):
    """same iterations as the oracle from the family's X0 (count, regularisations, every used variable, multipliers), and the active-set
    condition from the PRODUCT's solution: the bound, slack and row paths did real work"""
    name = name_of(mid)
    mpc = pc.check_same_iterates_as_oracle(make_mpc, name, x0=CASES[name].X0)
    check_shape(mpc, mid)
    nlp = pc.oracle_nlp(name)
    check_active_set_condition(mid, active_set(nlp, mpc.opt_x_num.master, mpc.lam_g_num, mpc.opt_p_num.master))
    return mpc


def check_batch_members(make_mpc, mid, B=5, seed=7):
    """make_step_batch on B distinct initial states X0 (1 +- 2 %) against B single make_step calls (the convention of
    test_batch_is_deterministic_and_equals_single_solves: u0 to 1e-9), and twice for equal bits"""
    name = name_of(mid)
    ex = CASES[name]
    rng = np.random.default_rng(seed)
    X0 = ex.X0 * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, size=(B, ex.X0.size)))
    mpc = make_mpc(name, max_batch=B)
    r = mpc.make_step_batch(X0)
    assert r["stats"]["success"].all(), r["stats"]["status"]
    r2 = mpc.make_step_batch(X0)
    assert np.array_equal(r["x"], r2["x"]) and np.array_equal(r["lam_g"], r2["lam_g"])
    assert len({r["x"][i].tobytes() for i in range(B)}) == B                     # (distinct problems)
    for i in range(B):
        m1 = make_mpc(name)                     # (a fresh controller per member: no previous input, no warm start)
        m1.x0 = X0[i]
        m1.set_initial_guess()
        u = m1.make_step(X0[i]).ravel()
        assert m1.solver_stats["success"]
        assert pc.relerr(r["u0"][i], u) < 1e-9, (i, r["u0"][i], u)
    return mpc


def check_sensitivities(make_mpc, mid="s3"):
    """differentiator_common.check_against_oracle_kkt on a member with several nl_cons rows (the oracle's KKT system with its slack block)"""
    return dc.check_against_oracle_kkt(make_mpc, name_of(mid))
