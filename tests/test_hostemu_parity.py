"""IPM logic on the TEST-ONLY host emulation of the device code (tests/hostemu.py): the same kernel
text as the gfx950 code object, one workgroup = one host thread.  Runs in the GPU-less CI container;
the -m gpu twin of this module (test_gpu_parity.py) runs the real HIP path."""
import os

import numpy as np
import pytest

import hostemu
import parity_common as pc
from do_mpc_amd.examples import CASES


def make_mpc(name, **kw):
    ex = CASES[name]
    with hostemu.patched():
        return ex.build_mpc(ex.build_model(), **kw)


@pytest.mark.parametrize("name,steps", [("oscillating_masses", 5), ("batch_reactor", 5), ("CSTR", 3), ("industrial_poly", 2),
                                        ("rotating_masses", 5), ("oscillating_masses_dae", 5), ("dip", 2)])
def test_golden_replay(name, steps):
    pc.check_golden_replay(make_mpc, name, steps)


@pytest.mark.parametrize("name", ["oscillating_masses", "batch_reactor", "industrial_poly", "rotating_masses",
                                  "oscillating_masses_dae", "CSTR"])      # (CSTR: nl_cons row and slack in the sparse reference)
def test_newton_direction_matches_sparse_kkt_solve(name):
    pc.check_newton_step(make_mpc, name)


@pytest.mark.parametrize("name", ["batch_reactor", "industrial_poly", "CSTR"])
def test_newton_direction_with_inertia_correction(name):
    """delta_w > 0: W'W and W'w0 of every edge are formed on demand from the stored W"""
    pc.check_newton_step(make_mpc, name, delta=0.05)


@pytest.mark.parametrize("name", ["oscillating_masses", "batch_reactor", "industrial_poly", "rotating_masses"])
def test_sweep_blocks_match_oracle_jacobian(name):
    mpc = make_mpc(name)
    pc.check_sweep_blocks(mpc, name, pc.HostArr, lambda d: d.a)


@pytest.mark.parametrize("name,opts", [("batch_reactor", None), ("rotating_masses", None),
                                       ("industrial_poly", None), ("CSTR", None)])
def test_same_iterates_as_the_oracle(name, opts):
    """IPOPT regularises every iteration of these problems (free unused variables make its matrix singular at delta_w = 0);
    the driver mirrors the delta_w sequence and keeps the bounded unused variables in the barrier problem."""
    mpc = pc.check_same_iterates_as_oracle(make_mpc, name, oracle_opts=opts)
    assert mpc.solver_stats["n_reg"] == mpc.solver_stats["iter_count"]


def _create_nlp(mpc):
    with hostemu.patched():
        mpc.create_nlp()


# continuous models with the docstring's example: the terms in the collocation states send the model through the dense edge path, which has no
# adjoint recovery of the continuity multipliers - same iterations, primal 2e-12, multipliers of the flat direction next to
# active state bounds 1.5e-4 of the largest (1.2 on 3 299); both multiplier vectors are stationary to 1e-9 (asserted in the check)
_XTRA_LAM_TOL = {("industrial_poly", "docstring"): 5e-4}


@pytest.mark.parametrize("name,which", [("oscillating_masses", "docstring"), ("oscillating_masses", "tree"), ("industrial_poly", "tree"),
                                        ("CSTR", "tree"), ("batch_reactor", "tree"), ("oscillating_masses_dae", "tree"),
                                        ("rotating_masses", "tree"), ("CSTR", "docstring"), ("batch_reactor", "docstring"),
                                        ("industrial_poly", "docstring")])
def test_cost_terms_added_to_nlp_obj_same_iterates_as_the_oracle(name, which):
    """optimizer.py:82-129: `nlp_obj += ...` between prepare_nlp() and create_nlp(), node-local terms (the docstring's own example among them)"""
    pc.check_added_cost_terms(make_mpc, _create_nlp, name, which, lam_tol=_XTRA_LAM_TOL.get((name, which), 1e-5))


@pytest.mark.parametrize("name,with_cost", [("oscillating_masses", False), ("CSTR", False), ("CSTR", True), ("industrial_poly", False),
                                            ("industrial_poly", True), ("batch_reactor", False), ("rotating_masses", False)])
def test_rows_appended_to_nlp_cons_same_iterates_as_the_oracle(name, with_cost):
    """optimizer.py:131-215: node-local inequality rows appended to nlp_cons between prepare_nlp() and create_nlp() (extra row slots of the
    node's first outgoing edge; g / lam_g come back in the reference's row order), alone and together with added cost terms"""
    pc.check_added_rows(make_mpc, _create_nlp, name, with_cost=with_cost)


@pytest.mark.parametrize("name,over", pc.NONCONVEX_CASES)
def test_nonconvex_examples_reach_the_oracles_local_solution(name, over):
    """Second-order correction + inertia correction: same local minimum as the IPOPT-default oracle with exact inertia."""
    mpc = pc.check_against_oracle_solve(make_mpc, name, oracle_opts=dict(inertia="ldl"), **over)
    if name == "kinematic_bicycle":
        assert mpc.solver_stats["n_soc"] >= 1          # (the case that needs the correction)


def test_second_order_correction_can_be_switched_off():
    """ipopt.max_soc = 0 reproduces the oracle without the correction (another local minimum of the kinematic bicycle)."""
    from oracle import ipm
    mpc = make_mpc("kinematic_bicycle", nlpsol_opts={"ipopt.max_soc": 0})
    ex = CASES["kinematic_bicycle"]
    mpc.x0 = ex.X0
    mpc.set_initial_guess()
    u0 = mpc.make_step(ex.X0).ravel()
    assert mpc.solver_stats["success"] and mpc.solver_stats["n_soc"] == 0
    nlp = pc.oracle_nlp("kinematic_bicycle")
    r = ipm.solve(nlp, nlp.initial_guess(ex.X0), nlp.opt_p(ex.X0, np.zeros(nlp.nu)), opts=dict(inertia="ldl", max_soc=0))
    assert pc.relerr(u0, nlp.u0_of(r["x"])) < pc.U_RTOL
    r4 = ipm.solve(nlp, nlp.initial_guess(ex.X0), nlp.opt_p(ex.X0, np.zeros(nlp.nu)), opts=dict(inertia="ldl"))
    assert pc.relerr(u0, nlp.u0_of(r4["x"])) > 1e-2    # (the two local minima are far apart)


def test_second_order_corrections_on_the_benchmark_problems_do_not_move_their_solutions():
    """industrial_poly cold solves of the benchmark's x0 batch: corrections are tried on some of them (accepted and rejected
    ones - the rejected path restores the Newton direction from its copy); same solutions as without them (one optimum)."""
    import bench
    X0 = bench.synthetic_x0_batch(8)
    res = []
    for soc in (4, 0):
        mpc = make_mpc("industrial_poly", max_batch=8, nlpsol_opts={"ipopt.max_soc": soc})
        r = mpc.make_step_batch(X0)
        assert np.all(r["stats"]["success"] != 0)
        res.append(r)
    st4, st0 = res[0]["stats"], res[1]["stats"]
    assert st4["n_soc"].sum() >= 1 and st0["n_soc"].sum() == 0
    # one sweep per iteration + the first (which also serves the least-squares multiplier estimate; the objective is not
    # rescaled on this problem) + the sweep at the estimate + one per correction
    assert np.array_equal(st4["n_sweeps"], st4["iter_count"] + 2 + st4["n_soc"])
    assert pc.relerr(res[0]["u0"], res[1]["u0"]) < 1e-7


def test_baseline_config_cstr_nominal_deg3_vs_oracle():
    # BASELINE.json configs[1]: CSTR nominal NMPC, N=20, collocation deg 3 (no fixture -> oracle)
    pc.check_against_oracle_solve(make_mpc, "CSTR", n_robust=0, collocation_deg=3)


def test_baseline_config_batch_reactor_n50_vs_oracle():
    # BASELINE.json configs[2]: batch_reactor economic NMPC, N=50
    pc.check_against_oracle_solve(make_mpc, "batch_reactor", n_horizon=50)


def test_batch_api_equals_single_solves():
    mpc = make_mpc("batch_reactor", max_batch=4)
    ex = CASES["batch_reactor"]
    rng = np.random.default_rng(5)
    X0 = ex.X0 * (1 + 0.05 * rng.uniform(-1, 1, size=(4, 4)))
    r = mpc.make_step_batch(X0)
    assert r["stats"]["success"].all()
    for i in range(4):
        m1 = make_mpc("batch_reactor")
        m1.x0 = X0[i]
        m1.set_initial_guess()
        u = m1.make_step(X0[i]).ravel()
        assert np.allclose(r["u0"][i], u, rtol=1e-12, atol=1e-14)


def test_empty_batch_and_bad_arguments():
    mpc = make_mpc("oscillating_masses")
    ps = mpc.structure
    out = mpc.S.solve_batch(np.zeros((0, ps.n_opt_x)), mpc._lb_opt_x.master, mpc._ub_opt_x.master,
                            mpc._nlp_cons_lb, mpc._nlp_cons_ub, np.zeros((0, ps.n_opt_p)))
    assert out["x"].shape == (0, ps.n_opt_x)
    with pytest.raises(ValueError):
        mpc.S(x0=np.zeros(3), lbx=mpc._lb_opt_x.master, ubx=mpc._ub_opt_x.master, lbg=mpc._nlp_cons_lb,
              ubg=mpc._nlp_cons_ub, p=mpc.opt_p_num.master)
    with pytest.raises(AssertionError):
        mpc.make_step(np.zeros(7))


def test_infeasible_problem_reports_failure_not_exception():
    # x0 far outside the +-2 K reactor band: no feasible robust trajectory.  The reference records
    # success=False and carries on (optimizer.py:770-778); so do we.
    mpc = make_mpc("industrial_poly", **{"nlpsol_opts": {"ipopt.max_iter": 60}})
    ex = CASES["industrial_poly"]
    x0 = ex.X0.copy()
    x0[3] += 25.0
    mpc.x0 = x0
    mpc.set_initial_guess()
    u0 = mpc.make_step(x0)
    assert u0.shape == (3, 1)
    assert mpc.solver_stats["success"] is False
    assert mpc.solver_stats["return_status"] in ("Maximum_Iterations_Exceeded", "Error_In_Step_Computation",
                                                 "Invalid_Number_Detected")


def test_industrial_poly_variant_b_tree_vs_oracle():
    # BASELINE.json configs[3], second reading: 3 parameter combinations, n_robust=2 (9 leaves, 174 edges)
    mpc = make_mpc("industrial_poly", n_robust=2, uncertainty="paired")
    nlp = pc.oracle_nlp("industrial_poly", n_robust=2, p_values=pc.PAIRED_P)
    assert (nlp.n_opt_x, nlp.n_g) == (mpc.structure.n_opt_x, mpc.structure.n_g) == (8100, 6970)
    ex = CASES["industrial_poly"]
    mpc.x0 = ex.X0
    mpc.set_initial_guess()
    u0 = mpc.make_step(ex.X0).ravel()
    assert mpc.solver_stats["success"]
    from oracle import ipm
    r = ipm.solve(nlp, nlp.initial_guess(ex.X0), nlp.opt_p(ex.X0, np.zeros(3)))
    assert r["stats"]["success"]
    assert pc.relerr(u0, nlp.u0_of(r["x"])) < pc.U_RTOL
    pc.check_kkt_with_oracle_functions(mpc, nlp, ex.X0)


def test_deeper_tree_27_leaves_kkt_properties():
    # n_robust=3: 27 leaves, 498 edges, 24 300 variables - checked through the oracle's NLP functions
    mpc = make_mpc("industrial_poly", n_robust=3, uncertainty="paired")
    nlp = pc.oracle_nlp("industrial_poly", n_robust=3, p_values=pc.PAIRED_P)
    ex = CASES["industrial_poly"]
    mpc.x0 = ex.X0
    mpc.set_initial_guess()
    mpc.make_step(ex.X0)
    assert mpc.solver_stats["success"]
    pc.check_kkt_with_oracle_functions(mpc, nlp, ex.X0)


def test_without_ipopts_one_sided_damping_the_cstr_golden_is_only_reached_to_1e_7(monkeypatch):
    """-DDOMPC_KAPPA_D=0 compiles the damping term kappa_d mu (x - l) of one-sided bounds out of the kernels (IPOPT section 3.7,
    default 1e-5 here as there): the CSTR golden, reproduced to 7e-14 with it (test_golden_replay), is then 3.5e-7 away -
    the soft-constraint and row slacks sit at their single bound and the optimum is sensitive to the barrier problem."""
    monkeypatch.setenv("DOMPC_DEFS", "DOMPC_KAPPA_D=0")
    mpc = make_mpc("CSTR")
    mpc.x0 = CASES["CSTR"].X0
    mpc.set_initial_guess()
    g = pc.golden("CSTR")
    u0 = mpc.make_step(g["mpc._x"][0]).ravel()
    assert 1e-8 < pc.relerr(u0, g["mpc._u"][0]) < 1e-6


def test_user_defined_rterm_written_as_the_default_gives_the_default_solution():
    pc.check_custom_rterm_equal_to_default(make_mpc)


@pytest.mark.parametrize("name", ["oscillating_masses", "CSTR"])
def test_user_defined_rterm_vs_oracle(name):
    pc.check_custom_rterm_vs_oracle(make_mpc, name)


@pytest.mark.parametrize("name,over,x0", pc.NL_COLLOC_CASES, ids=[c[0] for c in pc.NL_COLLOC_CASES])
def test_nl_cons_at_collocation_points(name, over, x0):
    pc.check_nl_cons_at_collocation_points(make_mpc, name, over, x0)


@pytest.mark.parametrize("over,x0", [c[1:] for c in pc.SINGLE_SLACK_CASES], ids=[c[0] for c in pc.SINGLE_SLACK_CASES])
def test_single_slack_shared_by_all_stages(over, x0):
    pc.check_single_slack(make_mpc, over, x0)


def test_single_slack_batch_equals_single_solves():
    pc.check_single_slack_batch(make_mpc)


@pytest.mark.parametrize("over,o_over,x0", [c[1:] for c in pc.OPEN_LOOP_CASES], ids=[c[0] for c in pc.OPEN_LOOP_CASES])
def test_open_loop_with_several_scenarios(over, o_over, x0):
    pc.check_open_loop(make_mpc, over, o_over, x0)


@pytest.mark.parametrize("name", ["CSTR", "batch_reactor", "industrial_poly"])
def test_dense_edge_path_reproduces_the_fast_path(name, monkeypatch):
    """-DDOMPC_FORCE_DENSE=1 sends a model without algebraic states through the dense edge path of the DAE models
    (csrc/dompc_dae.h: LDS-resident Gauss-Jordan with pivoting, dense condensing) - same iterates as the single-element
    fast path (register / matrix-core elimination), incl. the 9-scenario tree of industrial_poly"""
    ex = CASES[name]
    sol = []
    for defs in ("", "DOMPC_FORCE_DENSE=1"):
        monkeypatch.setenv("DOMPC_DEFS", defs)
        mpc = make_mpc(name)
        mpc.x0 = ex.X0
        mpc.set_initial_guess()
        mpc.make_step(ex.X0)
        assert mpc.solver_stats["success"]
        sol.append((mpc.solver_stats["iter_count"], mpc.opt_x_num.master.copy(), mpc.lam_g_num.copy()))
    assert sol[0][0] == sol[1][0]
    assert pc.relerr(sol[0][1], sol[1][1]) < 1e-11 and pc.relerr(sol[0][2], sol[1][2]) < 1e-9      # (measured 7e-14 / 1e-12)


def test_dense_elimination_with_row_loops_equals_the_register_variant(monkeypatch):
    """blocks of more than 48 unknowns keep the pivot steps of the dense path as loops over the rows (no example is that large):
    -DDOMPC_GJ_REGS_MAX=0 compiles that variant for the double inverted pendulum (36 unknowns, row interchanges at several
    pivots) - same iterations and solution as the in-register variant"""
    ex = CASES["dip"]
    sol = []
    for defs in ("", "DOMPC_GJ_REGS_MAX=0"):
        monkeypatch.setenv("DOMPC_DEFS", defs)
        mpc = make_mpc("dip", n_horizon=12)
        mpc.x0 = ex.X0
        mpc.set_initial_guess()
        mpc.make_step(ex.X0)
        assert mpc.solver_stats["success"]
        sol.append((mpc.solver_stats["iter_count"], mpc.opt_x_num.master.copy(), mpc.lam_g_num.copy()))
    assert sol[0][0] == sol[1][0] and sol[0][0] >= 5
    assert pc.relerr(sol[0][1], sol[1][1]) < 1e-11 and pc.relerr(sol[0][2], sol[1][2]) < 1e-9


def test_mid_size_tree_same_iterates_as_the_oracle():
    """27-leaf industrial_poly tree (n_robust = 3): oracle solve vs the kernels, same iterates"""
    pc.check_tree27_same_iterates_as_oracle(make_mpc)


def test_81_leaf_tree_equals_the_stored_oracle_solve():
    """81-leaf industrial_poly tree (n_robust = 4, 72 900 variables) against the stored oracle solve; the 243-leaf tree of BASELINE
    configs[4] runs in the GPU twin (test_gpu_parity.py)"""
    pc.check_big_tree_against_stored_oracle_solve(make_mpc, 81)


@pytest.mark.slow
def test_the_stored_81_leaf_oracle_solve_is_what_the_oracle_produces():
    """the fixture is not hand-made: tools/oracle_tree_fixture.py re-run (30 s)"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import oracle_tree_fixture as otf
    nlp, r, _ = otf.solve(4)
    o = pc.stored_oracle_tree(81)
    assert int(o["iter_count"]) == r["stats"]["iter_count"] and int(o["n_reg"]) == r["stats"]["n_reg"]
    assert np.array_equal(o["x"], r["x"]) and np.array_equal(o["lam_g"], r["lam_g"])


def test_control_interval_with_80_unknowns_same_iterates_as_the_oracle():
    pc.check_interval_with_more_than_64_unknowns(make_mpc)


def test_watchdog_ends_the_crawl_on_the_full_horizon_kite_problem():
    pc.check_watchdog_on_kite_full_horizon(make_mpc)


def test_watchdog_same_iterates_as_the_oracle_when_it_starts_after_every_shortened_step():
    """trigger = 1 on the cold industrial_poly solve: three watchdogs start (and succeed at their first step) in the product AND in the
    oracle - same 56 iterations, same final iterate: the two restatements of the procedure agree where their iterates are comparable"""
    from oracle import ipm
    name = "industrial_poly"
    mpc = make_mpc(name, nlpsol_opts={"ipopt.watchdog_shortened_iter_trigger": 1})
    nlp = pc.oracle_nlp(name)
    x0 = pc.golden(name)["mpc._x"][0]
    mpc.x0 = x0
    mpc.set_initial_guess()
    mpc.make_step(x0)
    st = mpc.solver_stats
    r = ipm.solve(nlp, nlp.initial_guess(x0), mpc.opt_p_num.master.copy(), opts=dict(watchdog_shortened_iter_trigger=1))
    assert st["n_watchdog"] == r["stats"]["n_watchdog"] == 3 and st["iter_count"] == r["stats"]["iter_count"] == 56
    assert pc.relerr(mpc.opt_x_num.master, r["x"]) < 1e-9


def test_open_loop_on_a_discrete_model_with_an_uncertain_parameter():
    pc.check_open_loop_discrete(hostemu.patched)


@pytest.mark.parametrize("name", ["CSTR", "industrial_poly", "oscillating_masses"])
def test_thread_per_entry_loops_of_the_wide_mode_give_the_same_bits(name, monkeypatch):
    """a single problem spread over several workgroups assembles gradients / dual residuals per VARIABLE and evaluates trial points per
    PIECE of an edge instead of per node / per edge (csrc: fine_items); -DDOMPC_FINE_ITEMS=1 runs those loops on the host emulation:
    same iterations, bitwise the same solution and multipliers (same arithmetic per entry, same order of every sum)"""
    ex = CASES[name]
    x0 = pc.golden(name)["mpc._x"][0]
    sol = []
    for defs in ("", "DOMPC_FINE_ITEMS=1"):
        monkeypatch.setenv("DOMPC_DEFS", defs)
        mpc = make_mpc(name)
        mpc.x0 = x0
        mpc.set_initial_guess()
        mpc.make_step(x0)
        assert mpc.solver_stats["success"]
        sol.append((mpc.solver_stats["iter_count"], mpc.solver_stats["n_trials"], mpc.opt_x_num.master.copy(), mpc.lam_g_num.copy(), mpc.lam_x_num.copy()))
    assert sol[0][:2] == sol[1][:2]
    assert np.array_equal(sol[0][2], sol[1][2]) and np.array_equal(sol[0][3], sol[1][3]) and np.array_equal(sol[0][4], sol[1][4])


def test_newton_direction_on_the_last_barrier_level_satisfies_the_state_rows():
    pc.check_newton_step_at_late_iterate(make_mpc)
