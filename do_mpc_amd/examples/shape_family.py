"""A synthetic family of small NMPC problems whose only purpose is their SHAPE: state, input, slack and nl_cons counts that no
shipped example has, chosen to select the index cases of the matrix-core Riccati recursion (csrc/dompc_riccati16.h) and the
sizes one past its limits (tests/riccati_shape_common.py).

NOT AN EXAMPLE OF THE REFERENCE: nothing like it exists there, and no stored reference run can exist.  The tests that use it
are oracle checks (oracle/models.py: case_shape_family states the same problems in sympy), not reproductions.

The model: a stable, mildly nonlinear ring of `nx` states driven by `nu` inputs,
    x_i' = -a_i x_i + b_i x_(i+1) + 0.1 p x_i x_(i-1) + sum_j B_ij u_j        (indices mod nx),
polynomial only; a, b, B are fixed numbers drawn from default_rng(nx * 100 + nu); one uncertain parameter p in {1, 1.2, 0.8}.
The controller: Radau collocation of degree 2, one finite element, horizon 4, robust horizon 1 (a root with three children, three
chains below), quadratic tracking of SET_POINT, a number per input as rterm, boxes on every state and input and the rows
    x_q^2 + x_(q+1) + 0.5 u_(q mod nu) <= ub_q ,    q = 0 .. n_soft + n_hard - 1 ,
the first n_soft of them soft with a slack of their own (penalty 10), the others hard.
"""
from types import SimpleNamespace

import numpy as np

from .. import MPC, Model

P_VALUES = (1.0, 1.2, 0.8)
X_BOX, U_BOX = 2.0, 1.0
SET_POINT, R_TERM, PENALTY = 1.2, 0.02, 10.0
T_STEP, N_HORIZON, N_ROBUST = 0.2, 4, 1
# ub_q = (value of row q at X0 with u = 0) + offset.  The set-point lies above X0 and every entry of B is positive: every input wants
# its upper bound.  With 0.51 (soft) / 0.53 (hard) the row leaves its input free to reach that bound at the first stage (0.5 u <= offset:
# an input bound is active) and ends active at the later stages, where the states have risen.  In two members one input is shared by a
# soft and a hard row: there the row that is to end active as well must be the tighter of the two.
UB_SOFT, UB_HARD = 0.51, 0.53
UB_OFFSET = {(10, 2, 2, 1): (0.8, 0.51, 0.51), (4, 2, 1, 4): (0.4, 0.53, 0.53, 0.53, 0.53)}      # (nx, nu, n_soft, n_hard) -> offset per row


def numbers(nx, nu):
    """a (nx), b (nx), B (nx, nu): the family's fixed coefficients; every entry of B is at least 0.3 (every input acts on every state)"""
    rng = np.random.default_rng(nx * 100 + nu)
    a = rng.uniform(0.5, 1.5, nx)
    b = rng.uniform(-0.5, 0.5, nx)
    B = rng.uniform(0.3, 1.0, (nx, nu))
    return a, b, B


def x0_of(nx):
    """the family's initial state: distinct entries (an index slip moves the solution)"""
    return 0.5 + 0.3 * np.cos(np.arange(nx))


def row_ub(nx, nu, n_soft, n_hard, q):
    """ub_q: the value of row q at the initial state with zero input plus the row's offset (UB_OFFSET, else UB_SOFT / UB_HARD)"""
    x0 = x0_of(nx)
    off = UB_OFFSET.get((nx, nu, n_soft, n_hard), (UB_SOFT,) * n_soft + (UB_HARD,) * n_hard)
    return float(x0[q % nx] ** 2 + x0[(q + 1) % nx] + off[q])


def build_model(nx=4, nu=2, symvar_type="SX"):
    a, b, B = numbers(nx, nu)
    mdl = Model("continuous", symvar_type)
    x = [mdl.set_variable(var_type="_x", var_name="x%d" % i) for i in range(nx)]
    u = [mdl.set_variable(var_type="_u", var_name="u%d" % j) for j in range(nu)]
    p = mdl.set_variable(var_type="_p", var_name="p")
    for i in range(nx):
        rhs = -float(a[i]) * x[i] + float(b[i]) * x[(i + 1) % nx] + 0.1 * p * x[i] * x[(i - 1) % nx]
        for j in range(nu):
            rhs = rhs + float(B[i, j]) * u[j]
        mdl.set_rhs("x%d" % i, rhs)
    mdl.setup()
    return mdl


def build_mpc(model, n_soft=0, n_hard=0, silence_solver=True, **overrides):
    nx, nu = model.n_x, model.n_u
    mpc = MPC(model)
    st = mpc.settings
    st.n_horizon, st.n_robust, st.open_loop = N_HORIZON, N_ROBUST, 0
    st.t_step = T_STEP
    st.state_discretization, st.collocation_type = "collocation", "radau"
    st.collocation_deg, st.collocation_ni = 2, 1
    st.store_full_solution = True
    for k, v in overrides.items():
        setattr(st, k, v)
    if silence_solver:
        st.supress_ipopt_output()
    track = (model.x["x0"] - SET_POINT) ** 2
    for i in range(1, nx):
        track = track + (model.x["x%d" % i] - SET_POINT) ** 2
    mpc.set_objective(mterm=track, lterm=track)
    mpc.set_rterm(**{"u%d" % j: R_TERM for j in range(nu)})
    for i in range(nx):
        mpc.bounds["lower", "_x", "x%d" % i] = -X_BOX
        mpc.bounds["upper", "_x", "x%d" % i] = X_BOX
    for j in range(nu):
        mpc.bounds["lower", "_u", "u%d" % j] = -U_BOX
        mpc.bounds["upper", "_u", "u%d" % j] = U_BOX
    for q in range(n_soft + n_hard):
        row = model.x["x%d" % (q % nx)] ** 2 + model.x["x%d" % ((q + 1) % nx)] + 0.5 * model.u["u%d" % (q % nu)]
        if q < n_soft:
            mpc.set_nl_cons("row%d" % q, row, ub=row_ub(nx, nu, n_soft, n_hard, q), soft_constraint=True, penalty_term_cons=PENALTY)
        else:
            mpc.set_nl_cons("row%d" % q, row, ub=row_ub(nx, nu, n_soft, n_hard, q), soft_constraint=False)
    mpc.set_uncertainty_values(p=np.array(P_VALUES))
    mpc.setup()
    return mpc


# id -> (nx, nu, n_soft, n_hard): the shapes of tests/riccati_shape_common.py
MEMBERS = {"s1": (1, 1, 0, 0), "s2": (3, 1, 0, 0), "s3": (5, 2, 1, 1), "s4": (6, 2, 2, 2), "s5": (8, 4, 0, 0),
           "s6": (10, 2, 2, 1), "s7": (14, 1, 0, 0), "s8": (9, 4, 0, 0), "s9": (4, 2, 1, 4)}


def member(mid):
    """member `mid` with the surface of an example module: build_model(), build_mpc(model, **overrides), X0"""
    nx, nu, n_soft, n_hard = MEMBERS[mid]
    return SimpleNamespace(build_model=lambda symvar_type="SX": build_model(nx, nu, symvar_type),
                           build_mpc=lambda model, **kw: build_mpc(model, n_soft, n_hard, **kw),
                           X0=x0_of(nx), shape=MEMBERS[mid])


X0 = x0_of(4)
