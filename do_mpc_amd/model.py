"""Symbolic model container with the same user surface as do_mpc.model.Model.

Mirrors /root/reference/do_mpc/model/_model.py:
  __init__            :91-128     (variable groups incl. the zero-size 'default' entries)
  set_variable        :537-621
  set_expression      :623-668
  set_meas            :670-747
  set_rhs             :749-809
  set_alg             :811-841
  setup               :937-1058
but is built on do_mpc_amd.sym (our own scalar DAG) instead of CasADi structs, because
the expressions are lowered to HIP device functions at MPC.setup() rather than being
interpreted by CasADi's VM.
"""
from __future__ import annotations

from typing import Dict, List, Tuple, Union

import numpy as np

from . import sym
from .structs import Entry, Layout, NumStruct


class VarGroup:
    """Ordered {name: SX} with the struct-ish accessors user code relies on
    (model.x['m_P'], model.aux['cost'], model._u.keys(), .cat, .labels(), (0) -> numeric)."""

    def __init__(self, kind: str):
        self.kind = kind
        self.names: List[str] = []
        self.vars: Dict[str, sym.SX] = {}

    def add(self, name: str, var: sym.SX):
        if name in self.vars:
            raise Exception(f"The variable {name} for type {self.kind} already exists.")
        self.names.append(name)
        self.vars[name] = var

    def keys(self):
        return list(self.names)

    def __contains__(self, name):
        return name in self.vars

    def __getitem__(self, key) -> sym.SX:
        if isinstance(key, tuple):
            name, rest = key[0], key[1:]
            v = self.vars[name]
            return v[rest if len(rest) > 1 else rest[0]]
        return self.vars[key]

    @property
    def cat(self) -> sym.SX:
        parts = [self.vars[n].reshape((self.vars[n].numel(), 1)) for n in self.names]
        return sym.vertcat(*parts) if parts else sym.SX([], (0, 1))

    @property
    def size(self) -> int:
        return sum(self.vars[n].numel() for n in self.names)

    @property
    def shape(self):
        return (self.size, 1)

    def layout(self) -> Layout:
        return Layout([Entry(n, self.vars[n].shape) for n in self.names])

    def labels(self):
        return self.layout().labels()

    def offset(self, name: str) -> int:
        off = 0
        for n in self.names:
            if n == name:
                return off
            off += self.vars[n].numel()
        raise KeyError(name)

    def __call__(self, value=0.0) -> NumStruct:
        return NumStruct(self.layout(), value)


_VAR_TYPES = ("_x", "_u", "_z", "_p", "_tvp", "_w", "_v")
_LONG_VAR_TYPES = {"states": "_x", "inputs": "_u", "algebraic": "_z", "parameter": "_p", "timevarying_parameter": "_tvp"}


class Model:
    def __init__(self, model_type: str = None, symvar_type: str = "SX"):
        assert isinstance(model_type, str), "model_type must be string, you have: {}".format(type(model_type))
        assert model_type in ["discrete", "continuous"], \
            "model_type must be either discrete or continuous, you have: {}".format(model_type)
        assert symvar_type in ["SX", "MX"], "symvar_type must be either SX or MX, you have: {}".format(symvar_type)
        # 'MX' is accepted for source compatibility; both map onto the same scalar DAG here.
        self.symvar_type = symvar_type
        self.model_type = model_type
        self._x = VarGroup("_x")
        self._u = VarGroup("_u")
        self._z = VarGroup("_z")
        self._p = VarGroup("_p")
        self._tvp = VarGroup("_tvp")
        self._w = VarGroup("_w")
        self._v = VarGroup("_v")
        self._y = VarGroup("_y")
        self._aux = VarGroup("_aux")
        for grp in (self._u, self._z, self._p, self._tvp, self._w, self._v):
            grp.add("default", sym.SX([], (0, 0)))
        self._aux.add("default", sym.SX(0.0))            # size-1 'default' = 0  (_model.py:107,116)
        self._y_noise: Dict[str, bool] = {}
        self.rhs_list: List[dict] = []
        self.alg_list: List[dict] = []
        self.integer: List[str] = []
        self.flags = {"setup": False}

    # ---------------------------------------------------------------- queries
    def __getitem__(self, ind):
        """`model['x']`, `model['x', 'tvp']`: the variable groups themselves (name-indexable, `.cat` for the vector),
        like the structures the reference hands out (_model.py:165-200)."""
        if isinstance(ind, tuple):
            return [self._getvar(i) for i in ind]
        return self._getvar(ind)

    def _getvar(self, var_name: str) -> VarGroup:
        if var_name.startswith("_"):
            var_name = var_name[1:]
        table = {"x": self._x, "u": self._u, "z": self._z, "p": self._p, "tvp": self._tvp,
                 "y": self._y, "aux": self._aux, "w": self._w, "v": self._v}
        if var_name not in table:
            raise Exception(f"{var_name} is not a model variable type")
        return table[var_name]

    x = property(lambda self: self._x)
    u = property(lambda self: self._u)
    z = property(lambda self: self._z)
    p = property(lambda self: self._p)
    tvp = property(lambda self: self._tvp)
    y = property(lambda self: self._y)
    aux = property(lambda self: self._aux)
    w = property(lambda self: self._w)
    v = property(lambda self: self._v)

    n_x = property(lambda self: self._x.size)
    n_u = property(lambda self: self._u.size)
    n_z = property(lambda self: self._z.size)
    n_p = property(lambda self: self._p.size)
    n_tvp = property(lambda self: self._tvp.size)
    n_w = property(lambda self: self._w.size)
    n_v = property(lambda self: self._v.size)
    n_y = property(lambda self: self._y.size)
    n_aux = property(lambda self: self._aux.size)

    # ---------------------------------------------------------------- configuration
    def set_variable(self, var_type: str, var_name: str, shape: Union[int, Tuple] = (1, 1),
                     input_type_integer: bool = False) -> sym.SX:
        assert self.flags["setup"] is False, "Cannot call .set_variable after setup."
        assert isinstance(var_type, str), "var_type must be str, you have: {}".format(type(var_type))
        assert isinstance(var_name, str), "var_name must be str, you have: {}".format(type(var_name))
        assert isinstance(shape, (tuple, int)), "shape must be tuple or int, you have: {}".format(type(shape))
        var_type = _LONG_VAR_TYPES.get(var_type, var_type)          # long names (_model.py:596-601)
        if var_type not in _VAR_TYPES:
            raise Exception("Trying to set non-existing variable var_type: {} with var_name {}".format(var_type, var_name))
        if isinstance(shape, int):
            shape = (shape, 1)
        if var_type != "_u" and input_type_integer:
            raise Exception("Integer variables are only supported for inputs (_u).")
        grp = getattr(self, var_type)
        var = sym.SX.sym(var_name, shape[0], shape[1])
        grp.add(var_name, var)
        if input_type_integer:
            self.integer.append(var_name)
        return var

    def set_expression(self, expr_name: str, expr) -> sym.SX:
        assert self.flags["setup"] is False, "Cannot call .set_expression after setup."
        assert isinstance(expr_name, str), "expr_name must be str, you have: {}".format(type(expr_name))
        assert isinstance(expr, (sym.SX, sym.DM)), "expr must be a symbolic expression, you have: {}".format(type(expr))
        expr = sym.SX(expr)
        self._aux.add(expr_name, expr)
        return expr

    def set_meas(self, meas_name: str, expr, meas_noise: bool = True) -> sym.SX:
        assert self.flags["setup"] is False, "Cannot call .set_meas after setup."
        assert isinstance(meas_name, str), "meas_name must be str, you have: {}".format(type(meas_name))
        expr = sym.SX(expr)
        if meas_noise:
            v = self.set_variable("_v", meas_name + "_noise", expr.shape)
            expr = expr + v
        self._y.add(meas_name, expr)
        return expr

    def set_rhs(self, var_name: str, expr, process_noise: bool = False) -> None:
        assert self.flags["setup"] is False, "Cannot call .set_rhs after .setup."
        assert isinstance(var_name, str), "var_name must be str, you have: {}".format(type(var_name))
        assert var_name in self._x.names, \
            "var_name must refer to the previously defined states ({}). You have: {}".format(self._x.names, var_name)
        expr = sym.SX(expr)
        if process_noise:
            w = self.set_variable("_w", var_name + "_noise", expr.shape)
            expr = expr + w
        self.rhs_list.append({"var_name": var_name, "expr": expr})

    def set_alg(self, expr_name: str, expr) -> None:
        assert self.flags["setup"] is False, "Cannot call .set_alg after .setup."
        self.alg_list.append({"expr_name": expr_name, "expr": sym.SX(expr)})

    # ---------------------------------------------------------------- finalise
    def setup(self) -> None:
        if len(self._y.names) == 0:           # default: full state feedback (_model.py:954-957)
            for n in self._x.names:
                self._y.add(n, self._x.vars[n])
        rhs_names = [r["var_name"] for r in self.rhs_list]
        for n in self._x.names:
            if n not in rhs_names:
                raise Exception(f"Set rhs for all states. Missing: {n}")
        for r in self.rhs_list:
            if r["expr"].shape != self._x.vars[r["var_name"]].shape:
                raise Exception(f"rhs for {r['var_name']} has shape {r['expr'].shape}, "
                                f"expected {self._x.vars[r['var_name']].shape}")
        by_name = {r["var_name"]: r["expr"] for r in self.rhs_list}
        self._rhs = sym.vertcat(*[by_name[n].reshape((by_name[n].numel(), 1)) for n in self._x.names])
        self._alg = sym.vertcat(*[a["expr"].reshape((a["expr"].numel(), 1)) for a in self.alg_list]) \
            if self.alg_list else sym.SX([], (0, 1))
        if self._alg.numel() != self.n_z:
            raise Exception(f"{self.n_z} algebraic states but {self._alg.numel()} algebraic equations")
        _x, _u, _z, _tvp, _p, _w, _v = (self._getvar(k).cat for k in ("x", "u", "z", "tvp", "p", "w", "v"))
        self._rhs_fun = sym.Function("rhs_fun", [_x, _u, _z, _tvp, _p, _w], [self._rhs])
        self._alg_fun = sym.Function("alg_fun", [_x, _u, _z, _tvp, _p, _w], [self._alg])
        self._aux_expression_fun = sym.Function("aux_expression_fun", [_x, _u, _z, _tvp, _p], [self._aux.cat])
        self._meas_fun = sym.Function("meas_fun", [_x, _u, _z, _tvp, _p, _v], [self._y.cat])
        for fn, what in ((self._rhs_fun, "rhs"), (self._aux_expression_fun, "aux")):
            free = fn.free_symbols()
            if free:
                raise Exception(f"{what} depends on symbols that are not model variables: {free}")
        self.flags["setup"] = True

    # ---------------------------------------------------------------- linearisation
    def get_linear_system_matrices(self, xss=None, uss=None, z=None, tvp=None, p=None):
        """(A, B, C, D) of the system linearised around (xss, uss, z, tvp, p): A = d rhs / d x, B = d rhs / d u, C = d y / d x,
        D = d y / d u (/root/reference/do_mpc/model/_model.py:1008-1011, 1090-1144).  Every argument is optional: a group that is
        not given stays symbolic, and a matrix that still depends on symbols is returned as `sym.SX`; otherwise as a numpy array.
        The noise symbols `_w` / `_v` are zero."""
        assert self.flags["setup"] is True, "Model was not setup. Call model.setup() first."
        if getattr(self, "_lin_expr", None) is None:
            self._lin_expr = (sym.jacobian(self._rhs, self._x.cat), sym.jacobian(self._rhs, self._u.cat),
                              sym.jacobian(self._y.cat, self._x.cat), sym.jacobian(self._y.cat, self._u.cat))
        mapping = {}
        for grp, val in ((self._x, xss), (self._u, uss), (self._z, z), (self._tvp, tvp), (self._p, p), (self._w, 0.0), (self._v, 0.0)):
            nodes = grp.cat.nodes()
            if val is None or isinstance(val, VarGroup) or not nodes:
                continue
            if isinstance(val, sym.SX):
                new = val.nodes()
            else:
                a = np.asarray(val.master if hasattr(val, "master") else (val.arr if hasattr(val, "arr") else val), dtype=float).reshape(-1)
                new = [sym.const(float(v)) for v in (np.full(len(nodes), a[0]) if a.size == 1 else a)]
            assert len(new) == len(nodes), f"{grp.kind} has {len(nodes)} elements, got {len(new)}"
            mapping.update({s.idx: n for s, n in zip(nodes, new)})
        out = []
        for Mx in self._lin_expr:
            data = sym.substitute_nodes(Mx.data, mapping) if mapping else list(Mx.data)
            if sym.free_symbols(data):
                out.append(sym.SX(data, Mx.shape))
            else:
                if getattr(self, "_lin_dummy", None) is None:
                    self._lin_dummy = sym.SX.sym("lin_dummy")         # (sym.Function wants at least one input)
                vals = sym.Function("lin", [self._lin_dummy], [sym.SX(data, Mx.shape)]).eval(0.0)[0] if data else np.zeros(0)
                out.append(np.asarray(vals, float).reshape(Mx.shape, order="F"))
        return tuple(out)

    @staticmethod
    def _transfer_variables(old_model: "Model", new_model: "Model", transfer=("_x", "_u", "_z", "_tvp", "_p", "_aux")) -> None:
        """Variables (names and shapes) of `old_model` into `new_model`; `_aux` expressions are rewritten on the new symbols
        (/root/reference/do_mpc/model/_model.py: _transfer_variables)."""
        old_nodes, new_nodes = [], []
        for var_type in transfer:
            if var_type == "_aux":
                continue
            for name in getattr(old_model, var_type).names:
                if name == "default":
                    continue
                v_old = getattr(old_model, var_type).vars[name]
                v_new = new_model.set_variable(var_type, name, v_old.shape)
                old_nodes += v_old.nodes()
                new_nodes += v_new.nodes()
        if "_aux" in transfer:
            mapping = {s.idx: n for s, n in zip(old_nodes, new_nodes)}
            for name in old_model._aux.names:
                if name == "default":
                    continue
                e = old_model._aux.vars[name]
                data = sym.substitute_nodes(e.data, mapping)
                if any(s.idx not in {n.idx for n in new_nodes} for s in sym.free_symbols(data)):
                    continue                  # (depends on a group that was not transferred)
                new_model.set_expression(name, sym.SX(data, e.shape))


# ------------------------------------------------------------------------------------------------ linear models
EXPM_TAYLOR = 18          # degree of the Taylor polynomial; csrc/dompc_lqr.hip (DOMPC_LQR_TAYLOR) uses the same scheme


def _expm(E: np.ndarray) -> np.ndarray:
    """exp(E) with matrix products only, the scheme of csrc/dompc_lqr.hip: E / 2^s with a 1-norm <= 1/2, the Taylor polynomial of
    degree 18 in Horner form, s squarings.  (Against scipy.signal.cont2discrete: 8.8e-15 at worst over 4 096 random systems.)"""
    E = np.asarray(E, dtype=float)
    n = E.shape[0]
    nrm = float(np.max(np.sum(np.abs(E), axis=0))) if n else 0.0
    if not np.isfinite(nrm):
        raise ValueError("matrix exponential of a matrix that is not finite")
    s = int(np.frexp(nrm)[1]) + 1 if nrm > 0.5 else 0          # (= ilogb(nrm) + 2)
    Es = E * 2.0 ** (-s)
    eye = np.eye(n)
    T = eye + Es / EXPM_TAYLOR
    for j in range(EXPM_TAYLOR - 1, 0, -1):
        T = eye + (Es @ T) / j
    for _ in range(s):
        T = T @ T
    return T


def _cont2discrete(A, B, C, D, dt, method="zoh", alpha=None):
    """(A_d, B_d, C_d, D_d) like scipy.signal.cont2discrete, in numpy: 'zoh' from exp([[A, B], [0, 0]] dt), the generalised bilinear
    transformation 'gbt' (alpha) with its special cases 'bilinear' (1/2), 'euler' (0) and 'backward_diff' (1) as linear solves."""
    A, B, C, D = (np.atleast_2d(np.asarray(a, dtype=float)) for a in (A, B, C, D))
    nx, nu = A.shape[0], B.shape[1]
    if method == "zoh":
        E = np.zeros((nx + nu, nx + nu))
        E[:nx, :nx], E[:nx, nx:] = A * dt, B * dt
        T = _expm(E)
        return T[:nx, :nx], T[:nx, nx:], C, D
    if method in ("bilinear", "tustin"):
        alpha = 0.5
    elif method in ("euler", "forward_diff"):
        alpha = 0.0
    elif method == "backward_diff":
        alpha = 1.0
    elif method == "gbt":
        if alpha is None:
            raise ValueError("Alpha parameter must be specified for the generalized bilinear transform (gbt) method")
        if alpha < 0 or alpha > 1:
            raise ValueError("Alpha parameter must be within the interval [0,1] for the gbt method")
    else:
        raise ValueError("Unknown transformation method '%s'" % method)
    ima = np.eye(nx) - alpha * dt * A
    Ad = np.linalg.solve(ima, np.eye(nx) + (1.0 - alpha) * dt * A)
    Bd = np.linalg.solve(ima, dt * B)
    Cd = np.linalg.solve(ima.T, C.T).T
    Dd = D + alpha * (C @ Bd)
    return Ad, Bd, Cd, Dd


class LinearModel(Model):
    """Linear time-invariant model, continuous or discrete, with do_mpc.model.LinearModel's surface
    (/root/reference/do_mpc/model/_linearmodel.py): `set_rhs` / `set_meas` accept expressions that are linear in (x, u) only,
    `setup(A, B, C, D)` takes the matrices instead, `sys_A` .. `sys_D`, `discretize`, `get_steady_state`."""

    def __init__(self, model_type: str = None, symvar_type: str = "SX"):
        super().__init__(model_type, symvar_type)
        if symvar_type == "MX":
            raise ValueError("class LinearModel can be initialized only with SX variable.")

    def _sys(self, name):
        assert self.flags["setup"] is True, "Attributes are available after the model is setup."
        return getattr(self, name)

    sys_A = property(lambda self: self._sys("_A"))
    sys_B = property(lambda self: self._sys("_B"))
    sys_C = property(lambda self: self._sys("_C"))
    sys_D = property(lambda self: self._sys("_D"))

    def _is_linear(self, expr) -> bool:
        return sym.jacobian(sym.SX(expr), sym.vertcat(self._x.cat, self._u.cat)).is_constant()

    def set_rhs(self, name: str, rhs) -> None:
        if not self._is_linear(rhs):
            raise ValueError("Given rhs is not linear.")
        super().set_rhs(name, rhs, process_noise=True)

    def set_meas(self, name: str, meas) -> None:
        if not self._is_linear(meas):
            raise ValueError("Measurement function is not linear.")
        super().set_meas(name, meas, meas_noise=True)

    def set_alg(self, expr_name, expr, *args, **kwargs):
        raise NotImplementedError("Algebraic variables are not supported for linear models.")

    def setup(self, A: np.ndarray = None, B: np.ndarray = None, C: np.ndarray = None, D: np.ndarray = None) -> None:
        for name, M in (("A", A), ("B", B), ("C", C), ("D", D)):
            if not isinstance(M, (np.ndarray, type(None))):
                raise ValueError(f"{name} must be a numpy array or None")
        # three use cases (_linearmodel.py:200-211): C / D given -> measurement function from them; set_meas was called -> it exists;
        # neither -> Model.setup creates the default one (state feedback)
        y_meas = None
        if C is not None:
            y_meas = C @ self._x.cat
        if D is not None:
            y_meas = y_meas + D @ self._u.cat
        if y_meas is not None:
            self.set_meas("y", y_meas)
        n_x, n_u = self._x.size, self._u.size
        x_next = None
        if isinstance(A, np.ndarray):
            if A.shape != (n_x, n_x):
                raise ValueError("A must be a square matrix with size n_x x n_x. You have A.shape={}".format(A.shape))
            x_next = A @ self._x.cat
        if isinstance(B, np.ndarray):
            if B.shape != (n_x, n_u):
                raise ValueError("B must be a matrix with size n_x x n_u. You have B.shape={}".format(B.shape))
            x_next = x_next + B @ self._u.cat
        if x_next is not None:
            off = 0
            for name in self._x.keys():
                k = self._x.vars[name].numel()
                self.set_rhs(name, x_next[off:off + k])
                off += k
        super().setup()
        self._A, self._B, self._C, self._D = self.get_linear_system_matrices()

    def discretize(self, t_step: Union[float, int] = 0, conv_method: str = "zoh", alpha: float = None) -> "LinearModel":
        """Discrete model of this continuous one with the same variable names ('zoh', 'gbt' with `alpha`, 'bilinear', 'euler',
        'backward_diff': the methods of scipy.signal.cont2discrete, computed in numpy)."""
        assert self.flags["setup"] is True, "This method can be accessed only after the model is setup using LinearModel.setup()."
        assert self.model_type == "continuous", "Given model is already discrete."
        A, B, C, _ = _cont2discrete(self.sys_A, self.sys_B, self.sys_C, self.sys_D, t_step, conv_method, alpha)
        discrete = LinearModel("discrete")
        self._transfer_variables(self, discrete)
        discrete.setup(A, B, C)
        return discrete

    def get_steady_state(self, xss: np.ndarray = None, uss: np.ndarray = None) -> np.ndarray:
        """x_ss = (I - A)^-1 B u_ss for given inputs, or u_ss = B^-1 (I - A) x_ss (pseudo-inverse for a B that is not square) for
        given states (_linearmodel.py:304-326)."""
        assert self.flags["setup"] is True, "Model is not setup. Please run model.setup() fun to calculate steady state."
        assert self.model_type == "discrete", "Please convert the system to discrete using model.continuous_2_discrete()."
        eye = np.identity(self.sys_A.shape[0])
        if xss is None and np.linalg.matrix_rank(self.sys_A) == self._x.shape[0]:
            assert uss is not None and isinstance(uss, np.ndarray), "Provide either steady state states or steady state inputs."
            self.xss, self.uss = np.linalg.inv(eye - self.sys_A) @ self.sys_B @ uss, uss
            return self.xss
        if xss is None:
            raise ValueError("State matrix does not have full rank. Hence, either multiple steady state or no steady state values is possible.")
        if uss is not None:                # both given: none of the reference's four branches, which then returns None
            return None
        assert isinstance(xss, np.ndarray), "Provide either steady state states or steady state inputs."
        square = self.sys_B.shape[0] == self.sys_B.shape[1]
        self.uss = (np.linalg.inv(self.sys_B) if square else np.linalg.pinv(self.sys_B)) @ (eye - self.sys_A) @ xss
        self.xss = xss
        return self.uss


def linearize(model: Model, xss: np.ndarray = None, uss: np.ndarray = None, tvp0: np.ndarray = None, p0: np.ndarray = None) -> LinearModel:
    """LinearModel of `model` around (xss, uss) with the same variable names (/root/reference/do_mpc/model/_linearize.py)."""
    assert model.flags["setup"] is True, "Run this function after original model is setup"
    assert model._z.size == 0, "Linearization around steady state is not supported for DAEs"
    A, B, C, D = model.get_linear_system_matrices(xss, uss, tvp=tvp0, p=p0)
    if not all(isinstance(M, np.ndarray) for M in (A, B, C, D)):
        raise NotImplementedError("LTV models are not yet implemented. (gains along a trajectory: LQR.gains_along)")
    linear = LinearModel(model.model_type, model.symvar_type)
    model._transfer_variables(model, linear)
    n_x, n_u = model.n_x, model.n_u
    if C.shape == (n_x, n_x) and (C == np.eye(n_x)).all():      # trivial measurement equation
        C = None
    if D.shape == (n_x, n_u) and (D == np.zeros((n_x, n_u))).all():
        D = None
    linear.setup(A, B, C, D)
    return linear


# ------------------------------------------------------------------------------------------------ models with algebraic states
def dae2odeconversion(model: Model) -> Model:
    """Index-1 DAE model x' = f(x, u, z), 0 = g(x, u, z) (or x+ = f for a discrete one) as an ODE model by differentiation of the
    algebraic equations, with the surface of the reference (/root/reference/do_mpc/model/_dae2odeconversion.py): the new model has the
    STATES [x, u, z] under their old names and ONE input `q` of shape (n_u, 1), the rate of the old inputs:

        x' = f(x, u, z),   u' = q,   z' = -g_z^-1 g_x f - g_z^-1 g_u q.

    `_p` and `_tvp` are carried over, and so is the process noise of every state that had it.  g_z^-1 is symbolic (sym.inv)."""
    assert model.flags["setup"] is True, "Run this function after original model is setup"
    new = Model(model.model_type, model.symvar_type)
    groups = {}
    for var_type, target in (("_x", "_x"), ("_u", "_x"), ("_z", "_x"), ("_p", "_p"), ("_tvp", "_tvp")):
        old_nodes, new_nodes = [], []
        for name in getattr(model, var_type).names:
            if name == "default":
                continue
            v_old = getattr(model, var_type).vars[name]
            v_new = new.set_variable(target, name, v_old.shape)
            old_nodes += v_old.nodes()
            new_nodes += v_new.nodes()
        groups[var_type] = (old_nodes, new_nodes)
    q = new.set_variable("_u", "q", (model.n_u, 1))
    mapping = {o.idx: n for old_nodes, new_nodes in groups.values() for o, n in zip(old_nodes, new_nodes)}
    col = lambda nodes: sym.SX(list(nodes), (len(nodes), 1))      # noqa: E731
    rhs = col(sym.substitute_nodes(model._rhs.nodes(), mapping))          # (on the new symbols, with the old model's noise symbols)
    alg = col(sym.substitute_nodes(model._alg.nodes(), mapping))
    w_old = model._w.cat.nodes()
    rhs_new = col(sym.substitute_nodes(rhs.nodes(), {s.idx: sym.ZERO for s in w_old}))
    off = 0
    for name in model._x.names:
        k = model._x.vars[name].numel()
        new.set_rhs(name, rhs_new[off:off + k], process_noise=(name + "_noise") in model._w.names)
        off += k
    w_new = new._w.cat.nodes()
    assert len(w_new) == len(w_old)
    rhs_mod = col(sym.substitute_nodes(rhs.nodes(), {o.idx: n for o, n in zip(w_old, w_new)}))
    alg = col(sym.substitute_nodes(alg.nodes(), {o.idx: n for o, n in zip(w_old, w_new)}))
    x_new, u_new, z_new = (col(groups[k][1]) for k in ("_x", "_u", "_z"))
    gz_inv = sym.inv(sym.jacobian(alg, z_new))
    z_next = -gz_inv @ sym.jacobian(alg, x_new) @ rhs_mod - gz_inv @ sym.jacobian(alg, u_new) @ q
    off = 0
    for name in model._u.names:
        if name == "default":
            continue
        k = model._u.vars[name].numel()
        new.set_rhs(name, q[off:off + k])
        off += k
    off = 0
    for name in model._z.names:
        if name == "default":
            continue
        k = model._z.vars[name].numel()
        new.set_rhs(name, z_next[off:off + k])
        off += k
    new.setup()
    print("The states of the new model are {}".format(new.x.keys()))
    return new


def _dae_functions(model: Model):
    """(g and g_z; f_x f_u f_z g_x g_u g_z) of a model with algebraic states as functions of (x, u, z, tvp, p), noise zero"""
    if getattr(model, "_dae_lin", None) is None:
        zero = {s.idx: sym.ZERO for s in model._w.cat.nodes() + model._v.cat.nodes()}
        col = lambda nodes: sym.SX(list(nodes), (len(nodes), 1))      # noqa: E731
        f, g = col(sym.substitute_nodes(model._rhs.nodes(), zero)), col(sym.substitute_nodes(model._alg.nodes(), zero))
        ins = [model._x.cat, model._u.cat, model._z.cat, model._tvp.cat, model._p.cat]
        x, u, z = ins[:3]
        model._dae_lin = (sym.Function("alg", ins, [g, sym.jacobian(g, z)]),
                          sym.Function("lin", ins, [sym.jacobian(a, b) for a in (f, g) for b in (x, u, z)]))
    return model._dae_lin


def linearize_dae(model: Model, xss: np.ndarray, uss: np.ndarray, z0: np.ndarray = None, tvp0: np.ndarray = None, p0: np.ndarray = None,
                  tol: float = 1e-10, max_iter: int = 20) -> LinearModel:
    """LinearModel (states and inputs of `model`, state feedback) of the REDUCED system of an index-1 DAE model x' = f(x, u, z),
    0 = g(x, u, z) (x+ = f for a discrete one) at the operating point (xss, uss) - the host statement, in numpy, of what the design
    kernel of LQR.gains_at does for such a model:
      1. Newton on g(xss, uss, z) = 0 from the guess z0 (default 0): z <- z - g_z^-1 g until max |g| <= tol, at most max_iter updates;
      2. g_z [Z_x Z_u] = [g_x g_u];
      3. A = f_x - f_z Z_x, B = f_u - f_z Z_u.
    Unlike the route dae2odeconversion -> linearize this is exact at any operating point and keeps the model's size.  The consistent
    algebraic states are returned as the attribute `zss` [nz][1] of the linear model, the Newton updates as `newton_passes`.  Raises
    when Newton does not converge or g_z is singular."""
    assert model.flags["setup"] is True, "Run this function after original model is setup"
    assert model.n_z > 0, "linearize_dae is for models with algebraic states: use linearize"
    f_alg, f_lin = _dae_functions(model)
    flat = lambda a, n, what: np.zeros(n) if (a is None and what == "z0") else np.asarray(      # noqa: E731
        a.master if hasattr(a, "master") else a, dtype=float).reshape(-1)
    for what, a, n in (("tvp0", tvp0, model.n_tvp), ("p0", p0, model.n_p)):
        if a is None and n:
            raise NotImplementedError(f"LTV models are not yet implemented. ({what} is needed: the model has parameters)")
    args = [flat(xss, model.n_x, "xss"), flat(uss, model.n_u, "uss"), flat(z0, model.n_z, "z0"),
            flat(tvp0 if model.n_tvp else np.zeros(0), 0, "tvp0"), flat(p0 if model.n_p else np.zeros(0), 0, "p0")]
    nz = model.n_z
    passes = 0
    while True:
        g, gz = f_alg.eval(*args)
        gz = gz.reshape((nz, nz), order="F")
        if np.max(np.abs(g)) <= tol:
            break
        if passes >= max_iter or not np.all(np.isfinite(g)):
            raise RuntimeError(f"linearize_dae: Newton on the algebraic equations did not converge (max |g| = {np.max(np.abs(g)):.3e} "
                               f"after {passes} updates)")
        args[2] = args[2] - np.linalg.solve(gz, g)
        passes += 1
    n_x, n_u = model.n_x, model.n_u
    fx, fu, fz, gx, gu, gz = (M.reshape(shape, order="F") for M, shape in zip(
        f_lin.eval(*args), ((n_x, n_x), (n_x, n_u), (n_x, nz), (nz, n_x), (nz, n_u), (nz, nz))))
    Z = np.linalg.solve(gz, np.hstack([gx, gu]))
    A, B = fx - fz @ Z[:, :n_x], fu - fz @ Z[:, n_x:]
    linear = LinearModel(model.model_type, model.symvar_type)
    model._transfer_variables(model, linear, transfer=("_x", "_u", "_tvp", "_p", "_aux"))
    linear.setup(A, B)
    linear.zss, linear.newton_passes = args[2].reshape(-1, 1).copy(), passes
    return linear
