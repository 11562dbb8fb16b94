"""Extended Kalman filter with do_mpc.estimator.EKF's user surface, batched on the GPU.

Reference surface mirrored here (/root/reference/do_mpc/estimator/_ekf.py): `EKF(model)`, `settings.t_step`, `P0` (validated like
there, default identity), `get_/set_p_fun`, `get_/set_tvp_fun`, `setup()`, `x0`, `set_initial_guess()`,
`make_step(y_next, u_next, Q_k, R_k) -> x0`, `data` (`_x` = the posterior, `_u`, `_p`, `_tvp`, `_time`).  Underneath, the CasADi
Functions, the IDAS integrator of [x; P] and the dense update of make_step (:281-311) are one launch of csrc/dompc_ekf.hip behind
the C ABI `dompc_ekf_*` (include/dompc_ipm.h): `step_batch(...)` advances B independent filters with one launch,
`step_batch_device(...)` does the same in place on device pointers.  The reference integrates with IDAS at CasADi's default
tolerances; here `settings.abstol` / `reltol` (default 1e-10, like the Simulator of this package) steer an explicit Dormand-Prince
pair with step-size control on [x; P] - there is no implicit method for a stiff covariance equation.

Models with algebraic states (`_z`; x' = f(x, u, z), 0 = g(x, u, z), y = h(x, u, z)).  The reference hands z and g to IDAS but asserts
n_alg == 0 ('EKF with algebraic equations not ready for use!'), and by default `setup()` here refuses such a model too.  With
`settings.dae_reduction = True` the filter runs on the reduced system z = zeta(x, u), with the reference's evaluation points carried
over: A_k = f_x - f_z g_z^-1 g_x and C_k = h_x - h_z g_z^-1 g_x at the prior estimate (x0, zeta(x0, u)); discrete models
x- = f(x0, u, zeta(x0, u)), continuous models [x; P] integrated with the reduced A along the trajectory, every stage solving g = 0;
the measurement function h(x-, u, zeta(x-, u)).  Newton on g = 0 (`settings.z_tol`, `settings.z_max_iter`) and the reduction run
inside the launch.  `z0` (zeros after setup) is the guess of the first solve; `step_batch(..., Z0=)` returns `Z`, the algebraic
states consistent with the a-priori state x- - the last solve of the step and the warm start for the next call, NOT z at the
posterior - and `newton`, the Newton updates of each filter.  Status bit 2: an iteration did not converge, or g_z was singular or
not finite; that filter keeps its prior x, P and its Z0.

There is no CPU fallback: without a HIP device `setup()` raises.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from . import _native, build, lowering
from .model import Model
from .simulator import _flat_struct, _rows
from .structs import NumStruct


@dataclass
class EKFSettings:
    """`t_step` of the reference's EstimatorSettings; tolerances and step limit of the covariance integration (continuous models)"""
    t_step: float = None
    abstol: float = 1e-10
    reltol: float = 1e-10
    max_steps: int = 0                    # integration steps per filter and call (0 = 200000)
    gpu_index: int = 0
    dae_reduction: bool = False           # models with algebraic states: filter the reduced system z = zeta(x, u) (else: refused)
    z_tol: float = 1e-10                  # ... Newton on g = 0 stops at max |g| <= z_tol
    z_max_iter: int = 20                  # ... or after this many updates of one solve (status bit 2)

    def check_for_mandatory_settings(self):
        if self.t_step is None:
            raise ValueError("t_step must be set")


class EKFDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("nx", "nu", "np", "ntvp", "ny", "discrete")] + \
               [("code_object_path", C.c_char_p), ("model_hash", C.c_char_p), ("device", C.c_int32), ("max_steps", C.c_int32),
                ("t_step", C.c_double), ("reltol", C.c_double), ("abstol", C.c_double),
                ("nz", C.c_int32), ("z_max_iter", C.c_int32), ("z_tol", C.c_double)]


def _bind(lib_path: str) -> C.CDLL:
    lib = C.CDLL(lib_path)
    vp = C.c_void_p
    lib.dompc_ekf_create.argtypes = [C.POINTER(EKFDesc), C.POINTER(vp)]
    lib.dompc_ekf_create.restype = C.c_int
    lib.dompc_ekf_destroy.argtypes = [vp]
    lib.dompc_ekf_last_error.argtypes = [vp]
    lib.dompc_ekf_last_error.restype = C.c_char_p
    lib.dompc_ekf_step_batch.argtypes = [vp, C.c_int32] + [vp] * 8 + [C.c_int32] + [vp] * 3
    lib.dompc_ekf_step_batch.restype = C.c_int
    lib.dompc_ekf_step_batch_device.argtypes = [vp, C.c_int32] + [vp] * 8 + [C.c_int32] + [vp] * 2
    lib.dompc_ekf_step_batch_device.restype = C.c_int
    lib.dompc_ekf_step_dae_batch.argtypes = [vp, C.c_int32] + [vp] * 9 + [C.c_int32] + [vp] * 5
    lib.dompc_ekf_step_dae_batch.restype = C.c_int
    lib.dompc_ekf_step_dae_batch_device.argtypes = [vp, C.c_int32] + [vp] * 9 + [C.c_int32] + [vp] * 3
    lib.dompc_ekf_step_dae_batch_device.restype = C.c_int
    return lib


def _mats(a, n: int, B: int, what: str):
    """-> (contiguous f64 array, shared flag): one n x n matrix shared by the batch, or [B][n][n]"""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if a.shape == (n, n):
        return a, True
    if a.shape != (B, n, n):
        raise ValueError(f"{what}: expected shape ({n}, {n}) or ({B}, {n}, {n}), got {a.shape}")
    return a, False


class EKF:
    def __init__(self, model: Model):
        assert model.flags["setup"] is True, "Model for estimator was not setup. After the complete model creation call model.setup()."
        self.model = model
        self.settings = EKFSettings()
        self.flags = {"setup": False, "set_initial_guess": False, "set_tvp_fun": False, "set_p_fun": False, "first_step": True}
        self._x0 = model._x(0.0)
        self._z0 = model._z(0.0)
        self._t0 = np.array([0.0])
        self._P0 = np.eye(model.n_x)
        from .controller import MPCData
        self.data = MPCData(model)
        self._native = _native.Native("ekf", _bind, build.ekf_code_object)

    _lib = property(lambda self: self._native.lib)     # the bound library and the native handle (None before setup / after close)
    _h = property(lambda self: self._native.h)

    # ------------------------------------------------------------------ iterated variables
    def _set_x0(self, v):
        a = np.asarray(v.master if hasattr(v, "master") else v, dtype=float).reshape(-1)
        assert a.size == self.model.n_x, f"x0 has incorrect size {a.size}, expected {self.model.n_x}"
        self._x0.master[:] = a

    def _set_z0(self, v):
        a = np.asarray(v.master if hasattr(v, "master") else v, dtype=float).reshape(-1)
        assert a.size == self.model.n_z, f"z0 has incorrect size {a.size}, expected {self.model.n_z}"
        self._z0.master[:] = a

    x0 = property(lambda self: self._x0, _set_x0)
    z0 = property(lambda self: self._z0, _set_z0)          # models with algebraic states: the guess of the next step's first Newton solve
    t0 = property(lambda self: self._t0)

    @property
    def P0(self) -> np.ndarray:
        """error covariance of the estimate (n_x x n_x); the identity until it is set (_ekf.py:61-100)"""
        return self._P0

    @P0.setter
    def P0(self, val):
        if not isinstance(val, np.ndarray):
            raise TypeError(f"P0 must be a numpy.ndarray, got {type(val).__name__}")
        if val.ndim != 2:
            raise ValueError(f"P0 must be a 2D matrix, got {val.ndim}D array")
        if val.shape[0] != val.shape[1]:
            raise ValueError(f"P0 must be square, got shape {val.shape}")
        if val.shape[0] != self.model.n_x:
            raise ValueError(f"P0 must have shape ({self.model.n_x}, {self.model.n_x}) to match state dimension, got {val.shape}")
        self._P0 = np.array(val, dtype=float)

    # ------------------------------------------------------------------ configuration
    def get_p_template(self) -> NumStruct:
        return self.model._p(0.0)

    def set_p_fun(self, p_fun: Callable) -> None:
        assert isinstance(p_fun(0), NumStruct), "p_fun has incorrect return type."
        assert self.get_p_template().labels() == p_fun(0).labels(), \
            "Incorrect output of p_fun. Use get_p_template to obtain the required structure."
        self.p_fun = p_fun
        self.flags["set_p_fun"] = True

    def get_tvp_template(self) -> NumStruct:
        return self.model._tvp(0.0)

    def set_tvp_fun(self, tvp_fun: Callable) -> None:
        assert isinstance(tvp_fun(0), NumStruct), "tvp_fun has incorrect return type."
        assert self.get_tvp_template().labels() == tvp_fun(0).labels(), \
            "Incorrect output of tvp_fun. Use get_tvp_template to obtain the required structure."
        self.tvp_fun = tvp_fun
        self.flags["set_tvp_fun"] = True

    def _check_validity(self):
        if not self.flags["set_tvp_fun"] and self.model.n_tvp > 0:
            raise Exception("You have not supplied a function to obtain the time-varying parameters defined in model. "
                            "Use .set_tvp_fun() prior to setup.")
        if not self.flags["set_p_fun"] and self.model.n_p > 0:
            raise Exception("You have not supplied a function to obtain the parameters defined in model. Use .set_p_fun() prior to setup.")
        if not self.flags["set_tvp_fun"]:
            tvp0 = self.get_tvp_template()
            self.set_tvp_fun(lambda t: tvp0)
        if not self.flags["set_p_fun"]:
            p0 = self.get_p_template()
            self.set_p_fun(lambda t: p0)

    def _lower(self) -> str:
        m = self.model
        return lowering.lower_ekf(
            x_sym=m._x.cat.nodes(), u_sym=m._u.cat.nodes(), tvp_sym=m._tvp.cat.nodes(), p_sym=m._p.cat.nodes(),
            w_sym=m._w.cat.nodes(), v_sym=m._v.cat.nodes(), rhs=m._rhs.nodes(), meas=m._y.cat.nodes(),
            discrete=m.model_type == "discrete", name=type(m).__name__,
            z_sym=m._z.cat.nodes(), alg=(m._alg.nodes() if m.n_z else []), dae_reduction=bool(self.settings.dae_reduction))

    def setup(self, _lib_path: Optional[str] = None, _code_object: Optional[str] = None) -> None:
        self.settings.check_for_mandatory_settings()
        m = self.model
        # (refuses by name: algebraic states without settings.dae_reduction, more than 16 states / measurements / algebraic states)
        self.generated_header = self._lower()
        self.model_hash = self.generated_header.rsplit('EKF_MODEL_HASH "', 1)[1].split('"')[0]
        self._check_validity()
        self._native = _native.Native("ekf", _bind, build.ekf_code_object, _lib_path, _code_object)
        self.code_object = _code_object = self._native.load(self.generated_header, self.model_hash)
        d = EKFDesc(nx=m.n_x, nu=m.n_u, np=m.n_p, ntvp=m.n_tvp, ny=m.n_y, discrete=1 if m.model_type == "discrete" else 0,
                    code_object_path=_code_object.encode(), model_hash=self.model_hash.encode(),
                    device=self.settings.gpu_index, max_steps=self.settings.max_steps,
                    t_step=float(self.settings.t_step), reltol=float(self.settings.reltol), abstol=float(self.settings.abstol),
                    nz=m.n_z, z_max_iter=int(self.settings.z_max_iter), z_tol=float(self.settings.z_tol))
        self._native.create(d)
        self.counter = 0
        self.flags["setup"] = True

    def _check(self, rc):
        self._native.check(rc)

    def close(self):
        self._native.close()

    def set_initial_guess(self) -> None:
        assert self.flags["setup"] is True, "EKF was not setup yet. Please call EKF.setup()."
        self.flags["set_initial_guess"] = True

    def reset_history(self) -> None:
        self.data.init_storage()
        self._t0 = np.array([0.0])
        self.counter = 0

    # ------------------------------------------------------------------ runtime
    def step_batch(self, X, Pcov, Y, U, Q, R, P=None, TVP=None, Z0=None) -> dict:
        """One filter step of B independent filters.  X: [B][nx] prior estimates, Pcov: [B][nx][nx] their covariances, Y: [B][ny]
        measurements, U: [B][nu] or one row; Q (nx x nx) and R (ny x ny): one matrix or one per filter; P / TVP: [B][n] or one row
        (default p_fun(t0) / tvp_fun(t0)).  Returns {'x', 'P', 'status', 'n_steps'}: the posterior; status bit 0 = the integration did
        not reach t_step, bit 1 = S singular or not finite (the a-priori estimate is returned).
        Models with algebraic states: Z0 [B][nz] or one row, the guess of the first Newton solve (default `z0`); the result also has
        'Z' (the algebraic states consistent with the a-priori state x-: the last solve of the step, the warm start for the next
        call - not z at the posterior) and 'newton' (int32, Newton updates of each filter); status bit 2 = a Newton iteration did not
        converge, or g_z was singular or not finite (with bit 0 when it happens during the integration): that filter hands back its
        prior x, P and its Z0."""
        assert self.flags["setup"], "EKF was not setup yet. Please call EKF.setup()."
        m = self.model
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float64)).reshape(-1, m.n_x)
        B = X.shape[0]
        Pc = np.ascontiguousarray(np.asarray(Pcov, dtype=np.float64))
        if Pc.shape != (B, m.n_x, m.n_x):
            raise ValueError(f"Pcov: expected shape ({B}, {m.n_x}, {m.n_x}), got {Pc.shape}")
        Yv = np.ascontiguousarray(np.asarray(Y, dtype=np.float64)).reshape(B, m.n_y) if m.n_y else np.zeros((B, 1))
        t0 = float(self._t0[0])
        u, su = _rows(U, m.n_u, B)
        p, sp = _rows(P if P is not None else self.p_fun(t0), m.n_p, B)
        tvp, st = _rows(TVP if TVP is not None else self.tvp_fun(t0), m.n_tvp, B)
        Qm, sq = _mats(Q, m.n_x, B, "Q")
        Rm, sr = _mats(R, m.n_y, B, "R") if m.n_y else (np.zeros(1), True)
        mask = (1 if su else 0) | (2 if st else 0) | (4 if sp else 0) | (8 if sq else 0) | (16 if sr else 0)
        xo, Po = np.empty_like(X), np.empty_like(Pc)
        status = np.zeros(B, dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        if m.n_z:
            z = np.asarray(self._z0.master if Z0 is None else Z0, dtype=np.float64)
            if z.shape not in ((m.n_z,), (1, m.n_z), (B, m.n_z)):
                raise ValueError(f"Z0: expected shape ({m.n_z},) or ({B}, {m.n_z}), got {z.shape}")
            z = np.ascontiguousarray(np.broadcast_to(z.reshape(-1, m.n_z), (B, m.n_z)))
            zo, newton = np.empty_like(z), np.zeros(B, dtype=np.int32)
            rc = self._lib.dompc_ekf_step_dae_batch(self._h, B, ptr(X), ptr(Pc), ptr(Yv), ptr(u), ptr(z), ptr(tvp), ptr(p), ptr(Qm), ptr(Rm),
                                                    mask, ptr(xo), ptr(Po), ptr(zo), ptr(newton), ptr(status))
            self._check(rc)
            return {"x": xo, "P": Po, "status": status & 0xFF, "n_steps": status >> 8, "Z": zo, "newton": newton}
        rc = self._lib.dompc_ekf_step_batch(self._h, B, ptr(X), ptr(Pc), ptr(Yv), ptr(u), ptr(tvp), ptr(p), ptr(Qm), ptr(Rm), mask,
                                            ptr(xo), ptr(Po), ptr(status))
        self._check(rc)
        return {"x": xo, "P": Po, "status": status & 0xFF, "n_steps": status >> 8}

    def step_batch_device(self, B, x, Pcov, y, u, tvp, p, Q, R, status=0, shared_mask=0, stream=0, z=0, newton=0):
        """All arguments are raw device addresses (ints, e.g. torch tensor .data_ptr()); x and Pcov are updated in place;
        asynchronous on `stream`.  shared_mask: bit 0/1/2/3/4 = u/tvp/p/Q/R is one row shared by all filters.
        Models with algebraic states: z [B][nz], guess in, the algebraic states consistent with the a-priori state out, in place (0: the
        guess is 0 and nothing is handed back); newton [B] int32 (0: not wanted)."""
        if self.model.n_z:
            args = [C.c_void_p(int(a) if a else None) for a in (x, Pcov, y, u, z, tvp, p, Q, R)]
            rc = self._lib.dompc_ekf_step_dae_batch_device(self._h, int(B), *args, int(shared_mask), C.c_void_p(int(newton) if newton else None),
                                                           C.c_void_p(int(status) if status else None),
                                                           C.c_void_p(int(stream) if stream else None))
            self._check(rc)
            return
        args = [C.c_void_p(int(a) if a else None) for a in (x, Pcov, y, u, tvp, p, Q, R)]
        rc = self._lib.dompc_ekf_step_batch_device(self._h, int(B), *args, int(shared_mask), C.c_void_p(int(status) if status else None),
                                                   C.c_void_p(int(stream) if stream else None))
        self._check(rc)

    def make_step(self, y_next, u_next, Q_k, R_k) -> np.ndarray:
        """One step of the filter (_ekf.py:231-329): the new state estimate from the measurement `y_next` and the input `u_next` with
        the process / measurement noise covariances Q_k / R_k; stores it in x0 (and the covariance in P0) and returns it as a column."""
        assert self.flags["setup"] is True, "EKF was not setup yet. Please call EKF.setup()."
        assert self.flags["set_initial_guess"] is True, "Initial guess was not provided. Please call EKF.set_initial_guess()."
        m = self.model
        Q_k, R_k = np.asarray(Q_k), np.asarray(R_k)
        assert Q_k.shape == (m.n_x, m.n_x), "Q_k must be a square matrix of shape ({}, {})".format(m.n_x, m.n_x)
        assert R_k.shape == (m.n_y, m.n_y), "R_k must be a square matrix of shape ({}, {})".format(m.n_y, m.n_y)
        self.flags["first_step"] = False
        # p_fun / tvp_fun see the time BEFORE the step; the record gets the time AFTER it (the reference's `t0` is an alias of the
        # array it then increments in place, _ekf.py:268-279, 326)
        t0 = float(self._t0[0])
        tvp0 = _flat_struct(self.tvp_fun(t0), m.n_tvp)
        p0 = _flat_struct(self.p_fun(t0), m.n_p)
        u = np.asarray(u_next.master if hasattr(u_next, "master") else u_next, dtype=float).reshape(-1)
        assert u.size == m.n_u, "u_next has incorrect shape. You have: {}, expected: {}".format(u.shape, (m.n_u, 1))
        y = np.asarray(y_next.master if hasattr(y_next, "master") else y_next, dtype=float).reshape(-1)
        assert y.size == m.n_y, "y_next has incorrect shape. You have: {}, expected: {}".format(y.shape, (m.n_y, 1))
        self.counter += 1
        r = self.step_batch(self._x0.master[None, :], self._P0[None, :, :], y[None, :], u, Q_k, R_k, P=p0, TVP=tvp0)
        self._t0 = self._t0 + self.settings.t_step
        if int(r["status"][0]) & 4:
            raise RuntimeError("EKF: Newton on the algebraic equations did not converge, or g_z is singular or not finite "
                               "(settings.z_tol, settings.z_max_iter, z0)")
        if int(r["status"][0]) & 1:
            raise RuntimeError("EKF: the integration of state and covariance did not reach t_step (step limit or NaN right-hand side)")
        self._x0.master[:] = r["x"][0]
        self._P0 = r["P"][0].copy()
        self.last_status = int(r["status"][0])
        if m.n_z:
            self._z0.master[:] = r["Z"][0]            # (consistent with the a-priori state: the warm start of the next step)
            self.data.update(_z=r["Z"][0])
        self.data.update(_x=r["x"][0], _u=u, _p=p0, _tvp=tvp0, _time=self._t0.copy())
        return r["x"][0].reshape(-1, 1)
