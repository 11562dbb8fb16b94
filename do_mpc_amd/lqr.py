"""Linear quadratic regulator with do_mpc.controller.LQR's user surface; the design is batched on the GPU.

Reference surface mirrored here (/root/reference/do_mpc/controller/_lqr.py): `LQR(model)` on a discrete `LinearModel`,
`settings.t_step` / `settings.n_horizon` (None = infinite horizon), `set_param`, `set_objective(Q, R, P)`, `set_rterm(delR)`
(inputRatePenalization mode), `set_setpoint(xss, uss)`, `setup()`, `make_step(x0) -> u0`, `reset_history`, `discrete_gain(A, B)`,
`data`, the iterated `x0`, `u0`, `t0`.  Two behaviours of the reference are kept on purpose: P defaults to Q (with a warning) on a
finite horizon, and the finite-horizon gain is the K of the LAST pass of the backward recursion, used as a constant.

Underneath, scipy's solve_discrete_are / the recursion of discrete_gain - and, for `gains_at`, the Jacobians of
do_mpc.model.linearize and the zero-order hold of LinearModel.discretize - are one launch of csrc/dompc_lqr.hip behind the C ABI
`dompc_lqr_*` (include/dompc_ipm.h): `gains_batch` designs B controllers for B discrete pairs, `gains_at` for B operating points of
a nonlinear model, `*_device` do the same on device pointers.  `setup()` is the batch of one.  A model with algebraic states
(index-1 DAE) is designed by `gains_at` on its original states and inputs: Newton on the algebraic equations and the reduction
A = f_x - f_z g_z^-1 g_x, B = f_u - f_z g_z^-1 g_u run inside the same launch (the reference's own route for such a model,
do_mpc.model.dae2odeconversion -> linearize -> LQR, is in model.py and needs nothing of the kernel).

There is no CPU fallback: without a HIP device `setup()` raises.
"""
from __future__ import annotations

import ctypes as C
import warnings
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _native, build, lowering
from .model import LinearModel, Model
from .simulator import _rows
from .structs import NumStruct


@dataclass
class LQRSettings:
    """`t_step`, `n_horizon` of the reference's LQRSettings; `tol` / `max_iter` end the doubling iteration of the infinite horizon"""
    t_step: float = None
    n_horizon: Optional[int] = None
    tol: float = 1e-13                    # relative change of the Riccati iterate
    max_iter: int = 50
    z_tol: float = 1e-10                  # models with algebraic states: Newton on g = 0 stops at max |g| <= z_tol ...
    z_max_iter: int = 20                  # ... or after z_max_iter updates (at most 127)
    gpu_index: int = 0

    def check_for_mandatory_settings(self):
        if self.t_step is None:
            raise ValueError("t_step must be set")


class LQRDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("nx", "nu", "n", "rate", "has_model", "discrete", "np", "ntvp")] + \
               [("code_object_path", C.c_char_p), ("model_hash", C.c_char_p), ("device", C.c_int32), ("n_horizon", C.c_int32),
                ("max_iter", C.c_int32), ("t_step", C.c_double), ("tol", C.c_double), ("nz", C.c_int32), ("z_max_iter", C.c_int32),
                ("z_tol", C.c_double)]


def _bind(lib_path: str) -> C.CDLL:
    lib = C.CDLL(lib_path)
    vp = C.c_void_p
    lib.dompc_lqr_create.argtypes = [C.POINTER(LQRDesc), C.POINTER(vp)]
    lib.dompc_lqr_create.restype = C.c_int
    lib.dompc_lqr_destroy.argtypes = [vp]
    lib.dompc_lqr_last_error.argtypes = [vp]
    lib.dompc_lqr_last_error.restype = C.c_char_p
    lib.dompc_lqr_design_batch.argtypes = [vp, C.c_int32] + [vp] * 9 + [C.c_int32] + [vp] * 5
    lib.dompc_lqr_design_batch.restype = C.c_int
    lib.dompc_lqr_design_batch_device.argtypes = [vp, C.c_int32] + [vp] * 9 + [C.c_int32] + [vp] * 4
    lib.dompc_lqr_design_batch_device.restype = C.c_int
    lib.dompc_lqr_design_dae_batch.argtypes = [vp, C.c_int32] + [vp] * 8 + [C.c_int32] + [vp] * 6
    lib.dompc_lqr_design_dae_batch.restype = C.c_int
    lib.dompc_lqr_design_dae_batch_device.argtypes = [vp, C.c_int32] + [vp] * 10 + [C.c_int32] + [vp] * 5
    lib.dompc_lqr_design_dae_batch_device.restype = C.c_int
    lib.dompc_lqr_pairs_device.argtypes = [vp, C.c_int32, C.c_int32] + [vp] * 5 + [C.c_int32] + [vp] * 5
    lib.dompc_lqr_pairs_device.restype = C.c_int
    lib.dompc_lqr_tv_device.argtypes = [vp, C.c_int32, C.c_int32] + [vp] * 6 + [C.c_int32, vp, vp, C.c_int32] + [vp] * 4
    lib.dompc_lqr_tv_device.restype = C.c_int
    lib.dompc_lqr_tv.argtypes = [vp, C.c_int32, C.c_int32] + [vp] * 10 + [C.c_int32] + [vp] * 8
    lib.dompc_lqr_tv.restype = C.c_int
    return lib


def _mats(a, r: int, c: int, B: int, what: str):
    """-> (contiguous f64 array, shared flag): one r x c matrix shared by the batch, or [B][r][c]"""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if a.shape == (r, c):
        return a, True
    if a.shape != (B, r, c):
        raise ValueError(f"{what}: expected shape ({r}, {c}) or ({B}, {r}, {c}), got {a.shape}")
    return a, False


def _blkdiag(a, b):
    """diag(a, b) for one pair or a batch of pairs (either may be shared)"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    lead = a.shape[:-2] if a.ndim == 3 else b.shape[:-2]
    n, m = a.shape[-1], b.shape[-1]
    out = np.zeros(lead + (n + m, n + m))
    out[..., :n, :n] = a
    out[..., n:, n:] = b
    return out


def _rated(A, B):
    """design pair of inputRatePenalization mode: A~ = [[A, B], [0, I]], B~ = [[B], [I]] (_lqr.py:219-223)"""
    nu = B.shape[1]
    return np.block([[A, B], [np.zeros((nu, A.shape[1])), np.identity(nu)]]), np.block([[B], [np.identity(nu)]])


class _Design(_native.Native):
    """one code object + runtime handle (`lib`, `h`): (nx, nu, mode) without a model, or with the Jacobians of one"""

    def __init__(self, lqr: "LQR", model: Optional[Model]):
        nx, nu, rate = lqr.model.n_x, lqr.model.n_u, lqr.mode == "inputRatePenalization"
        if model is None:
            hdr = lowering.lower_lqr(nx=nx, nu=nu, rate=rate)
        else:
            assert model.flags["setup"] is True, "Run this function after original model is setup"
            assert (model.n_x, model.n_u) == (nx, nu), "the model must have the states and inputs of the controller's model"
            hdr = lowering.lower_lqr(nx=nx, nu=nu, rate=rate, x_sym=model._x.cat.nodes(), u_sym=model._u.cat.nodes(),
                                     tvp_sym=model._tvp.cat.nodes(), p_sym=model._p.cat.nodes(), w_sym=model._w.cat.nodes(),
                                     v_sym=model._v.cat.nodes(), z_sym=model._z.cat.nodes(), rhs=model._rhs.nodes(),
                                     discrete=model.model_type == "discrete", name=type(model).__name__,
                                     **({"alg": model._alg.nodes()} if model.n_z else {}))
        self.header = hdr
        self.hash = hdr.rsplit('LQR_MODEL_HASH "', 1)[1].split('"')[0]
        self.model = model
        super().__init__("lqr", _bind, build.lqr_code_object, lqr._emu, "")
        self.key = None                   # the settings the handle was created with


class LQR:
    def __init__(self, model: LinearModel):
        self.model = model
        assert isinstance(model, LinearModel), "LQR can only be used with linear models. Initialize the model with LinearModel class."
        assert model.flags["setup"] is True, "Model for LQR was not setup. After the complete model creation call model.setup()."
        assert model.model_type == "discrete", "Initialize LQR with discrete system. Discretize the system using LinearModel.discretize()"
        self.model_type = model.model_type
        self._x0 = model._x(0.0)
        self._u0 = model._u(0.0)
        self._t0 = np.array([0.0])
        from .controller import MPCData
        self.data = MPCData(model)
        self.settings = LQRSettings()
        self.mode = "standard"
        self.flags = {"setup": False}
        self._emu = None                  # TEST-ONLY: the host-emulation library, or (header, hash) -> host-emulation library
        self._designs = {}

    # ------------------------------------------------------------------ iterated variables (model/_iteratedvariables.py)
    def _set_iter(self, name, v):
        tgt = getattr(self, name)
        a = np.asarray(v.master if hasattr(v, "master") else v, dtype=float).reshape(-1)
        assert a.size == tgt.master.size, f"{name} has incorrect size {a.size}, expected {tgt.master.size}"
        tgt.master[:] = a

    x0 = property(lambda self: self._x0, lambda self, v: self._set_iter("_x0", v))
    u0 = property(lambda self: self._u0, lambda self, v: self._set_iter("_u0", v))
    t0 = property(lambda self: self._t0)

    # ------------------------------------------------------------------ configuration
    def reset_history(self) -> None:
        self._t0 = np.array([0.0])
        self.data.init_storage()

    def set_param(self, **kwargs) -> None:
        for key, value in kwargs.items():
            if hasattr(self.settings, key):
                setattr(self.settings, key, value)
            else:
                print("Warning: Key {} does not exist for MPC.".format(key))

    def set_objective(self, Q: np.ndarray, R: np.ndarray, P: np.ndarray = None) -> None:
        assert self.flags["setup"] is False, "Objective can not be set after LQR is setup"
        from . import sym
        symbolic = (sym.SX, sym.DM)
        self.Q, self.R = Q, R
        if P is None and self.settings.n_horizon is not None:
            self.P = Q
            warnings.warn("P is not given explicitly. Q is chosen as P for calculating finite discrete gain")
        else:
            self.P = P
        n_x, n_u = self.model.n_x, self.model.n_u
        assert self.Q.shape == (n_x, n_x), "Q must have shape = {}. You have {}".format((n_x, n_x), self.Q.shape)
        assert self.R.shape == (n_u, n_u), "R must have shape = {}. You have {}".format((n_u, n_u), self.R.shape)
        if isinstance(self.Q, symbolic):
            raise Exception("Q matrix must be of type class numpy.ndarray")
        if isinstance(self.R, symbolic):
            raise Exception("R matrix must be of type class numpy.ndarray")
        if self.settings.n_horizon is not None and isinstance(self.P, symbolic):
            raise Exception("P matrix must be of type class numpy.ndarray")
        if self.settings.n_horizon is not None:
            assert self.P.shape == self.Q.shape, "P must have same shape as Q. You have {}".format(self.P.shape)

    def set_rterm(self, delR: np.ndarray) -> None:
        """inputRatePenalization mode (_lqr.py:178-226): the input rate is the input of the design pair
        A~ = [[A, B], [0, I]], B~ = [[B], [I]] with the weights Q~ = diag(Q, R), R~ = delR"""
        self.A_rated, self.B_rated = _rated(self.model._A, self.model._B)
        self.delR = delR
        self.mode = "inputRatePenalization"

    def set_setpoint(self, xss: np.ndarray = None, uss: np.ndarray = None) -> None:
        assert self.flags["setup"] is True, "LQR is not setup. Run setup() function."
        n_x, n_u = self.model.n_x, self.model.n_u
        if isinstance(xss, np.ndarray):
            self.xss = xss
        elif not hasattr(self, "xss"):
            self.xss = np.zeros((n_x, 1))
        if isinstance(uss, np.ndarray):
            self.uss = uss
        elif not hasattr(self, "uss"):
            self.uss = np.zeros((n_u, 1))
        if self.mode == "inputRatePenalization":
            self.xss = np.block([[self.xss], [self.uss]])
            self.uss = np.zeros((n_u, 1))
            assert self.xss.shape == (n_x + n_u, 1), "xss must be of shape {}. You have {}".format((n_x + n_u, 1), self.xss.shape)
        if self.mode == "standard":
            assert self.xss.shape == (n_x, 1), "xss must be of shape {}. You have {}".format((n_x, 1), self.xss.shape)
        assert self.uss.shape == (n_u, 1), "uss must be of shape {}. You have {}".format((n_u, 1), self.uss.shape)

    # ------------------------------------------------------------------ native designs
    @property
    def n_design(self) -> int:
        return self.model.n_x + (self.model.n_u if self.mode == "inputRatePenalization" else 0)

    def _design(self, model: Optional[Model]) -> _Design:
        """handle for designs of this controller's size and mode (and `model`'s Jacobians), created on first use and again when a
        setting that the handle holds has changed"""
        key = (id(model) if model is not None else None, self.mode)
        d = self._designs.get(key)
        if d is None:
            d = self._designs[key] = _Design(self, model)
        s = self.settings
        nh = 0 if s.n_horizon is None else int(s.n_horizon)
        if nh < 1 and s.n_horizon is not None:
            raise ValueError(f"n_horizon must be None (infinite horizon) or at least 1, you have {s.n_horizon}")
        cont = model is not None and model.model_type == "continuous"
        nz = 0 if model is None else model.n_z
        skey = (nh, int(s.max_iter), float(s.tol), float(s.t_step) if cont else 0.0, int(s.gpu_index)) + \
            ((float(s.z_tol), int(s.z_max_iter)) if nz else ())
        if d.h is not None and d.key == skey:
            return d
        code_object = d.load(d.header, d.hash)
        desc = LQRDesc(nx=self.model.n_x, nu=self.model.n_u, n=self.n_design, rate=1 if self.mode == "inputRatePenalization" else 0,
                       has_model=0 if model is None else 1, discrete=0 if cont else 1,
                       np=0 if model is None else model.n_p, ntvp=0 if model is None else model.n_tvp,
                       code_object_path=code_object.encode(), model_hash=d.hash.encode(), device=s.gpu_index, n_horizon=nh,
                       max_iter=int(s.max_iter), t_step=float(s.t_step) if cont else 0.0, tol=float(s.tol), nz=nz,
                       z_max_iter=int(s.z_max_iter) if nz else 0, z_tol=float(s.z_tol) if nz else 0.0)
        d.create(desc)
        d.key = skey
        return d

    def header(self, model: Optional[Model] = None) -> str:
        """the lowered header of this controller's designs (without a model, or with `model`'s Jacobians)"""
        return _Design(self, model).header

    def close(self):
        for d in self._designs.values():
            d.close()

    def _weights(self, Q, R, P, B, finite=None):
        """design-size weights (Q~ = diag(Q, R), R~ = delR, P~ = diag(P, R) in inputRatePenalization mode, _lqr.py:484-490) from the
        arguments or, where they are missing, from set_objective / set_rterm -> (Q, R, P or None, shared mask bits 0..2)"""
        rate = self.mode == "inputRatePenalization"
        n_x, n_u, n = self.model.n_x, self.model.n_u, self.n_design
        tv = finite == "tv"                          # (the time-varying recursion: always finite, P defaults to Q)
        finite = self.settings.n_horizon is not None if finite is None else bool(finite)
        Qs = self._Q_user if Q is None else Q
        Rs = self._R_user if R is None else R
        Ps = (self._P_user if P is None else P) if finite else None
        if tv and (Ps is None or np.size(Ps) == 0):
            Ps = Qs
        assert Qs is not None and Rs is not None and np.size(Qs) != 0 and np.size(Rs) != 0, \
            "Enter tuning parameter Q and R for the lqr problem using set_objective() function."
        if finite:
            assert Ps is not None and np.size(Ps) != 0, \
                "Terminal cost is required to calculate gain. Enter the required value using set_objective() function."
        if rate:
            if not hasattr(self, "delR"):
                raise AttributeError("set delR using set_rterm fun to execute in inputRatePenalization mode.")
            Qs, Rs = np.asarray(Qs, float), np.asarray(Rs, float)
            if Qs.shape[-1] == n_x:                      # (weights of the model's size: assemble the design-size ones)
                Qd = _blkdiag(Qs, Rs)
                Pd = _blkdiag(Ps, Rs) if finite else None
                Rd = np.asarray(self.delR, float)
            else:
                Qd, Pd, Rd = Qs, Ps, Rs
        else:
            Qd, Rd, Pd = Qs, Rs, Ps
        Qd, sq = _mats(Qd, n, n, B, "Q")
        Rd, sr = _mats(Rd, n_u, n_u, B, "R")
        sp = True
        if finite:
            Pd, sp = _mats(Pd, n, n, B, "P")
        return Qd, Rd, Pd, (1 if sq else 0) | (2 if sr else 0) | (4 if sp else 0)

    def gains_batch(self, A, B, Q=None, R=None, P=None) -> dict:
        """Designs for Bn discrete pairs A [Bn][nx][nx], B [Bn][nx][nu] in one launch, in this controller's mode and horizon.  Q, R, P:
        one matrix or one per design, of the model's size (in inputRatePenalization mode R~ = delR of set_rterm, Q~ = diag(Q, R)) or
        already of design size; default: the weights of set_objective.  Returns {'K': [Bn][nu][n], 'P': [Bn][n][n], 'iters', 'status'};
        status bit 0 = the doubling did not converge (pair not stabilisable or not detectable), bit 1 = singular or non-finite block
        (K = 0, P = Q)."""
        m = self.model
        A = np.ascontiguousarray(np.asarray(A, dtype=np.float64))
        if A.ndim != 3 or A.shape[1:] != (m.n_x, m.n_x):
            raise ValueError(f"A: expected shape (Bn, {m.n_x}, {m.n_x}), got {A.shape}")
        Bn = A.shape[0]
        Bm = np.ascontiguousarray(np.asarray(B, dtype=np.float64))
        if Bm.shape != (Bn, m.n_x, m.n_u):
            raise ValueError(f"B: expected shape ({Bn}, {m.n_x}, {m.n_u}), got {Bm.shape}")
        return self._run(None, Bn, A, Bm, None, None, None, None, Q, R, P)

    def gains_at(self, model: Model, XSS, USS, TVP=None, P=None, Q=None, R=None, PAR=None, Z0=None, z_out: bool = True) -> dict:
        """Designs at Bn operating points XSS [Bn][nx], USS [Bn][nu] of the nonlinear `model` in ONE launch: Jacobians at the
        points, zero-order hold over settings.t_step for a continuous model, Riccati solution and gain.  Q, R, P: the weights, as in
        gains_batch (P is the terminal weight of a finite horizon).  TVP / PAR: the model's time-varying and constant parameters, one
        row or one per point.  Returns what gains_batch returns plus 'A', 'B': the discrete pairs.

        A model with algebraic states (x' = f(x, u, z), 0 = g(x, u, z)) is designed on its ORIGINAL states and inputs: Z0 [Bn][nz] or
        [nz] (default 0) is the guess of the algebraic states, every design solves g = 0 for z by Newton's method (settings.z_tol,
        settings.z_max_iter) and linearises the reduced system x' = f(x, u, zeta(x, u)): A = f_x - f_z g_z^-1 g_x, B = f_u - f_z
        g_z^-1 g_u, exact at any operating point.  The dict then holds 'Z' [Bn][nz], the consistent algebraic states (unless
        z_out=False), and 'newton', the Newton updates of every design; status bit 2 = Newton did not converge, or g_z singular or
        not finite at the last iterate (K = 0, P = Q, A = B = 0)."""
        m = self.model
        X = np.ascontiguousarray(np.asarray(XSS, dtype=np.float64)).reshape(-1, m.n_x)
        Bn = X.shape[0]
        U = np.ascontiguousarray(np.asarray(USS, dtype=np.float64)).reshape(Bn, m.n_u)
        if model.model_type == "continuous":
            self.settings.check_for_mandatory_settings()
        Z = None
        if model.n_z:
            Z = np.zeros((Bn, model.n_z)) if Z0 is None else np.asarray(Z0, dtype=np.float64)
            Z = np.ascontiguousarray(np.broadcast_to(Z.reshape(-1, model.n_z), (Bn, model.n_z)))
        return self._run(model, Bn, None, None, X, U, TVP, PAR, Q, R, P, Z, z_out)

    def _run(self, model, Bn, A, Bm, X, U, TVP, Pm, Q, R, Pt, Z=None, z_out=True) -> dict:
        d = self._design(model)
        lib = d.lib
        m = self.model
        n, n_u = self.n_design, m.n_u
        Qd, Rd, Pd, mask = self._weights(Q, R, Pt, Bn)
        tvp = p = None
        if model is not None:
            tvp, st = _rows(TVP, model.n_tvp, Bn)
            p, sp = _rows(Pm, model.n_p, Bn)
            mask |= (8 if st else 0) | (16 if sp else 0)
            A, Bm = None, None
        K = np.empty((Bn, n_u, n))
        Pout = np.empty((Bn, n, n))
        Ao = np.empty((Bn, m.n_x, m.n_x)) if model is not None else None
        Bo = np.empty((Bn, m.n_x, m.n_u)) if model is not None else None
        status = np.zeros(Bn, dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None      # noqa: E731
        Zo = np.empty_like(Z) if Z is not None and z_out else None
        if Z is not None:
            rc = lib.dompc_lqr_design_dae_batch(d.h, Bn, ptr(X), ptr(U), ptr(Z), ptr(tvp), ptr(p), ptr(Qd), ptr(Rd), ptr(Pd), mask,
                                                ptr(K), ptr(Pout), ptr(Ao), ptr(Bo), ptr(Zo), ptr(status))
        else:
            rc = lib.dompc_lqr_design_batch(d.h, Bn, ptr(A), ptr(Bm), ptr(X), ptr(U), ptr(tvp), ptr(p), ptr(Qd), ptr(Rd), ptr(Pd), mask,
                                            ptr(K), ptr(Pout), ptr(Ao), ptr(Bo), ptr(status))
        d.check(rc)
        out = {"K": K, "P": Pout, "iters": (status >> 8) & 0xFFFF, "status": status & 0xFF}
        if model is not None:
            out["A"], out["B"] = Ao, Bo
        if Z is not None:
            out["newton"] = status >> 24
            if Zo is not None:
                out["Z"] = Zo
        return out

    def gains_batch_device(self, Bn, A, B, Q, R, K, P, P_term=0, status=0, shared_mask=0, stream=0):
        """gains_batch on raw device addresses (ints, e.g. torch tensor .data_ptr()), asynchronous on `stream`.  Q, R, P_term are of
        DESIGN size; shared_mask: bit 0/1/2 = Q/R/P_term is one matrix shared by all designs."""
        d = self._design(None)
        args = [C.c_void_p(int(a) if a else None) for a in (A, B, 0, 0, 0, 0, Q, R, P_term)]
        rc = d.lib.dompc_lqr_design_batch_device(
            d.h, int(Bn), *args, int(shared_mask), C.c_void_p(int(K)), C.c_void_p(int(P)), C.c_void_p(int(status) if status else None),
            C.c_void_p(int(stream) if stream else None))
        d.check(rc)

    def gains_at_device(self, model, Bn, x, u, Q, R, K, P, tvp=0, p=0, P_term=0, A=0, B=0, status=0, shared_mask=0, stream=0, z=0,
                        z_out=0):
        """gains_at on raw device addresses; A / B (optional) receive the discrete pairs.  shared_mask: bit 0/1/2/3/4 =
        Q/R/P_term/tvp/p is one row shared by all designs.  A model with algebraic states needs z [Bn][nz], the guess of the algebraic
        states; z_out [Bn][nz] (optional, may be z itself) receives the consistent ones."""
        d = self._design(model)
        vp = lambda a: C.c_void_p(int(a) if a else None)      # noqa: E731
        if model.n_z:
            rc = d.lib.dompc_lqr_design_dae_batch_device(
                d.h, int(Bn), *[vp(a) for a in (A, B, x, u, z, tvp, p, Q, R, P_term)], int(shared_mask), vp(K), vp(P), vp(z_out), vp(status),
                vp(stream))
        else:
            rc = d.lib.dompc_lqr_design_batch_device(
                d.h, int(Bn), *[vp(a) for a in (A, B, x, u, tvp, p, Q, R, P_term)], int(shared_mask), vp(K), vp(P), vp(status), vp(stream))
        d.check(rc)

    # ------------------------------------------------------------------ time-varying designs along trajectories
    def _run_tv(self, model, Bn, K, A, Bm, X, U, Z, tvp, p, mask, Q, R, P, P_traj) -> dict:
        d = self._design(model)
        m = self.model
        n, n_u = self.n_design, m.n_u
        Qd, Rd, Pd, wmask = self._weights(Q, R, P, Bn, finite="tv")
        Kout = np.empty((K, Bn, n_u, n))
        P0 = np.empty((Bn, n, n))
        Pt = np.empty((K + 1, Bn, n, n)) if P_traj else None
        Ao = np.empty((K, Bn, m.n_x, m.n_x)) if model is not None else None
        Bo = np.empty((K, Bn, m.n_x, m.n_u)) if model is not None else None
        Zo = np.empty((K, Bn, model.n_z)) if model is not None and model.n_z else None
        ps = np.zeros((K, Bn), dtype=np.int32) if model is not None else None
        status = np.zeros(Bn, dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None      # noqa: E731
        d.check(d.lib.dompc_lqr_tv(d.h, Bn, K, ptr(A), ptr(Bm), ptr(X), ptr(U), ptr(Z), ptr(tvp), ptr(p), ptr(Qd), ptr(Rd), ptr(Pd),
                                   mask | wmask, ptr(Kout), ptr(P0), ptr(Pt), ptr(Ao), ptr(Bo), ptr(Zo), ptr(ps), ptr(status)))
        out = {"K": Kout, "P0": P0, "status": status & 0xFF, "step": (status >> 8) & 0xFFFF}
        if Pt is not None:
            out["P"] = Pt
        if model is not None:
            out["A"], out["B"], out["pair_status"], out["newton"] = Ao, Bo, ps & 0xFF, ps >> 24
            if Zo is not None:
                out["Z"] = Zo
        return out

    def gains_tv_batch(self, A, B, Q=None, R=None, P=None, P_traj: bool = False) -> dict:
        """Time-varying LQR for Bn trajectories of K discrete pairs A [K][Bn][nx][nx], B [K][Bn][nx][nu] (one trajectory: without the
        batch axis) in one launch: P = P_f, then K_k = -(B_k'PB_k + R)^-1 B_k'PA_k, P <- Q + A_k'P(A_k + B_k K_k) for k = K-1 .. 0, in
        this controller's mode.  Q, R, P (terminal weight, default Q): as in gains_batch, one per trajectory or shared; there are no
        per-step weights.  settings.n_horizon is not read: the horizon is K.  Returns {'K': [K][Bn][nu][n], 'P0': [Bn][n][n], 'status',
        'step'} and, with P_traj=True, 'P': [K+1][Bn][n][n].  status bit 1 = singular or non-finite block, bit 2 = non-finite pair,
        met at step 'step': K_j = 0 for j <= step, the gains behind it are kept, P0 = Q."""
        m = self.model
        A = np.ascontiguousarray(np.asarray(A, dtype=np.float64))
        Bm = np.ascontiguousarray(np.asarray(B, dtype=np.float64))
        if A.ndim == 3:
            A, Bm = A[:, None], Bm[:, None]
        if A.ndim != 4 or A.shape[2:] != (m.n_x, m.n_x) or A.shape[0] < 1:
            raise ValueError(f"A: expected shape (K, Bn, {m.n_x}, {m.n_x}) with K >= 1, got {A.shape}")
        K, Bn = A.shape[:2]
        if Bm.shape != (K, Bn, m.n_x, m.n_u):
            raise ValueError(f"B: expected shape ({K}, {Bn}, {m.n_x}, {m.n_u}), got {Bm.shape}")
        return self._run_tv(None, Bn, K, np.ascontiguousarray(A), np.ascontiguousarray(Bm), None, None, None, None, None, 0, Q, R, P, P_traj)

    def gains_along(self, model: Model, X_traj, U_traj, TVP=None, PAR=None, Q=None, R=None, P=None, Z0=None, P_traj: bool = False) -> dict:
        """Time-varying LQR along Bn trajectories of the nonlinear `model`: knots X_traj [K][Bn][nx], U_traj [K][Bn][nu] (step-major,
        as the rollouts record them; one trajectory: without the batch axis).  One launch forms the discrete pair of every knot - the
        pair gains_at forms there: Jacobians frozen at (x*_k, u*_k), zero-order hold over settings.t_step for a continuous model,
        Newton and reduction for algebraic states (Z0 [K][Bn][nz], [nz] or None = 0) - and a second one runs the recursion of
        gains_tv_batch.  TVP: [ntvp], [K][ntvp] (shared by the trajectories) or [K][Bn][ntvp]; PAR: [np] or [Bn][np].  Returns what
        gains_tv_batch returns plus 'A', 'B' (the pairs), 'pair_status' [K][Bn] (bit 1 = the exponential failed, bit 2 = Newton or the
        reduction failed: the pair is zero and the trajectory reports status bit 2 at that step), 'newton' and, for a model with
        algebraic states, 'Z' [K][Bn][nz]."""
        m = self.model
        X = np.asarray(X_traj, dtype=np.float64)
        if X.ndim == 2:
            X = X[:, None]
        if X.ndim != 3 or X.shape[2] != m.n_x or X.shape[0] < 1:
            raise ValueError(f"X_traj: expected shape (K, Bn, {m.n_x}) with K >= 1, got {X.shape}")
        K, Bn = X.shape[:2]
        X = np.ascontiguousarray(X)
        U = np.ascontiguousarray(np.asarray(U_traj, dtype=np.float64).reshape(K, Bn, m.n_u))
        if model.model_type == "continuous":
            self.settings.check_for_mandatory_settings()
        mask, tvp, p = 8 | 16, None, None
        if model.n_tvp:
            tvp = np.zeros(model.n_tvp) if TVP is None else np.asarray(TVP, dtype=np.float64)
            if tvp.ndim == 3:
                if tvp.shape != (K, Bn, model.n_tvp):
                    raise ValueError(f"TVP: expected shape ({K}, {Bn}, {model.n_tvp}), got {tvp.shape}")
                mask &= ~8
            else:
                tvp = np.broadcast_to(tvp.reshape(-1, model.n_tvp), (K, model.n_tvp))
            tvp = np.ascontiguousarray(tvp)
        if model.n_p:
            p, sp = _rows(PAR, model.n_p, Bn)
            mask = mask if sp else mask & ~16
        Z = None
        if model.n_z:
            Z = np.zeros(model.n_z) if Z0 is None else np.asarray(Z0, dtype=np.float64)
            Z = np.ascontiguousarray(np.broadcast_to(Z if Z.ndim == 3 else Z.reshape(-1, model.n_z)[:1], (K, Bn, model.n_z)))
        return self._run_tv(model, Bn, K, None, None, X, U, Z, tvp, p, mask, Q, R, P, P_traj)

    def gains_tv_batch_device(self, Bn, K, A, B, Q, R, P_term, P0, K_traj=0, law_M=0, ld=0, P_traj=0, pair_status=0, status=0,
                              shared_mask=0, stream=0, _design=None):
        """gains_tv_batch on raw device addresses, asynchronous on `stream`.  Q, R, P_term are of DESIGN size (shared_mask bit 0/1/2 =
        one matrix shared by all trajectories).  Gains go to K_traj [K][Bn][nu][n] and / or, in standard mode, to law_M
        [K][nu][nx][ld] (ld >= Bn): the layout of the rollout's law record with law_step = ld."""
        d = self._design(None) if _design is None else _design
        vp = lambda a: C.c_void_p(int(a) if a else None)      # noqa: E731
        d.check(d.lib.dompc_lqr_tv_device(d.h, int(Bn), int(K), vp(A), vp(B), vp(pair_status), vp(Q), vp(R), vp(P_term), int(shared_mask),
                                          vp(K_traj), vp(law_M), int(ld), vp(P_traj), vp(P0), vp(status), vp(stream)))

    def gains_along_device(self, model, Bn, K, x, u, A, B, Q, R, P_term, P0, tvp=0, p=0, z=0, z_out=0, K_traj=0, law_M=0, ld=0, P_traj=0,
                           pair_status=0, status=0, shared_mask=0, stream=0, recursion=True):
        """gains_along on raw device addresses: the pairs launch (into A [K][Bn][nx][nx], B [K][Bn][nx][nu], which the caller
        provides) and the recursion launch behind it on `stream`.  shared_mask: bit 0/1/2 = Q/R/P_term shared, bit 3 = tvp is
        [K][ntvp], bit 4 = p is [np].  pair_status [K][Bn] (optional) lets the recursion see a failed knot; without it such a knot is
        a pair of zeros.  recursion=False: the pairs launch alone."""
        d = self._design(model)
        vp = lambda a: C.c_void_p(int(a) if a else None)      # noqa: E731
        d.check(d.lib.dompc_lqr_pairs_device(d.h, int(Bn), int(K), vp(x), vp(u), vp(z), vp(tvp), vp(p), int(shared_mask), vp(A), vp(B),
                                             vp(z_out), vp(pair_status), vp(stream)))
        if recursion:
            self.gains_tv_batch_device(Bn, K, A, B, Q, R, P_term, P0, K_traj, law_M, ld, P_traj, pair_status, status, shared_mask, stream, d)

    # ------------------------------------------------------------------ setup and runtime
    _Q_user = property(lambda self: getattr(self, "_Q0", getattr(self, "Q", None)))
    _R_user = property(lambda self: getattr(self, "_R0", getattr(self, "R", None)))
    _P_user = property(lambda self: getattr(self, "_P0", getattr(self, "P", None)))

    def discrete_gain(self, A: np.ndarray, B: np.ndarray) -> np.ndarray:
        """Gain of one discrete pair in DESIGN size (in inputRatePenalization mode: A_rated, B_rated) with the weights self.Q, self.R,
        self.P as they stand - finite horizon: the K of the last pass of the recursion; infinite horizon: from the Riccati solution
        (_lqr.py:127-176).  Computed on the GPU like every design."""
        assert self.Q.size != 0 and self.R.size != 0, "Enter tuning parameter Q and R for the lqr problem using set_objective() function."
        if self.settings.n_horizon is not None:
            assert self.P.size != 0, "Terminal cost is required to calculate gain. Enter the required value using set_objective() function."
        A, B = np.asarray(A, float), np.asarray(B, float)
        n_x, n_u, n = self.model.n_x, self.model.n_u, self.n_design
        if A.shape != (n, n) or B.shape != (n, n_u):
            raise ValueError(f"discrete_gain: expected A of shape ({n}, {n}) and B of shape ({n}, {n_u}) in {self.mode} mode, "
                             f"got {A.shape} and {B.shape}")
        if n != n_x:                       # the kernel forms [[A, B], [0, I]], [[B], [I]] itself from the model-size pair
            Ar, Br = _rated(A[:n_x, :n_x], B[:n_x])
            if not (np.array_equal(A, Ar) and np.array_equal(B, Br)):
                raise ValueError("discrete_gain: in inputRatePenalization mode the pair must be A~ = [[A, B], [0, I]], B~ = [[B], [I]]")
        r = self.gains_batch(A[None, :n_x, :n_x], B[None, :n_x, :], Q=self.Q, R=self.R, P=self.P)
        self.design_status, self.design_iters = int(r["status"][0]), int(r["iters"][0])
        if self.design_status & 2:
            raise RuntimeError("LQR: singular or non-finite block in the design (B'PB + R, R or I + G H)")
        if self.design_status & 1:
            warnings.warn("LQR: the Riccati iteration did not converge (the pair is not stabilisable or not detectable)")
        self.P_riccati = r["P"][0]
        return r["K"][0]

    def setup(self, _lib_path: Optional[str] = None, _code_object: Optional[str] = None) -> None:
        """Computes the gain K (on the GPU, the batch of one).  TEST-ONLY: `_lib_path` with `_code_object=""` selects the host
        emulation - the path of the library built for this controller's designs, or a callable (header, hash) -> path that builds
        the library of every design the controller asks for (gains_at needs one per model)."""
        self.settings.check_for_mandatory_settings()
        if _lib_path is not None:
            assert _code_object == "", "a library of its own is the host emulation: _code_object must be \"\""
            self._emu = _lib_path
        if self.mode in ["standard", None]:
            self.mode = "standard"
            self._Q0, self._R0, self._P0 = self.Q, self.R, self.P
            self.K = self.discrete_gain(self.model._A, self.model._B)
        elif self.mode == "inputRatePenalization":
            # design-size weights (_lqr.py:484-490)
            self._Q0, self._R0, self._P0 = self.Q, self.R, self.P
            if not (hasattr(self, "A_rated") and hasattr(self, "B_rated")):
                raise AttributeError("set delR using set_rterm fun to execute in inputRatePenalization mode.")
            zq = np.zeros((self.Q.shape[0], self.R.shape[1]))
            self.Q = np.block([[self.Q, zq], [zq.T, self.R]])
            if self.settings.n_horizon is not None:
                self.P = np.block([[self.P, zq], [zq.T, self.R]])
            self.R = self.delR
            self.K = self.discrete_gain(self.A_rated, self.B_rated)
        else:
            raise Exception("mode must be standard, inputRatePenalization, None. you have {}".format(self.mode))
        self.flags["setup"] = True

    def make_step(self, x0: np.ndarray) -> np.ndarray:
        assert self.flags["setup"] is True, "LQR is not setup. run setup() function."
        from . import sym
        if isinstance(x0, NumStruct):
            x0 = x0.master.reshape(-1, 1)
        elif isinstance(x0, sym.DM):
            x0 = np.asarray(x0.arr, float).reshape(-1, 1)
        elif not isinstance(x0, np.ndarray):
            raise Exception("Invalid type {} for x0. Must be {}".format(type(x0), (np.ndarray, sym.DM, NumStruct)))
        x0 = np.asarray(x0, float).reshape(-1, 1)
        if not hasattr(self, "xss") and not hasattr(self, "uss"):
            self.set_setpoint()
        u_prev = self._u0.master.reshape(-1, 1).copy()
        if self.mode == "standard":
            u0 = self.K @ (x0 - self.xss) + self.uss
        else:
            u0 = self.K @ (np.block([[x0], [u_prev]]) - self.xss) + self.uss + u_prev
        self.data.update(_x=x0, _u=u0, _time=self._t0.copy())
        self._t0 = self._t0 + self.settings.t_step
        self._x0.master[:] = x0.ravel()
        self._u0.master[:] = u0.ravel()
        return u0

    def make_step_batch(self, X, K=None, XSS=None, USS=None, U_prev=None):
        """u = K (x - xss) + uss (+ u_prev in inputRatePenalization mode, x then stacked with u_prev) for B members; X: [B][nx];
        K: self.K or [B][nu][n]; XSS / USS: one set-point (default: set_setpoint's) or one per member, of the MODEL's size.  numpy
        arrays give a numpy array, torch tensors (on any device) a tensor."""
        assert self.flags["setup"] is True, "LQR is not setup. run setup() function."
        m = self.model
        rate = self.mode == "inputRatePenalization"
        tensor = type(X).__module__.startswith("torch")
        if tensor:
            import torch
            conv = lambda a: a if type(a).__module__.startswith("torch") else torch.as_tensor(np.asarray(a, float), dtype=X.dtype, device=X.device)      # noqa: E731
            cat, zeros = (lambda a, b: torch.cat((a, b), dim=1)), (lambda s: torch.zeros(s, dtype=X.dtype, device=X.device))
        else:
            conv = lambda a: np.asarray(a, float)      # noqa: E731
            cat, zeros = (lambda a, b: np.concatenate((a, b), axis=1)), np.zeros
        X = conv(X).reshape(-1, m.n_x)
        B = X.shape[0]
        if XSS is None and USS is None and hasattr(self, "xss"):
            xs = np.asarray(self.xss, float).ravel()
            XSS, USS = xs[:m.n_x], (xs[m.n_x:] if rate else np.asarray(self.uss, float).ravel())
        xss = conv(XSS).reshape(-1, m.n_x) if XSS is not None else zeros((1, m.n_x))
        uss = conv(USS).reshape(-1, m.n_u) if USS is not None else zeros((1, m.n_u))
        Kb = conv(self.K if K is None else K).reshape(-1, m.n_u, self.n_design)
        if rate:
            up = conv(U_prev).reshape(B, m.n_u) if U_prev is not None else zeros((B, m.n_u))
            e = cat(X - xss, up - uss)
            return (Kb @ e[:, :, None])[:, :, 0] + up
        return (Kb @ (X - xss)[:, :, None])[:, :, 0] + uss
