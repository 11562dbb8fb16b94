"""Simulator - the plant side of the closed loop, batched on the GPU.

Mirror of the reference's `do_mpc.simulator.Simulator` surface (/root/reference/do_mpc/simulator.py:106-850):
`Simulator(model)`, `settings.t_step / abstol / reltol / integration_tool` (`set_param(**kw)` forwards to it),
`get_p_template / set_p_fun`, `get_tvp_template / set_tvp_fun`, `setup()`, the iterated variables `x0`, `u0`, `t0`,
`make_step(u0, v0=None, w0=None) -> y_next`.  Underneath, the CVODES integrator object of simulator.py:381-416 is
replaced by the batched Runge-Kutta integrator of csrc/dompc_plant.hip (explicit pair + implicit SDIRK) behind the C ABI `dompc_plant_*`
(include/dompc_ipm.h); `make_step_batch(X, U, ...)` advances B samples with one launch, and
`step_batch_device(...)` does the same on device pointers so that an x0 batch never leaves HBM between the
controller's `make_step_batch` calls.

There is no CPU fallback: without a HIP device `setup()` raises.  Stiff plants: `settings.integration_tool` ('cvodes' / 'idas':
explicit pair with an implicit repeat for stiff samples; 'sdirk4': implicit only; 'dopri5': explicit only).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional

import numpy as np

from . import _native, build, lowering, sym
from .model import Model
from .structs import Entry, Layout, NumStruct


@dataclass
class SimulatorSettings:
    """settings of the reference's ContinousSimulatorSettings (simulator.py:42-104)"""
    t_step: float = None
    abstol: float = 1e-10
    reltol: float = 1e-10
    # 'cvodes' / 'idas' (the reference's implicit integrators): explicit pair, stiff samples repeat their interval with the
    # implicit SDIRK method; 'dopri5': explicit only; 'sdirk4': implicit only (csrc/dompc_plant.hip)
    integration_tool: str = "cvodes"
    integration_opts: Dict = field(default_factory=dict)
    gpu_index: int = 0
    max_steps: int = 0                    # integration steps per sample and control interval (0 = 200000)

    def check_for_mandatory_settings(self):
        if self.t_step is None:
            raise ValueError("t_step must be set")


class PlantDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("nx", "nu", "np", "ntvp", "nw", "nv", "ny", "discrete")] + \
               [("code_object_path", C.c_char_p), ("model_hash", C.c_char_p), ("device", C.c_int32), ("max_steps", C.c_int32),
                ("t_step", C.c_double), ("reltol", C.c_double), ("abstol", C.c_double)]


class RolloutDesc(C.Structure):
    """dompc_plant_rollout_desc of include/dompc_ipm.h"""
    _fields_ = [(n, C.c_void_p) for n in ("law", "G", "up_ref", "U_prev0", "X_traj", "U_traj", "W_traj", "V_traj", "Y_traj", "Z_traj",
                                          "tvp_rows", "p_rows", "p_loops", "plant_status", "law_status")] + \
               [("reseed_z", C.c_int32), ("pad", C.c_int32), ("law_step", C.c_int64)]


class AmpcLoopDesc(C.Structure):
    """dompc_plant_ampc_loop_desc of include/dompc_ipm.h"""
    SHAPE = ("n_in", "n_out", "n_hidden_layers", "n_neurons", "act", "out_act", "scaling")
    _fields_ = [("w", C.c_void_p), ("par", C.c_void_p)] + [(n, C.c_int32) for n in SHAPE + ("clip",)] + \
               [(n, C.c_void_p) for n in ("U_prev0", "X_traj", "U_traj", "W_traj", "V_traj", "Y_traj", "Z_traj", "tvp_rows", "p_rows",
                                          "p_loops", "plant_status", "z_guess")] + \
               [("reseed_z", C.c_int32), ("pad", C.c_int32)]


def _bind(lib_path: str) -> C.CDLL:
    lib = C.CDLL(lib_path)
    vp = C.c_void_p
    lib.dompc_plant_create.argtypes = [C.POINTER(PlantDesc), C.POINTER(vp)]
    lib.dompc_plant_create.restype = C.c_int
    lib.dompc_plant_destroy.argtypes = [vp]
    lib.dompc_plant_last_error.argtypes = [vp]
    lib.dompc_plant_last_error.restype = C.c_char_p
    lib.dompc_plant_step_batch.argtypes = [vp, C.c_int32] + [vp] * 6 + [C.c_int32] + [vp] * 3
    lib.dompc_plant_step_batch.restype = C.c_int
    lib.dompc_plant_step_batch_device.argtypes = [vp, C.c_int32] + [vp] * 6 + [C.c_int32] + [vp] * 3 + [vp]
    lib.dompc_plant_step_batch_device.restype = C.c_int
    lib.dompc_plant_set_method.argtypes = [vp, C.c_int32, C.c_int32]
    lib.dompc_plant_set_method.restype = C.c_int
    lib.dompc_plant_set_z0.argtypes = [vp, vp]
    lib.dompc_plant_set_z0.restype = C.c_int
    lib.dompc_plant_set_z_carry.argtypes = [vp, C.c_int32]
    lib.dompc_plant_set_z_carry.restype = C.c_int
    lib.dompc_plant_num_alg_states.argtypes = [vp]
    lib.dompc_plant_num_alg_states.restype = C.c_int32
    lib.dompc_plant_rollout_affine_device.argtypes = [vp, C.c_int32, C.c_int32] + [vp] * 8
    lib.dompc_plant_rollout_affine_device.restype = C.c_int
    lib.dompc_plant_rollout_device.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(RolloutDesc), vp]
    lib.dompc_plant_rollout_device.restype = C.c_int
    lib.dompc_plant_ampc_loop_device.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(AmpcLoopDesc), vp]
    lib.dompc_plant_ampc_loop_device.restype = C.c_int
    lib.dompc_plant_z_guess_device.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(vp)]
    lib.dompc_plant_z_guess_device.restype = C.c_int
    return lib


def _rows(a, n: int, B: int):
    """-> (contiguous f64 array or None, shared flag): one row of n values shared by the batch, or [B][n]"""
    if n == 0:
        return np.zeros(1), True
    if a is None:
        return np.zeros(n), True
    if hasattr(a, "master"):
        a = a.master
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if a.size == n:
        return a.reshape(n), True
    if a.shape != (B, n):
        raise ValueError(f"expected {n} values or an array of shape ({B}, {n}), got {a.shape}")
    return a, False


def _flat_struct(v, n):
    return np.asarray(v.master if hasattr(v, "master") else v, dtype=float).reshape(-1)[:n] if n else np.zeros(0)


class Simulator:
    def __init__(self, model: Model):
        assert model.flags["setup"] is True, "Model for simulator was not setup. After the complete model creation call model.setup()."
        self.model = model
        self.settings = SimulatorSettings()
        if model.model_type == "discrete":
            self.settings.t_step = self.settings.t_step
        self._x0 = model._x(0.0)
        self._u0 = model._u(0.0)
        self._z0 = model._z(0.0)
        self._t0 = np.array([0.0])
        from .controller import MPCData                 # per-step records like the reference's simulator.data (simulator.py:833-841)
        self.data = MPCData(model)
        self.flags = {"set_tvp_fun": False, "set_p_fun": False, "setup": False, "first_step": True}
        self._native = _native.Native("plant", _bind, build.plant_code_object)
        self._pairs = {}                  # network hash -> the plant handle on the pair object of (this plant, that network shape)
        self._ampc_loop_lib = None        # TEST-ONLY: (plant header, network header, pair hash) -> host-emulation library of a pair

    _lib = property(lambda self: self._native.lib)     # the bound library and the native handle (None before setup / after close)
    _h = property(lambda self: self._native.h)

    # ------------------------------------------------------------------ iterated variables (model/_iteratedvariables.py)
    def _set_iter(self, name, v):
        tgt = getattr(self, name)
        a = np.asarray(v.master if hasattr(v, "master") else v, dtype=float).reshape(-1)
        assert a.size == tgt.master.size, f"{name} has incorrect size {a.size}, expected {tgt.master.size}"
        tgt.master[:] = a

    x0 = property(lambda self: self._x0, lambda self, v: self._set_iter("_x0", v))
    z0 = property(lambda self: self._z0, lambda self, v: self._set_iter("_z0", v))
    u0 = property(lambda self: self._u0, lambda self, v: self._set_iter("_u0", v))
    t0 = property(lambda self: self._t0)

    # ------------------------------------------------------------------ configuration
    def set_param(self, **kwargs) -> None:
        for k, v in kwargs.items():
            if not hasattr(self.settings, k):
                print(f"Warning: Key {k} does not exist for Simulator.")
            else:
                setattr(self.settings, k, v)

    def get_tvp_template(self) -> NumStruct:
        return self.model._tvp(0.0)

    def set_tvp_fun(self, tvp_fun: Callable) -> None:
        assert self.get_tvp_template().labels() == tvp_fun(0).labels(), \
            "Incorrect output of tvp_fun. Use get_tvp_template to obtain the required structure."
        self.tvp_fun = tvp_fun
        self.flags["set_tvp_fun"] = True

    def get_p_template(self) -> NumStruct:
        return self.model._p(0.0)

    def set_p_fun(self, p_fun: Callable) -> None:
        assert self.get_p_template().labels() == p_fun(0).labels(), \
            "Incorrect output of p_fun. Use get_p_template to obtain the required structure."
        self.p_fun = p_fun
        self.flags["set_p_fun"] = True

    def _check_validity(self):
        # simulator.py:299-319: default (constant zero) parameter functions when the model has none
        if not self.flags["set_tvp_fun"]:
            if self.model.n_tvp:
                raise Exception("You have not supplied a function to obtain the time-varying parameters defined in model. "
                                "Use .set_tvp_fun() prior to setup.")
            tvp0 = self.get_tvp_template()
            self.tvp_fun = lambda t: tvp0
        if not self.flags["set_p_fun"]:
            if self.model.n_p:
                raise Exception("You have not supplied a function to obtain the parameters defined in model. "
                                "Use .set_p_fun() prior to setup.")
            p0 = self.get_p_template()
            self.p_fun = lambda t: p0

    def _lower(self) -> str:
        m = self.model
        return lowering.lower_plant(
            x_sym=m._x.cat.nodes(), u_sym=m._u.cat.nodes(), tvp_sym=m._tvp.cat.nodes(), p_sym=m._p.cat.nodes(),
            w_sym=m._w.cat.nodes(), v_sym=m._v.cat.nodes(), rhs=m._rhs.nodes(), meas=m._y.cat.nodes(),
            discrete=m.model_type == "discrete", name=type(m).__name__,
            z_sym=m._z.cat.nodes(), alg=(m._alg.nodes() if m.n_z else []))

    def setup(self, _lib_path: Optional[str] = None, _code_object: Optional[str] = None) -> None:
        self.settings.check_for_mandatory_settings()
        self._check_validity()
        m = self.model
        self.generated_header = self._lower()
        self.model_hash = self.generated_header.rsplit('PLANT_MODEL_HASH "', 1)[1].split('"')[0]
        self._native = _native.Native("plant", _bind, build.plant_code_object, _lib_path, _code_object)
        _code_object = self._native.load(self.generated_header, self.model_hash)
        d = PlantDesc(nx=m.n_x, nu=m.n_u, np=m.n_p, ntvp=m.n_tvp, nw=m.n_w, nv=m.n_v, ny=m.n_y,
                      discrete=1 if m.model_type == "discrete" else 0,
                      code_object_path=_code_object.encode(), model_hash=self.model_hash.encode(),
                      device=self.settings.gpu_index, max_steps=self.settings.max_steps,
                      t_step=float(self.settings.t_step), reltol=float(self.settings.reltol), abstol=float(self.settings.abstol))
        self._native.create(d)
        h = self._h
        tool = str(self.settings.integration_tool).lower()
        methods = {"cvodes": 0, "idas": 0, "auto": 0, "dopri5": 1, "rk45": 1, "sdirk4": 2, "implicit": 2}
        if tool not in methods:
            raise ValueError(f"integration_tool {self.settings.integration_tool!r}: expected one of {sorted(methods)}")
        self._check(self._lib.dompc_plant_set_method(h, methods[tool], int(self.settings.integration_opts.get("explicit_limit", 0))))
        self._seed_z()
        self.flags["setup"] = True

    def _seed_z(self):
        """Newton start of the algebraic states on the device = simulator.z0 (simulator.py:603-620: sim_z_num)"""
        if self.model.n_z and self._h:
            z = np.ascontiguousarray(self._z0.master, dtype=np.float64)
            self._lib.dompc_plant_set_z0(self._h, z.ctypes.data_as(C.c_void_p))

    def _check(self, rc):
        self._native.check(rc)

    def close(self):
        self._native.close()
        for nat in self._pairs.values():
            nat.close()
        self._pairs = {}

    # ------------------------------------------------------------------ runtime
    def set_initial_guess(self) -> None:
        """Initial guess of the algebraic states for the DAE solver (simulator.py:603-620): `simulator.z0` becomes the Newton start of
        the algebraic equations for every sample (the kernel then continues from the values it found at the end of the previous
        step, like IDAS from sim_z_num); the records' z (`_host_z`) starts from the same values."""
        assert self.flags["setup"], "Simulator was not setup yet. Please call Simulator.setup()."
        self._seed_z()

    def _host_z(self, x, u, tvp, p) -> np.ndarray:
        """algebraic states at (x, u) for the data records (Newton's method on the model's own functions, from the last values)"""
        m = self.model
        if not m.n_z:
            return np.zeros(0)
        if getattr(self, "_algJ_fun", None) is None:
            from . import sym
            ins = [m._x.cat, m._u.cat, m._z.cat, m._tvp.cat, m._p.cat, m._w.cat]
            self._algJ_fun = sym.Function("alg_jz", ins, [sym.jacobian(m._alg, m._z.cat)])
        z, w = self._z0.master.copy(), np.zeros(m.n_w)
        for _ in range(30):
            a = np.asarray(m._alg_fun.eval(x, u, z, tvp, p, w)[0], float).ravel()
            J = np.asarray(self._algJ_fun.eval(x, u, z, tvp, p, w)[0], float).reshape(m.n_z, m.n_z, order="F")
            dz = np.linalg.solve(J, a)
            z = z - dz
            if np.max(np.abs(dz)) <= 1e-13 * max(1.0, np.max(np.abs(z))):
                break
        self._z0.master[:] = z
        return z

    def make_step_batch(self, X, U=None, P=None, TVP=None, W=None, V=None, carry_z: bool = False) -> dict:
        """Advance B samples by one control interval.  X: [B][nx]; U, P, TVP, W, V: [B][n] or one row shared by all
        samples (P / TVP default to p_fun(t0) / tvp_fun(t0)).  Returns {'x', 'y', 'status', 'n_steps'}; status bit 0: the integration
        did not reach t_step (failure), bit 1: the implicit method produced the result (no failure).
        DAE plants: the Newton iteration for the algebraic states of every sample starts from `simulator.z0` - unless `carry_z`, which
        says that row b of this call continues the trajectory of row b of the previous call (then from the values found there)."""
        assert self.flags["setup"], "Simulator is not setup. Call simulator.setup() first."
        m = self.model
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float64)).reshape(-1, m.n_x)
        B = X.shape[0]
        t0 = float(self._t0[0])
        u, su = _rows(U, m.n_u, B)
        p, sp = _rows(P if P is not None else self.p_fun(t0), m.n_p, B)
        tvp, st = _rows(TVP if TVP is not None else self.tvp_fun(t0), m.n_tvp, B)
        w, sw = _rows(W, m.n_w, B)
        v, sv = _rows(V, m.n_v, B)
        mask = (1 if su else 0) | (2 if st else 0) | (4 if sp else 0) | (8 if sw else 0) | (16 if sv else 0)
        xn = np.empty((B, m.n_x))
        y = np.empty((B, max(m.n_y, 1)))
        status = np.zeros(B, dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        self._lib.dompc_plant_set_z_carry(self._h, 1 if carry_z else 0)
        rc = self._lib.dompc_plant_step_batch(self._h, B, ptr(X), ptr(u), ptr(tvp), ptr(p), ptr(w), ptr(v), mask,
                                              ptr(xn), ptr(y), ptr(status))
        self._check(rc)
        return {"x": xn, "y": y[:, :m.n_y], "status": status & 0xFF, "n_steps": status >> 8}

    def step_batch_device(self, B, x, u, tvp, p, x_next, y=0, status=0, w=0, v=0, shared_mask=0, stream=0):
        """All arguments are raw device addresses (ints, e.g. torch tensor .data_ptr()); asynchronous on `stream`."""
        args = [C.c_void_p(int(a) if a else None) for a in (x, u, tvp, p, w, v)]
        outs = [C.c_void_p(int(a) if a else None) for a in (x_next, y, status)]
        rc = self._lib.dompc_plant_step_batch_device(self._h, int(B), *args, int(shared_mask), *outs,
                                                     C.c_void_p(int(stream) if stream else None))
        self._check(rc)

    def rollout_affine_device(self, B, K, law, X_traj, U_traj, tvp_rows=0, p_rows=0, plant_status=0, law_status=0, stream=0):
        """K control steps affine law -> plant step in ONE launch for B loops (`dompc_plant_rollout_affine_device`): for k = 0 .. K-1 the
        input u = sat(u_ref + M (x - x_ref)) at X_traj[k] goes to U_traj[k] and the plant step - the one of `step_batch_device` - from
        X_traj[k] with U_traj[k] to X_traj[k + 1].  `law`: a ctypes `dompc_affine_law` record (include/dompc_ipm.h; `ASMPC.law_record()`,
        or one filled by hand - an LQR gain schedule is such a law: x_ref = xss, u_ref = uss, M = K, arrays with the loops innermost).
        The other arguments are raw device addresses: X_traj [K + 1][B][nx] with row 0 filled, U_traj [K][B][nu], tvp_rows [K][n_tvp]
        and p_rows [K][n_p] (the plant's parameters of each step, shared by the batch), plant_status and law_status [K][B] int32 (or
        0).  No noise, no measurement; a loop whose plant step fails goes on.  Asynchronous on `stream`.  Plants with algebraic states
        are refused: step them with `step_batch_device`."""
        if self.model.n_z:
            raise NotImplementedError("Simulator.rollout_affine_device: plants with algebraic states are not served by the rollout "
                                      "(the step-wise path, step_batch_device, serves them)")
        ptrs = [C.c_void_p(int(a) if a else None) for a in (X_traj, U_traj, tvp_rows, p_rows, plant_status, law_status)]
        rc = self._lib.dompc_plant_rollout_affine_device(self._h, int(B), int(K), C.c_void_p(C.addressof(law)), *ptrs,
                                                         C.c_void_p(int(stream) if stream else None))
        self._check(rc)

    def rollout_device(self, B, K, X_traj, U_traj, law=None, G=0, up_ref=0, U_prev0=0, W_traj=0, V_traj=0, Y_traj=0, Z_traj=0,
                       tvp_rows=0, p_rows=0, p_loops=0, plant_status=0, law_status=0, reseed_z=False, stream=0, law_step=0):
        """K control steps of B loops in ONE launch, for every plant (`dompc_plant_rollout_device`, include/dompc_ipm.h).  Raw device
        addresses, asynchronous on `stream`.  X_traj [K + 1][B][nx] with row 0 filled; per step k the plant step of `step_batch_device`
        from X_traj[k] to X_traj[k + 1] with
          the input   `law` (a ctypes `dompc_affine_law` record) at X_traj[k], written to U_traj[k] [K][B][nu], its status to law_status
                      [K][B]; with G [nu][nu][ld] the law has a previous-input term, u = sat(u_ref + M (x - x_ref) + G (u_prev - up_ref)),
                      up_ref [nu][ld], u_prev = U_prev0 [B][nu] at k = 0 and the (clipped) input of step k - 1 afterwards.  Without a law
                      U_traj[k] is read: an open-loop simulation.  law_step = s > 0: a law record PER STEP - the record of step k is
                      `law` with x_ref, u_ref, M and flags advanced by k nx s, k nu s, k nu nx s and k s elements (arrays [K][nx][ld],
                      [K][nu][ld], [K][nu][nx][ld], [K][ld] with s = ld: the layout `LQR.gains_along_device(law_M=)` writes); lb, ub,
                      x_scale, clip and max_dx are shared by the steps; refused together with G / up_ref;
          parameters  tvp_rows [K][n_tvp] shared by the batch; p_rows [K][n_p] shared by the batch OR p_loops [B][n_p], one row per loop;
          noise       W_traj [K][B][nw], V_traj [K][B][nv] (0: none);
          records     Y_traj [K][B][ny] (the measurement at X_traj[k + 1]), Z_traj [K][B][nz] (the algebraic states there), plant_status
                      [K][B] (0: not kept).
        The Newton starts of the algebraic states are carried from step to step and from call to call like those of
        `step_batch_device`; reseed_z: they start from `simulator.z0`.  A loop whose plant step fails goes on from the state it reached."""
        r = RolloutDesc()
        r.law = C.addressof(law) if law is not None else None
        for name, a in (("G", G), ("up_ref", up_ref), ("U_prev0", U_prev0), ("X_traj", X_traj), ("U_traj", U_traj), ("W_traj", W_traj),
                        ("V_traj", V_traj), ("Y_traj", Y_traj), ("Z_traj", Z_traj), ("tvp_rows", tvp_rows), ("p_rows", p_rows),
                        ("p_loops", p_loops), ("plant_status", plant_status), ("law_status", law_status)):
            setattr(r, name, int(a) if a else None)
        r.reseed_z = 1 if reseed_z else 0
        r.law_step = int(law_step)
        rc = self._lib.dompc_plant_rollout_device(self._h, int(B), int(K), C.byref(r), C.c_void_p(int(stream) if stream else None))
        self._check(rc)

    def _pair(self, ampc) -> "_native.Native":
        """the plant handle on the code object of the pair (this plant, the shape of `ampc`'s network): built or loaded on first use,
        kept per network shape; the settings of setup() apply to it as to the plant's own handle"""
        nat = self._pairs.get(ampc.model_hash)
        if nat is not None and nat.h is not None:
            return nat
        m, st = self.model, self.settings
        plant_hdr, net_hdr = self.generated_header, ampc.generated_header
        pair_hash = build.ampc_loop_pair_hash(self.model_hash, ampc.model_hash)
        emu = self._ampc_loop_lib
        nat = _native.Native("plant", _bind, lambda *_: build.ampc_loop_code_object(plant_hdr, net_hdr, pair_hash),
                             (lambda *_: emu(plant_hdr, net_hdr, pair_hash)) if emu is not None else None, "" if emu is not None else None)
        code_object = nat.load(plant_hdr, self.model_hash)
        d = PlantDesc(nx=m.n_x, nu=m.n_u, np=m.n_p, ntvp=m.n_tvp, nw=m.n_w, nv=m.n_v, ny=m.n_y,
                      discrete=1 if m.model_type == "discrete" else 0, code_object_path=code_object.encode(),
                      model_hash=self.model_hash.encode(), device=st.gpu_index, max_steps=st.max_steps, t_step=float(st.t_step),
                      reltol=float(st.reltol), abstol=float(st.abstol))
        nat.create(d)
        methods = {"cvodes": 0, "idas": 0, "auto": 0, "dopri5": 1, "rk45": 1, "sdirk4": 2, "implicit": 2}
        nat.check(nat.lib.dompc_plant_set_method(nat.h, methods[str(st.integration_tool).lower()], int(st.integration_opts.get("explicit_limit", 0))))
        self._pairs[ampc.model_hash] = nat
        return nat

    def rollout_ampc_device(self, ampc, B, K, X_traj, U_traj, U_prev0=0, W_traj=0, V_traj=0, Y_traj=0, Z_traj=0, tvp_rows=0, p_rows=0,
                            p_loops=0, plant_status=0, clip_to_bounds=True, reseed_z=False, stream=0):
        """K control steps approximate MPC -> plant of B loops in ONE launch (`dompc_plant_ampc_loop_device`, csrc/dompc_ampc_loop.hip):
        per step k the network step of `ampc.make_step_batch_device` at X_traj[k] - with an rterm also on the inputs applied before,
        U_prev0 [B][nu] at k = 0 and U_traj[k - 1] afterwards - writes U_traj[k], then the plant step of `step_batch_device` goes from
        X_traj[k] to X_traj[k + 1]; bit for bit the K pairs of launches.  Raw device addresses, asynchronous on `stream`; the
        parameters, noise, records and status are those of `rollout_device`.  The code object of the pair (this plant, the network's
        shape) is built or loaded on first use and kept; the network's CURRENT weights are used (they are data, as in
        `make_step_batch_device`).  The Newton starts of a plant with algebraic states are those of `step_batch_device`: the two paths
        can be mixed; reseed_z: they start from `simulator.z0`."""
        assert self.flags["setup"], "Simulator is not setup. Call simulator.setup() first."
        m = self.model
        who = "dompc_plant: dompc_plant_ampc_loop_device: "
        n_in, n_out = int(ampc.net.n_in), int(ampc.mpc.model.n_u)
        # (the sizes are compile-time facts of the pair's code object: what the entry point refuses is refused before one is built)
        if n_out != m.n_u:
            raise RuntimeError(who + "the network's n_out differs from the plant's nu")
        if n_in not in (m.n_x, m.n_x + m.n_u):
            raise RuntimeError(who + "the network's n_in is neither the plant's nx nor nx + nu")
        if int(B) <= 0 or int(K) <= 0:
            return
        nat = self._pair(ampc)
        r = AmpcLoopDesc()
        r.w, r.par = ampc.device_weights()
        for name, v in ampc.shape_fields().items():
            setattr(r, name, v)
        r.clip = 1 if clip_to_bounds else 0
        for name, a in (("U_prev0", U_prev0), ("X_traj", X_traj), ("U_traj", U_traj), ("W_traj", W_traj), ("V_traj", V_traj),
                        ("Y_traj", Y_traj), ("Z_traj", Z_traj), ("tvp_rows", tvp_rows), ("p_rows", p_rows), ("p_loops", p_loops),
                        ("plant_status", plant_status)):
            setattr(r, name, int(a) if a else None)
        if m.n_z and nat is not self._native:
            z = C.c_void_p()
            self._check(self._lib.dompc_plant_z_guess_device(self._h, int(B), 1 if reseed_z else 0, C.byref(z)))
            r.z_guess = z.value
        r.reseed_z = 1 if reseed_z else 0
        nat.check(nat.lib.dompc_plant_ampc_loop_device(nat.h, int(B), int(K), C.byref(r), C.c_void_p(int(stream) if stream else None)))

    def simulate_batch(self, X0, U, W=None, V=None, P=None, carry_z: bool = False) -> dict:
        """Open-loop simulation of B plants over K control steps in one launch (`rollout_device`).  X0: [B][nx]; U: [K][B][nu], or
        [K][nu] shared by the batch; W, V: process and measurement noise, likewise (None: none); P: [B][np], one parameter row per plant,
        constant over the steps (default: p_fun at the K times t0 + k t_step, shared by the batch); `_tvp`: tvp_fun at those times.
        Returns {'x' [K + 1][B][nx] (with the start), 'y' [K][B][ny], 'z' [K][B][nz], 'status', 'n_steps' [K][B]} (status bits as
        `make_step_batch`).  Like `make_step_batch` it does not touch x0, t0 or data.  DAE plants: the Newton iteration of every plant
        starts from `simulator.z0` - unless `carry_z`, which says that row b continues the trajectory of row b of the previous call."""
        assert self.flags["setup"], "Simulator is not setup. Call simulator.setup() first."
        import torch
        m = self.model
        X0 = np.ascontiguousarray(np.asarray(X0, dtype=np.float64)).reshape(-1, m.n_x)
        B = X0.shape[0]
        K = int(np.asarray(U).shape[0])

        def rows(a, n, name):
            """[K][B][n] from [K][B][n] or [K][n]"""
            a = np.asarray(a, dtype=np.float64)
            if a.shape == (K, n):
                a = np.broadcast_to(a[:, None, :], (K, B, n))
            if a.shape != (K, B, n):
                raise ValueError(f"Simulator.simulate_batch: {name} must have the shape ({K}, {B}, {n}) or ({K}, {n}), got {a.shape}")
            return np.ascontiguousarray(a)

        # (the host emulation of the tests: "device" memory is host memory)
        dev = torch.device("cpu") if self._native._lib_path is not None else torch.device("cuda", self.settings.gpu_index)
        t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)      # noqa: E731
        e = lambda *shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)      # noqa: E731
        t0, dt = float(self._t0[0]), float(self.settings.t_step)
        ts = [t0 + k * dt for k in range(K)]
        Ut = t(rows(U, m.n_u, "U"))
        Wt = t(rows(W, m.n_w, "W")) if W is not None and m.n_w else None
        Vt = t(rows(V, m.n_v, "V")) if V is not None and m.n_v else None
        tv = t(np.array([_flat_struct(self.tvp_fun(s), m.n_tvp) for s in ts])) if m.n_tvp else None
        p_rows = p_loops = None
        if m.n_p and P is not None:
            P = np.ascontiguousarray(np.asarray(P, dtype=np.float64))
            if P.shape != (B, m.n_p):
                raise ValueError(f"Simulator.simulate_batch: P must have the shape ({B}, {m.n_p}), got {P.shape}")
            p_loops = t(P)
        elif m.n_p:
            p_rows = t(np.array([_flat_struct(self.p_fun(s), m.n_p) for s in ts]))
        Xt, Yt, st = e(K + 1, B, m.n_x), e(K, B, max(m.n_y, 1)), e(K, B, dt=torch.int32)
        Zt = e(K, B, m.n_z) if m.n_z else None
        Xt[0].copy_(t(X0))
        ptr = lambda a: a.data_ptr() if a is not None else 0      # noqa: E731
        stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0
        self.rollout_device(B, K, ptr(Xt), ptr(Ut), W_traj=ptr(Wt), V_traj=ptr(Vt), Y_traj=ptr(Yt) if m.n_y else 0, Z_traj=ptr(Zt),
                            tvp_rows=ptr(tv), p_rows=ptr(p_rows), p_loops=ptr(p_loops), plant_status=ptr(st), reseed_z=not carry_z,
                            stream=stream)
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        status = st.cpu().numpy()
        return {"x": Xt.cpu().numpy(), "y": Yt.cpu().numpy()[:, :, :m.n_y], "z": Zt.cpu().numpy() if Zt is not None else np.zeros((K, B, 0)),
                "status": status & 0xFF, "n_steps": status >> 8}

    def make_step(self, u0=None, v0=None, w0=None) -> np.ndarray:
        """One closed-loop sample (simulator.py:757-850): integrates x0 over t_step with u0 and the current p / tvp,
        stores the new state in x0 and returns the measurement y_next as a column vector."""
        assert self.flags["setup"], "Simulator is not setup. Call simulator.setup() first."
        m = self.model
        if u0 is None:
            assert m.n_u == 0, "No input u0 provided. Please provide an input u0."
            u0 = np.zeros((0, 1))
        u0 = np.asarray(u0.master if hasattr(u0, "master") else u0, dtype=float)
        assert u0.size == m.n_u, "u0 has incorrect shape. You have: {}, expected: {}".format(u0.shape, (m.n_u, 1))
        t0 = float(self._t0[0])
        p0 = _flat_struct(self.p_fun(t0), m.n_p)
        tvp0 = _flat_struct(self.tvp_fun(t0), m.n_tvp)
        r = self.make_step_batch(self._x0.master[None, :], U=u0.reshape(-1), P=p0, TVP=tvp0,
                                 W=None if w0 is None else np.asarray(w0, float).reshape(-1),
                                 V=None if v0 is None else np.asarray(v0, float).reshape(-1), carry_z=True)       # (one trajectory)
        if int(r["status"][0]) & 1:          # bit 0: failure; bit 1 only says that the implicit SDIRK method produced the result
            raise RuntimeError("plant integration did not reach t_step (step limit or NaN right-hand side)")
        # records of the step: state BEFORE the step, the inputs and parameters it used, the new measurement (simulator.py:833-841)
        z0 = self._host_z(self._x0.master, u0.reshape(-1), tvp0, p0)      # (records only: the kernel solves for z itself)
        aux0 = m._aux_expression_fun.eval(self._x0.master, u0.reshape(-1), z0, tvp0, p0)[0]
        self.data.update(_x=self._x0.master.copy(), _u=u0.reshape(-1), _z=z0, _tvp=tvp0, _p=p0, _y=r["y"][0],
                         _aux=np.asarray(aux0, float).reshape(-1), _time=self._t0.copy())
        self._x0.master[:] = r["x"][0]
        self._u0.master[:] = u0.reshape(-1)
        self._t0 = self._t0 + self.settings.t_step
        self.flags["first_step"] = False
        return r["y"][0].reshape(-1, 1)
