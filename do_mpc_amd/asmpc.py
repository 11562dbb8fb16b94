"""Sensitivity-based MPC for B loops: solve and differentiate every `resolve_every`-th step, in between continue the optimal input to
first order in the state - on the device.

The controller is the class ASMPC of the reference's examples/batch_reactor_differentiator
(its examples/batch_reactor_differentiator/main.py:87-177):

    u = (I - G)^-1 (u0 + J (x - x_prev) - G u0),      J = du0/dx0, G = du0/du_prev at the last solution (main.py:170-172).

Since (I - G)^-1 (u0 - G u0) = u0 this is the affine state feedback u = u0 + M (x - x_prev), M = (I - G)^-1 J.  `solve` runs
`MPC.make_step_batch` and `DoMPCDifferentiator.differentiate_batch` and hands their result to the law preparation of
csrc/dompc_asmpc.hip, which forms M for every loop (Gauss-Jordan with partial pivoting on a row of 16 lanes); `make_step_batch` is one
launch of the law step, u = sat(u_ref + M (x - x_ref)).  The law record lives on the device; `Simulator.rollout_affine_device` reads it
to run K control steps law -> plant in one launch (closed_loop.BatchClosedLoopASMPC).

Flags of the law [B]: bit 0 - the member's solve or sensitivities failed, or J / G is not finite; bit 1 - I - G is singular.  Either
gives M = 0: the law holds u0, the input a plain MPC loop would have applied.  Status of a step [B]: bits 0 and 1 copied from the flags,
bit 2 - an input was clipped to `mpc.bounds[..., '_u']`, bit 3 - max |x - x_ref| / x_scaling > settings.max_dx, bit 4 (value 16; set
by the loops in the status they record, never by the law step) - the member was re-solved by an event at this step.

Event-triggered re-solves (settings.event_triggered, off by default).  Bit 3 alone only flags.  With the setting a member whose step
status carries a bit of settings.event_mask - far from its expansion point, or holding u0 after a failed solve - is solved again at
once, alone or with the other members flagged at that step: `select_device` lists them on the device (an ordered compaction),
`solve_members_device` gathers their rows, solves and differentiates the sub-batch and `update_law_device` writes their columns of
the resident law record; the other columns are not touched.  `make_step` and closed_loop.BatchClosedLoopASMPC.step act on it.

There is no CPU fallback: without a HIP device the calls raise.  Limits of the kernels: n_x <= 64, n_u <= 16; larger models are refused
by name, and so is everything `make_step_batch(..., sensitivities=True)` refuses.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native, build, lowering
from .differentiator import DoMPCDifferentiator


SELECT_SPAN = 1024                       # loops per workgroup of `select_device` (csrc/dompc_asmpc_args.h)


@dataclass
class ASMPCSettings:
    resolve_every: int = 1               # solve and differentiate on every resolve_every-th step (make_step, BatchClosedLoopASMPC)
    clip_to_bounds: bool = True          # clip the inputs to mpc.bounds[..., '_u'] (physical units; infinite bounds never clip)
    max_dx: float = float("inf")         # infinity norm of (x - x_ref) / x_scaling beyond which a step is flagged (status bit 3)
    active_set_reduction: bool = False   # handed to the differentiator
    event_triggered: bool = False        # a member whose step status carries a bit of event_mask is solved again in the same step
    event_mask: int = 8 | 1 | 2          # "far" (bit 3) and the two fallback bits: such a member holds u0, an MPC loop would solve it again


class AffineLaw(C.Structure):
    """dompc_affine_law of include/dompc_ipm.h"""
    _fields_ = [(n, C.c_void_p) for n in ("x_ref", "u_ref", "M", "flags", "lb", "ub", "x_scale")] + \
               [("ld", C.c_int64), ("max_dx", C.c_double), ("clip", C.c_int32), ("pad", C.c_int32)]


class ASMPCDesc(C.Structure):
    _fields_ = [("nx", C.c_int32), ("nu", C.c_int32), ("code_object_path", C.c_char_p), ("model_hash", C.c_char_p), ("device", C.c_int32)]


def _bind(lib_path: str) -> C.CDLL:
    lib = C.CDLL(lib_path)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    lib.dompc_asmpc_create.argtypes = [C.POINTER(ASMPCDesc), C.POINTER(vp)]
    lib.dompc_asmpc_destroy.argtypes = [vp]
    lib.dompc_asmpc_destroy.restype = None
    lib.dompc_asmpc_last_error.argtypes = [vp]
    lib.dompc_asmpc_last_error.restype = C.c_char_p
    lib.dompc_asmpc_set_options.argtypes = [vp, vp, vp, vp, i32, C.c_double]
    lib.dompc_asmpc_prepare_device.argtypes = [vp, i32, vp, vp, vp, i64, i64, vp, i64, i64, vp, vp]
    lib.dompc_asmpc_set_law.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    lib.dompc_asmpc_get_law.argtypes = [vp, vp, vp, vp, vp]
    lib.dompc_asmpc_law_batch.argtypes = [vp]
    lib.dompc_asmpc_law_batch.restype = i32
    lib.dompc_asmpc_law.argtypes = [vp, C.POINTER(AffineLaw)]
    lib.dompc_asmpc_step_batch.argtypes = [vp, i32, vp, vp, vp]
    lib.dompc_asmpc_step_batch_device.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.dompc_asmpc_step_law_device.argtypes = [vp, C.POINTER(AffineLaw), i32, vp, vp, vp, vp]
    lib.dompc_asmpc_step_law_device.restype = C.c_int
    lib.dompc_asmpc_select_device.argtypes = [vp, i32, vp, i32, vp, vp, vp]
    lib.dompc_asmpc_update_device.argtypes = [vp, i32, vp, vp, vp, vp, i64, i64, vp, i64, i64, vp, vp]
    lib.dompc_asmpc_update_law.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    for name in ("create", "set_options", "prepare_device", "set_law", "get_law", "law", "step_batch", "step_batch_device", "select_device",
                 "update_device", "update_law"):
        getattr(lib, "dompc_asmpc_" + name).restype = C.c_int
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class LawStep:
    """The law-step kernel of the (n_x, n_u) law object on a record of the caller's: u = sat(u_ref + M (x - x_ref)) for B loops in one
    launch (`dompc_asmpc_step_law_device`), without an MPC behind it - closed_loop.BatchClosedLoopTVLQR steps its time-varying law with it.
    TEST-ONLY: `_lib_path` (a path, or a callable (header, hash) -> path) selects the host emulation of the kernels."""

    def __init__(self, n_x: int, n_u: int, device: int = 0, _lib_path=None):
        self.generated_header = lowering.lower_asmpc(n_x, n_u)
        self.model_hash = self.generated_header.rsplit('ASMPC_MODEL_HASH "', 1)[1].split('"')[0]
        self._native = _native.Native("asmpc", _bind, build.asmpc_code_object, _lib_path, "" if _lib_path is not None else None)
        code_object = self._native.load(self.generated_header, self.model_hash)
        self._native.create(ASMPCDesc(nx=n_x, nu=n_u, code_object_path=code_object.encode(), model_hash=self.model_hash.encode(), device=int(device)))

    def step_device(self, law: AffineLaw, B, X_ptr, U_ptr, status_ptr=0, stream=0) -> None:
        """raw device addresses, asynchronous on `stream`"""
        vp = lambda a: C.c_void_p(int(a) if a else None)      # noqa: E731
        self._native.check(self._native.lib.dompc_asmpc_step_law_device(self._native.h, C.byref(law), int(B), vp(X_ptr), vp(U_ptr),
                                                                        vp(status_ptr), vp(stream)))

    def close(self):
        self._native.close()


class ASMPC:
    def __init__(self, mpc, _lib_path=None, _code_object=None):
        """TEST-ONLY: `_lib_path` (a path, or a callable (header, hash) -> path) with `_code_object=""` selects the host emulation of
        the kernels."""
        assert mpc.flags["setup"] is True, "MPC was not setup yet. Please call MPC.setup()."
        self.mpc = mpc
        self.settings = ASMPCSettings()
        m = mpc.model
        if getattr(mpc, "structure", None) is not None:                    # (a stand-in that carries sizes and bounds only: set_law and the law step)
            DoMPCDifferentiator(mpc)                                       # refuses what make_step_batch(..., sensitivities=True) refuses
        self.generated_header = lowering.lower_asmpc(m.n_x, m.n_u)         # refuses n_x > 64 and n_u > 16, by name
        self.model_hash = self.generated_header.rsplit('ASMPC_MODEL_HASH "', 1)[1].split('"')[0]
        self._native = _native.Native("asmpc", _bind, build.asmpc_code_object, _lib_path, _code_object)
        self._options = None             # what the handle's bounds, scaling, clip and max_dx were set from
        self._nd = None                  # (solver, active_set_reduction, differentiator)
        self._resident = {}              # device -> the solver's bounds and the input scaling as tensors (solve_device)
        self._keep = None                # inputs of an asynchronous law preparation
        self._keep_update = None         # ... and of an asynchronous update of some of its columns
        self._work = None                # compact tensors of solve_members_device
        self.last = None                 # result of the last solve()
        self._k = 0                      # make_step: calls so far
        self._u_data = [np.asarray(mpc.u0.master, dtype=float).reshape(-1, 1).copy()]

    # ------------------------------------------------------------------ native side
    _lib = property(lambda self: self._native.lib)     # the bound library and the native handle (None before first use / after close)
    _h = property(lambda self: self._native.h)

    def _handle(self):
        """the runtime handle (created on first use) with the CURRENT options: bounds, scaling, clip and max_dx are uploaded again
        when one of them changed since the last call"""
        m, st = self.mpc.model, self.settings
        if self._h is None:
            code_object = self._native.load(self.generated_header, self.model_hash)
            desc = ASMPCDesc(nx=m.n_x, nu=m.n_u, code_object_path=code_object.encode(), model_hash=self.model_hash.encode(),
                             device=int(self.mpc.settings.gpu_index))
            self._native.create(desc)
        if int(st.resolve_every) < 1:
            raise ValueError("ASMPC.settings.resolve_every must be an integer >= 1")
        lb, ub, xs = (np.ascontiguousarray(v.master, dtype=np.float64).reshape(-1) for v in (self.mpc._u_lb, self.mpc._u_ub, self.mpc._x_scaling))
        key = (bool(st.clip_to_bounds), float(st.max_dx), lb.tobytes(), ub.tobytes(), xs.tobytes())
        if key != self._options:
            self._check(self._lib.dompc_asmpc_set_options(self._h, _ptr(lb), _ptr(ub), _ptr(xs), 1 if st.clip_to_bounds else 0, float(st.max_dx)))
            self._options = key
        return self._h

    def _check(self, rc):
        self._native.check(rc)

    def close(self):
        self._native.close()
        self._options = None

    def _differentiator(self):
        red = bool(self.settings.active_set_reduction)
        if self._nd is None or self._nd[0] is not self.mpc.S or self._nd[1] != red:
            self._nd = (self.mpc.S, red, DoMPCDifferentiator(self.mpc, active_set_reduction=red))
        return self._nd[2]

    # ------------------------------------------------------------------ solve: the expansion point and the law
    def solve(self, X0, U_prev=None) -> dict:
        """B cold solves at the states X0 [B][n_x] with their sensitivities (`MPC.make_step_batch(..., sensitivities=True)`; with
        settings.active_set_reduction the differentiator runs with it), then the law preparation on the device.  Returns the solve's
        result; it is the expansion point of `make_step_batch` from now on."""
        if self.settings.active_set_reduction:
            r = self.mpc.make_step_batch(X0, U_prev=U_prev)
            r.update(self._differentiator().differentiate_batch(r))
        else:
            r = self.mpc.make_step_batch(X0, U_prev=U_prev, sensitivities=True)
        self.set_law(r["p"][:, :self.mpc.model.n_x], r["u0"], r["du0dx0"], r["du0du_prev"], r["ok"])
        self.last = r
        return r

    def solve_device(self, guess, P, sol, lam_g, f, stats) -> dict:
        """`solve` on tensors that live where the solver runs (torch, float64; `stats`: uint8, B dompc_stats records): guess and sol
        [B][n_opt_x], P [B][n_opt_p] (the states in its first n_x columns, u_prev in its last n_u), lam_g [B][n_g], f [B].  Chains
        `solve_batch_device` -> `differentiate_batch_device` -> law preparation on the current stream; nothing is copied to the host.
        Returns the tensors u0 [B][n_u] (physical units) and what differentiate_batch_device returns."""
        ps = self.mpc.structure
        h = self._handle()
        B = int(P.shape[0])
        out, x_prev, u0, ok, stream = self._solve_and_differentiate(B, guess, P, sol, lam_g, f, stats)
        nx, nu = ps.nx, ps.nu
        S = out["dxdp"]                                                 # [B][n_u][n_x + n_u]: J and G are views into it
        assert S.is_contiguous() and tuple(S.shape) == (B, nu, nx + nu)
        self._check(self._lib.dompc_asmpc_prepare_device(h, B, x_prev.data_ptr(), u0.data_ptr(), S.data_ptr(), nx + nu, nu * (nx + nu),
                                                         S.data_ptr() + 8 * nx, nx + nu, nu * (nx + nu), ok.data_ptr(),
                                                         C.c_void_p(int(stream) if stream else None)))
        self._keep = (x_prev, u0, ok, out)                              # (the launch is asynchronous: its inputs stay alive)
        out = dict(out)
        out["u0"] = u0
        return out

    def _solve_and_differentiate(self, B, guess, P, sol, lam_g, f, stats):
        """`solve_batch_device` -> `differentiate_batch_device` for the B rows of the tensors; returns what the law preparation reads:
        (result of the differentiator, x_prev [B][n_x], u0 [B][n_u] in physical units, ok [B] int32, the stream)"""
        import torch
        mpc, ps = self.mpc, self.mpc.structure
        dev = P.device
        if str(dev) not in self._resident:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)      # noqa: E731
            self._resident[str(dev)] = dict(lbx=up(mpc._lb_opt_x.master), ubx=up(mpc._ub_opt_x.master), lbg=up(mpc._nlp_cons_lb),
                                            ubg=up(mpc._nlp_cons_ub), us=up(mpc._u_scaling.master))
        r = self._resident[str(dev)]
        stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0
        mpc.S.solve_batch_device(B, guess.data_ptr(), r["lbx"].data_ptr(), r["ubx"].data_ptr(), r["lbg"].data_ptr(), r["ubg"].data_ptr(),
                                 P.data_ptr(), sol.data_ptr(), 0, 0, lam_g.data_ptr(), f.data_ptr(), stats.data_ptr(), stream=stream)
        out = self._differentiator().differentiate_batch_device(sol, lam_g, stats, P)
        nx, nu, iu = ps.nx, ps.nu, ps.iu(0, 0)
        u0 = torch.mul(sol[:, iu:iu + nu], r["us"])                     # u0 in physical units
        x_prev = P[:, :nx].contiguous()
        ok = out["ok"].to(torch.int32)
        return out, x_prev, u0, ok, stream

    # ------------------------------------------------------------------ event-triggered re-solves of some members
    def select_device(self, B, status_ptr, idx_ptr, count_ptr, stream=0) -> None:
        """the members whose step status carries a bit of settings.event_mask, on raw device addresses: status [B] (int32, what
        `make_step_batch_device` wrote) -> idx [B] (int32: those members in ascending order; entries beyond count are not written) and
        count [1] (int32); asynchronous on `stream`"""
        h = self._handle()
        self._check(self._lib.dompc_asmpc_select_device(h, int(B), C.c_void_p(int(status_ptr)), int(self.settings.event_mask),
                                                        C.c_void_p(int(idx_ptr)), C.c_void_p(int(count_ptr)),
                                                        C.c_void_p(int(stream) if stream else None)))

    def update_law_device(self, n, slot, x_prev, u0, S, ok) -> None:
        """the law preparation for n compact entries into the columns slot[:n] (int32 tensor, distinct members of the current law) of the
        resident law record; the other columns are not touched.  Tensors where the law lives: x_prev [n][n_x], u0 [n][n_u], S [n][n_u]
        [n_x + n_u] (the differentiator's dxdp: J and G are views into it, as in `solve_device`), ok [n] (int32).  Asynchronous on the
        current stream."""
        import torch
        ps = self.mpc.structure
        h = self._handle()
        n = int(n)
        if n == 0:
            return
        nx, nu = ps.nx, ps.nu
        dev = S.device
        stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0
        assert slot.dtype == torch.int32 and ok.dtype == torch.int32 and slot.is_contiguous() and x_prev.is_contiguous() and u0.is_contiguous()
        assert S.is_contiguous() and tuple(S.shape[1:]) == (nu, nx + nu) and min(int(t.shape[0]) for t in (slot, x_prev, u0, S, ok)) >= n
        self._check(self._lib.dompc_asmpc_update_device(h, n, slot.data_ptr(), x_prev.data_ptr(), u0.data_ptr(), S.data_ptr(), nx + nu,
                                                        nu * (nx + nu), S.data_ptr() + 8 * nx, nx + nu, nu * (nx + nu), ok.data_ptr(),
                                                        C.c_void_p(int(stream) if stream else None)))
        self._keep_update = (slot, x_prev, u0, S, ok)                   # (the launch is asynchronous: its inputs stay alive)

    def set_law_members(self, idx, x_prev, u0, du0dx0, du0du_prev, ok=None) -> None:
        """`set_law` for the members idx [n] of the current law only, from host arrays with n entries each: their columns of the law
        record are replaced, the others are not touched.  idx must be distinct and inside the current law (ValueError otherwise, before
        anything is launched)."""
        m = self.mpc.model
        h = self._handle()
        idx = np.asarray(idx).reshape(-1)
        if idx.size and not np.issubdtype(idx.dtype, np.integer):
            raise ValueError("ASMPC.set_law_members: idx must be integers")
        idx = idx.astype(np.int64)
        B, n = self.batch, idx.size
        if B <= 0:
            raise RuntimeError("ASMPC.set_law_members: no law to update (call solve or set_law first)")
        if n and (idx.min() < 0 or idx.max() >= B):
            raise ValueError(f"ASMPC.set_law_members: idx must lie in [0, {B}), the members of the current law")
        if np.unique(idx).size != n:
            raise ValueError("ASMPC.set_law_members: idx must be distinct")
        f = lambda a, *shape: np.ascontiguousarray(np.asarray(a, dtype=np.float64)).reshape(-1, *shape)      # noqa: E731
        x_prev, u0, J, G = f(x_prev, m.n_x), f(u0, m.n_u), f(du0dx0, m.n_u, m.n_x), f(du0du_prev, m.n_u, m.n_u)
        if not (x_prev.shape[0] == u0.shape[0] == J.shape[0] == G.shape[0] == n):
            raise ValueError("ASMPC.set_law_members: idx, x_prev, u0, du0dx0 and du0du_prev must have the same number of members")
        if n == 0:
            return
        okv = None if ok is None else np.ascontiguousarray(np.asarray(ok).reshape(n) != 0, dtype=np.int32)
        slot = np.ascontiguousarray(idx, dtype=np.int32)
        self._check(self._lib.dompc_asmpc_update_law(h, n, _ptr(slot), _ptr(x_prev), _ptr(u0), _ptr(J), _ptr(G), _ptr(okv)))

    def solve_members_device(self, idx, n, guess, P, sol, lam_g, f, stats) -> dict:
        """`solve_device` for the members idx[:n] (int32 tensor, distinct, ascending as `select_device` writes them) of the resident
        tensors of B loops: their rows of guess and P are gathered into compact tensors (allocated once, for B rows), the sub-batch
        is solved and differentiated, the law preparation writes the members' columns of the resident law record, and sol, lam_g, f
        and the stats records go back to the rows idx[:n].  The other rows and columns are not touched.  Everything on the current
        stream; `n` is a host integer.  Returns the compact u0 [n][n_u] and what differentiate_batch_device returns.
        The solver's launch shape follows n: the bits of a member's solution are those of a solve of a batch of n."""
        import torch
        from .solver import STATS_DTYPE
        ps = self.mpc.structure
        n, B = int(n), int(P.shape[0])
        if not 0 < n <= B:
            raise ValueError(f"ASMPC.solve_members_device: n = {n} members of a batch of {B}")
        if self.batch != B:
            raise RuntimeError(f"ASMPC.solve_members_device: the law holds {self.batch} loops, the tensors {B}")
        dev, item = P.device, STATS_DTYPE.itemsize
        w = self._work
        if w is None or w["B"] != B or w["dev"] != dev:
            e = lambda *shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)      # noqa: E731
            w = self._work = dict(B=B, dev=dev, guess=e(B, ps.n_opt_x), P=e(B, ps.n_opt_p), sol=e(B, ps.n_opt_x), lam_g=e(B, ps.n_g),
                                  f=e(B), stats=torch.zeros(B * item, dtype=torch.uint8, device=dev))
        ix = idx[:n].to(torch.int64)
        c = {k: w[k][:n] for k in ("guess", "P", "sol", "lam_g", "f")}
        c["stats"] = w["stats"][:n * item]
        torch.index_select(guess, 0, ix, out=c["guess"])
        torch.index_select(P, 0, ix, out=c["P"])
        out, x_prev, u0, ok, _ = self._solve_and_differentiate(n, c["guess"], c["P"], c["sol"], c["lam_g"], c["f"], c["stats"])
        self.update_law_device(n, idx[:n].contiguous(), x_prev, u0, out["dxdp"], ok)
        sol.index_copy_(0, ix, c["sol"])
        lam_g.index_copy_(0, ix, c["lam_g"])
        f.index_copy_(0, ix, c["f"])
        stats.view(B, item).index_copy_(0, ix, c["stats"].view(n, item))
        out = dict(out)
        out["u0"] = u0
        return out

    def set_law(self, x_prev, u0, du0dx0, du0du_prev, ok=None) -> None:
        """The law from given host arrays: x_prev [B][n_x], u0 [B][n_u], du0dx0 [B][n_u][n_x], du0du_prev [B][n_u][n_u], ok [B] (default:
        all True) - e.g. sensitivities stored by `AMPCSampler`."""
        m = self.mpc.model
        h = self._handle()
        f = lambda a, *shape: np.ascontiguousarray(np.asarray(a, dtype=np.float64)).reshape(-1, *shape)      # noqa: E731
        x_prev, u0, J, G = f(x_prev, m.n_x), f(u0, m.n_u), f(du0dx0, m.n_u, m.n_x), f(du0du_prev, m.n_u, m.n_u)
        B = x_prev.shape[0]
        if not (u0.shape[0] == J.shape[0] == G.shape[0] == B):
            raise ValueError("ASMPC.set_law: x_prev, u0, du0dx0 and du0du_prev must have the same number of members")
        okv = None if ok is None else np.ascontiguousarray(np.asarray(ok).reshape(B) != 0, dtype=np.int32)
        self._check(self._lib.dompc_asmpc_set_law(h, B, _ptr(x_prev), _ptr(u0), _ptr(J), _ptr(G), _ptr(okv)))

    @property
    def batch(self) -> int:
        """loops of the current law (0: none yet)"""
        return int(self._lib.dompc_asmpc_law_batch(self._h)) if self._h is not None else 0

    @property
    def law(self) -> dict:
        """the law record copied to the host: x_ref [B][n_x], u_ref [B][n_u], M [B][n_u][n_x], flags [B]"""
        B = self.batch
        if B <= 0:
            raise RuntimeError("ASMPC.law: no solution to expand about (call solve or set_law first)")
        m = self.mpc.model
        out = {"x_ref": np.empty((B, m.n_x)), "u_ref": np.empty((B, m.n_u)), "M": np.empty((B, m.n_u, m.n_x)), "flags": np.zeros(B, dtype=np.int32)}
        self._check(self._lib.dompc_asmpc_get_law(self._h, *[_ptr(out[k]) for k in ("x_ref", "u_ref", "M", "flags")]))
        return out

    def law_record(self) -> AffineLaw:
        """the device-side record (dompc_affine_law) for `Simulator.rollout_affine_device`; valid until the next solve / set_law"""
        self._handle()
        rec = AffineLaw()
        self._check(self._lib.dompc_asmpc_law(self._h, C.byref(rec)))
        return rec

    # ------------------------------------------------------------------ the law step
    def make_step_batch(self, X):
        """inputs U [B][n_u] for the states X [B][n_x] from the last solve, and the status [B] (bits: module docstring)"""
        h = self._handle()
        if self.batch <= 0:
            raise RuntimeError("ASMPC.make_step_batch: no solution to expand about (call solve or set_law first)")
        m = self.mpc.model
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float64)).reshape(-1, m.n_x)
        B = X.shape[0]
        U = np.empty((B, m.n_u))
        status = np.zeros(B, dtype=np.int32)
        self._check(self._lib.dompc_asmpc_step_batch(h, B, _ptr(X), _ptr(U), _ptr(status)))
        return U, status

    def make_step_batch_device(self, B, X_ptr, U_ptr, status_ptr=0, stream=0) -> None:
        """make_step_batch on raw device addresses (ints, e.g. torch tensor .data_ptr()) of X [B][n_x] and U [B][n_u] (float64) and
        status [B] (int32, or 0); asynchronous on `stream`"""
        h = self._handle()
        self._check(self._lib.dompc_asmpc_step_batch_device(h, int(B), C.c_void_p(int(X_ptr)), C.c_void_p(int(U_ptr)),
                                                            C.c_void_p(int(status_ptr) if status_ptr else None),
                                                            C.c_void_p(int(stream) if stream else None)))

    # ------------------------------------------------------------------ one loop, the reference class's surface
    def make_step(self, x0):
        """One loop with the reference class's semantics: on every settings.resolve_every-th call (the first included) the controller
        is solved at x0 - `mpc.make_step`, warm start and u_prev as in a plain MPC loop - and differentiated; otherwise the input is
        the continuation from the last solve.  With settings.event_triggered a call whose continuation reports a bit of
        settings.event_mask (x0 farther than max_dx from the last solve's state, or a fallback law) solves at this x0 in the same call,
        as if it were due; the period goes on counting calls.  Returns the input as a column; `u_data` records every one."""
        mpc, m = self.mpc, self.mpc.model
        x0 = np.asarray(x0, dtype=float).reshape(-1, 1)
        due = self._k % int(self.settings.resolve_every) == 0
        if due:
            self._solve_one(x0)
        u, st = self.make_step_batch(x0.reshape(1, -1))
        if not due:
            if self.settings.event_triggered and int(st[0]) & int(self.settings.event_mask):
                self._solve_one(x0)                               # the event: solved at this x0 in the same call, as if it were due
                u, st = self.make_step_batch(x0.reshape(1, -1))
            else:
                mpc._t0 = mpc._t0 + mpc.settings.t_step           # (a control step without a solve: the controller's clock moves on)
        self._k += 1
        u = u.reshape(-1, 1)
        mpc._u0.master[:] = u.ravel()                             # u_prev of the next solve: the input that was applied
        self._u_data.append(u.copy())
        return u

    def _solve_one(self, x0):
        """make_step's solve at x0: `mpc.make_step`, the sensitivities and the law of the one loop"""
        mpc, m = self.mpc, self.mpc.model
        u0 = mpc.make_step(x0)
        if not mpc.solver_stats.get("success", False):
            self.set_law(x0.ravel(), u0.ravel(), np.zeros((1, m.n_u, m.n_x)), np.zeros((1, m.n_u, m.n_u)), [False])
        else:
            nd = self._differentiator()
            r = {"x": mpc.opt_x_num.master[None, :].copy(), "lam_g": np.asarray(mpc.lam_g_num, float).reshape(1, -1).copy(),
                 "p": mpc.opt_p_num.master[None, :].copy(), "stats": self._stats_row()}
            s = nd.differentiate_batch(r)
            self.set_law(x0.ravel(), u0.ravel(), s["du0dx0"], s["du0du_prev"], s["ok"])

    def _stats_row(self):
        from .solver import STATS_DTYPE
        st = np.zeros(1, dtype=STATS_DTYPE)
        s = self.mpc.solver_stats
        st["success"], st["mu"], st["obj_scaling"] = 1, float(s["mu"]), float(s.get("obj_scaling", 1.0))
        return st

    @property
    def u_data(self) -> np.ndarray:
        """the inputs computed so far, one column each, after the controller's initial u0 (the reference's `u_data`)"""
        return np.hstack(self._u_data)
