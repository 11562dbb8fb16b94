"""Batched closed loops with the whole batch resident in device memory.

The reference closes the loop one sample at a time on the host - `u0 = mpc.make_step(x0)`, `y = simulator.make_step(u0)`,
`x0 = estimator.make_step(y)` (/root/reference/examples/industrial_poly/main.py:105-108) - and fans batches of such loops
out over processes (`do_mpc.sampling.Sampler`, /root/reference/do_mpc/sampling/_sampler.py:198-228).  Here B loops
advance together: one launch per controller, plant and estimator and control step, all on the same stream; states, inputs,
parameters and the warm-start solution stay in device memory (torch tensors are only the allocator).

The parts, each written once, and the seven loops composed of them:

  _Device          the torch device of a loop, host array -> device tensor (always a copy), its stream and its synchronisation
  _PlantSide       the plant: states, status, its `_p` / `_tvp` at the loop time, the batched step, optionally measurement and noise
  _ControllerSide  the MPC problem of B loops: `opt_p` rows, warm start, bounds, solution, statistics, its `_tvp` / `_p` at the loop
                   time, the batched solve and the bookkeeping of the next problem
  _record_run      n steps of a state-feedback loop collected into records

  BatchClosedLoop       _ControllerSide -> _PlantSide, state feedback
  BatchClosedLoopMHE    _ControllerSide -> _PlantSide (measuring) -> moving horizon estimator (its chain problem lives in the class)
  BatchClosedLoopEKF    _ControllerSide -> _PlantSide (measuring, noise) -> extended Kalman filter (its buffers live in the class)
  BatchClosedLoopLQR    gain (a torch expression) -> _PlantSide; run = _record_run, or fused: the gain as the law of the plant rollout
  BatchClosedLoopTVLQR  time-varying gains along a reference (LQR.gains_along_device) -> the plant rollout with a law record per step
  BatchClosedLoopAMPC   network kernel -> _PlantSide; run = _record_run, or fused: network and plant alternate inside one launch
  BatchClosedLoopASMPC  _ControllerSide (solved through ASMPC.solve_device, with multipliers) -> affine law -> _PlantSide; events, rollout

The reference's per-sample loop re-evaluates tvp_fun / p_fun at the current time in EVERY make_step of controller, plant and
estimator (_mpc.py:1009-1019, simulator.py:790-800, _mhe.py:940-950, _ekf.py:268-270) - a set-point staircase over the horizon moves
along.  Every part therefore keeps the start time and the step of ITS object and refreshes at `t0 + k * dt` from k = 1 on (the
values at k = 0 are uploaded at construction); the values are the same for every loop of the batch.
"""
from __future__ import annotations

import numpy as np

from .solver import STATS_DTYPE


class _Device:
    """device: index of a HIP device, or "cpu" where the loop serves a controller and a plant on the host emulation"""

    def __init__(self, device, host_ok: bool = False):
        import torch
        self.torch = torch
        if device == "cpu" and not host_ok:
            raise NotImplementedError('structured HIP backend: this closed loop has no host flavour (device="cpu")')
        self.dev = torch.device("cpu") if device == "cpu" else torch.device("cuda", device)

    def to_dev(self, a):
        """host array -> float64 tensor; a copy, also on the host (`from_numpy(...).to("cpu")` would alias the array)"""
        return self.torch.tensor(np.asarray(a, dtype=np.float64), device=self.dev)

    def empty(self, *shape):
        return self.torch.empty(shape, dtype=self.torch.float64, device=self.dev)

    def zeros(self, *shape, dtype=None):
        return self.torch.zeros(shape, dtype=dtype or self.torch.float64, device=self.dev)

    def stream(self):
        return self.torch.cuda.current_stream(self.dev).cuda_stream if self.dev.type == "cuda" else 0

    def sync(self):
        if self.dev.type == "cuda":
            self.torch.cuda.synchronize(self.dev)


def _stats_host(stats):
    """the solver statistics of a batch (uint8 device buffer) as a numpy record array"""
    return np.frombuffer(stats.cpu().numpy().tobytes(), dtype=STATS_DTYPE).copy()


class _PlantSide:
    """The plant of B loops.  X0: [B][nx].  measure: keep the measurements Y [B][max(ny, 1)] of every step; without it the loop is
    state feedback (`StateFeedback.make_step` returns y, estimator/_base.py:63-72) and the plant's measurement must be its state.
    noise: keep a buffer V [B][nv] that the loop fills and every step reads as measurement noise."""

    def __init__(self, simulator, dv: _Device, X0, measure: bool = False, noise: bool = False):
        m = simulator.model
        assert measure or m.n_y == m.n_x, "state feedback: the plant's measurement must be its state"
        self.sim, self.dv = simulator, dv
        self.X = dv.to_dev(X0)
        self.B = int(self.X.shape[0])
        self.Xn = dv.torch.empty_like(self.X)
        self.pstat = dv.zeros(self.B, dtype=dv.torch.int32)
        self.Y = dv.empty(self.B, max(m.n_y, 1)) if measure else None
        self.V = dv.zeros(self.B, m.n_v) if noise and m.n_v else None
        self.t0, self.dt = float(simulator._t0[0]), float(simulator.settings.t_step)
        tv, pp = self.rows(0, 1)
        self.tvp, self.p = dv.to_dev(tv[0]), dv.to_dev(pp[0])

    def rows(self, k: int, K: int):
        """the plant's _tvp / _p at the K loop times from step k on: [K][n] each (one zero per row without such parameters)"""
        m = self.sim.model
        ts = [self.t0 + (k + j) * self.dt for j in range(K)]
        # (a copy per row: a tvp_fun / p_fun usually fills and returns one template)
        tv = np.array([np.array(self.sim.tvp_fun(s).master, dtype=float).reshape(-1) for s in ts]) if m.n_tvp else np.zeros((K, 1))
        pp = np.array([np.array(self.sim.p_fun(s).master, dtype=float).reshape(-1) for s in ts]) if m.n_p else np.zeros((K, 1))
        return tv, pp

    def refresh(self, k: int) -> None:
        """_tvp / _p at the loop time of step k -> device"""
        m = self.sim.model
        if k > 0 and (m.n_p or m.n_tvp):
            tv, pp = self.rows(k, 1)
            if m.n_p:
                self.p.copy_(self.dv.to_dev(pp[0]))
            if m.n_tvp:
                self.tvp.copy_(self.dv.to_dev(tv[0]))

    def step(self, U, stream, shared_mask: int = 2 | 4 | 8 | 16, W=None, P=None) -> None:
        """one plant step of all loops with the inputs U [B][nu]; X is the new state afterwards.  shared_mask: _tvp and _p are one row
        for the batch (bits 1, 2), and so are the noise inputs (bits 3, 4) unless the loop clears their bits.  W: [B][nw] process
        noise of this step, one row per loop (bit 3 is cleared for it), or None.  P: [B][np], the plant's `_p` per loop in place of
        the row of p_fun (bit 2 is cleared for it), or None"""
        if W is not None:
            shared_mask &= ~8
        if P is not None:
            shared_mask &= ~4
        self.sim.step_batch_device(self.B, self.X.data_ptr(), U.data_ptr(), self.tvp.data_ptr(),
                                   (self.p if P is None else P).data_ptr(), self.Xn.data_ptr(),
                                   self.Y.data_ptr() if self.Y is not None else 0, self.pstat.data_ptr(),
                                   w=W.data_ptr() if W is not None else 0,
                                   v=self.V.data_ptr() if self.V is not None else 0, shared_mask=shared_mask, stream=stream)
        self.X, self.Xn = self.Xn, self.X

    def status(self):
        """(status, implicit) of the last step per loop: bit 0 and bit 1 of the plant's status word"""
        s = self.pstat.cpu().numpy()
        return s & 1, (s >> 1) & 1


class _ControllerSide:
    """The MPC problem of B loops.  x0: [B][nx], the states the first solve starts from; U_prev0: [B][nu] or None (0).  lam_g: keep a
    buffer for the constraint multipliers (the ASMPC loop, whose solve is `ASMPC.solve_device` on these tensors)."""

    def __init__(self, mpc, dv: _Device, x0, U_prev0=None, lam_g: bool = False):
        ps = self.ps = mpc.structure
        if getattr(ps, "open_loop_stack", False):
            raise NotImplementedError("structured HIP backend: the device-resident closed loop with open_loop and several scenarios "
                                      "(the controller's vectors live in the stacked chain layout there; use make_step_batch)")
        if getattr(mpc.S, "row_mapped", False):
            raise NotImplementedError("structured HIP backend: the device-resident closed loop with rows appended to nlp_cons (internal row "
                                      "layout, solver.RowMappedSolver); use make_step_batch")
        self.mpc, self.dv = mpc, dv
        self.B = B = x0.shape[0]
        self.t0, self.dt = float(mpc._t0[0]), float(mpc.settings.t_step)
        P = np.tile(mpc.opt_p_num.master, (B, 1))
        P[:, :ps.nx] = x0
        P[:, ps.p_off_tvp:ps.p_off_p] = mpc.tvp_fun(self.t0).master
        P[:, ps.p_off_p:ps.p_off_uprev] = mpc.p_fun(self.t0).master
        P[:, ps.p_off_uprev:] = 0.0 if U_prev0 is None else np.asarray(U_prev0, float).reshape(B, ps.nu)
        Xi = np.zeros((B, ps.n_opt_x))                         # initial guess = set_initial_guess semantics (mpc.x0 = x0, mpc.u0 = u_prev)
        Xi[:, :ps.off_z].reshape(B, -1, ps.nx)[:] = (x0 / mpc._x_scaling.master)[:, None, :]
        Xi[:, ps.off_u:ps.off_eps].reshape(B, -1, ps.nu)[:] = (P[:, ps.p_off_uprev:] / mpc._u_scaling.master)[:, None, :]
        self.P, self.guess = dv.to_dev(P), dv.to_dev(Xi)
        self.bounds = [dv.to_dev(v) for v in (mpc._lb_opt_x.master, mpc._ub_opt_x.master, mpc._nlp_cons_lb, mpc._nlp_cons_ub)]
        self.us = dv.to_dev(mpc._u_scaling.master)
        self.sol, self.f = dv.empty(B, ps.n_opt_x), dv.empty(B)
        self.lam_g = dv.empty(B, ps.n_g) if lam_g else None
        self.stats = dv.zeros(B * STATS_DTYPE.itemsize, dtype=dv.torch.uint8)
        self._p_row = P[0].copy()                              # host image of one opt_p row (its _tvp / _p blocks are re-uploaded)

    def refresh(self, k: int) -> None:
        """_tvp / _p at the loop time of step k -> their block of every opt_p row"""
        ps = self.ps
        if k > 0 and (ps.ntvp or ps.np_):
            tm = self.t0 + k * self.dt
            row = self._p_row
            row[ps.p_off_tvp:ps.p_off_p] = self.mpc.tvp_fun(tm).master
            row[ps.p_off_p:ps.p_off_uprev] = self.mpc.p_fun(tm).master
            self.P[:, ps.p_off_tvp:ps.p_off_uprev] = self.dv.to_dev(row[ps.p_off_tvp:ps.p_off_uprev])

    def solve(self, stream) -> None:
        lbx, ubx, lbg, ubg = self.bounds
        self.mpc.S.solve_batch_device(self.B, self.guess.data_ptr(), lbx.data_ptr(), ubx.data_ptr(), lbg.data_ptr(), ubg.data_ptr(),
                                      self.P.data_ptr(), self.sol.data_ptr(), 0, 0, 0, self.f.data_ptr(), self.stats.data_ptr(),
                                      stream=stream)

    def u0(self, out) -> None:
        """the first input of the solution in physical units -> out [B][nu]"""
        ps = self.ps
        iu = ps.iu(0, 0)
        self.dv.torch.mul(self.sol[:, iu:iu + ps.nu], self.us, out=out)

    def set_x0(self, x, U) -> None:
        """the parameters of a solve at the states x after the inputs U: x0 <- x, u_prev <- U"""
        self.P[:, :self.ps.nx] = x
        self.P[:, self.ps.p_off_uprev:] = U

    def next_problem(self, x, U) -> None:
        """x0 <- state or estimate, u_prev <- applied input, initial guess <- previous solution (unshifted, optimizer.py:754-768)"""
        self.set_x0(x, U)
        self.guess.copy_(self.sol)

    def stats_host(self):
        return _stats_host(self.stats)


def _record_run(loop, n: int) -> dict:
    """n control steps of a state-feedback loop; returns the records 'x' [n + 1][B][nx] (with the start), 'u' [n][B][nu] and the plant
    status of every step"""
    xs, us, st = [loop.plant.X.cpu().numpy().copy()], [], []
    for _ in range(int(n)):
        r = loop.step()
        xs.append(r["x"].copy())
        us.append(r["u0"].copy())
        st.append(r["plant_status"])
    return {"x": np.stack(xs), "u": np.stack(us) if us else np.zeros((0, loop.B, loop.plant.sim.model.n_u)),
            "plant_status": np.stack(st) if st else np.zeros((0, loop.B), dtype=np.int32)}


class BatchClosedLoop:
    """B closed loops controller -> plant with state feedback: per control step ONE `dompc_solve_batch_device` launch (structured IPM, B
    problems) and ONE `dompc_plant_step_batch_device` launch (plant integrator, B samples) on the same stream.
    X0: [B][nx]; U_prev0: [B][nu], the inputs before the first step (default 0)."""

    def __init__(self, mpc, simulator, X0, device: int = 0, U_prev0=None):
        self.mpc, self.sim = mpc, simulator
        ps = self.ps = mpc.structure
        dv = self.dv = _Device(device)
        X0 = np.asarray(X0, dtype=float).reshape(-1, ps.nx)
        self.B = B = X0.shape[0]
        self.ctrl = _ControllerSide(mpc, dv, X0, U_prev0)
        m = simulator.model
        assert m.n_x == ps.nx and m.n_u == ps.nu, "controller and plant must share states and inputs"
        self.plant = _PlantSide(simulator, dv, X0)
        self.U = dv.empty(B, ps.nu)
        self.k = 0

    def step(self) -> dict:
        """one control step of all B loops; returns the solver statistics (numpy record array) and the plant status"""
        ctrl, plant, stream = self.ctrl, self.plant, self.dv.stream()
        ctrl.refresh(self.k)
        plant.refresh(self.k)
        ctrl.solve(stream)
        ctrl.u0(out=self.U)
        plant.step(self.U, stream)
        ctrl.next_problem(plant.X, self.U)
        self.k += 1
        self.dv.sync()
        status, implicit = plant.status()
        return {"stats": ctrl.stats_host(), "plant_status": status, "plant_implicit": implicit, "u0": self.U.cpu().numpy(),
                "x": plant.X.cpu().numpy()}


class BatchClosedLoopMHE:
    """B closed loops controller -> plant -> moving horizon estimator -> controller advancing together, everything resident in HBM
    (the loop of examples/rotating_oscillating_masses_mhe_mpc/main.py, one sample at a time on the host there): per control step
    ONE batched solve of the controller (B problems), ONE batched plant step (states and measurements), ONE batched solve of the
    estimator (B estimation problems), plus index arithmetic on device tensors - the estimator's parameter vectors (previous
    estimates, sliding measurement window) and initial guesses are assembled from the previous device results.
    The controller's and the estimator's problems live in their chain layouts (do_mpc_amd/estimator.py); torch is the allocator
    and does the slicing."""

    def __init__(self, mpc, simulator, mhe, X0_true, x0_est=None, p_est0=None, device: int = 0):
        self.mpc, self.sim, self.mhe = mpc, simulator, mhe
        m = simulator.model
        ps, es = self.ps, self.es = mpc.structure, mhe._ps  # controller / estimator chain structures
        dv = self.dv = _Device(device)
        t = dv.to_dev
        X0_true = np.asarray(X0_true, dtype=float).reshape(-1, m.n_x)
        self.B = B = X0_true.shape[0]
        nx, npe = self.nx, self.npe = m.n_x, mhe.n_p_est
        x_est = np.zeros((B, nx)) if x0_est is None else np.broadcast_to(np.asarray(x0_est, float).reshape(-1, nx), (B, nx)).copy()
        p_est = np.zeros((B, npe)) if p_est0 is None else np.broadcast_to(np.asarray(p_est0, float).reshape(-1, npe), (B, npe)).copy()
        self.ctrl = _ControllerSide(mpc, dv, x_est)
        self.plant = _PlantSide(simulator, dv, X0_true, measure=True)
        self.U = dv.empty(B, m.n_u)
        # ---- estimator: chain opt_p rows (previous estimate | (tvp_k, y_k) per stage | p_set | 0), initial guess, bounds
        N = self.N = mhe.settings.n_horizon
        te = float(mhe._t0[0])
        op = np.zeros((B, mhe.n_opt_p))
        op[:, :nx] = x_est
        op[:, nx:nx + npe] = p_est
        op[:, mhe._po_pset:mhe._po_tvp] = mhe.p_fun(te).master
        op[:, mhe._po_tvp:mhe._po_y] = mhe.tvp_fun(te).master
        ge = np.zeros((B, mhe.n_opt_x))
        ge[:, :mhe._o_z].reshape(B, -1, nx)[:] = (x_est / mhe._x_scaling.master)[:, None, :]
        pes = mhe._p_est_scaling.master if npe else np.zeros(0)
        ge[:, mhe._o_p:] = p_est / pes if npe else p_est      # (opt_x holds the SCALED parameter, _mhe.py:939-941 / set_initial_guess)
        self.Pe, self.Ge = t(mhe._p_to_chain(op)), t(mhe._to_chain(ge))
        em = mhe._mpc
        self.e_lbx, self.e_ubx = t(em._lb_opt_x.master), t(em._ub_opt_x.master)
        self.e_lbg, self.e_ubg = t(em._nlp_cons_lb), t(em._nlp_cons_ub)
        self.e_sol, self.e_f = dv.empty(B, es.n_opt_x), dv.empty(B)
        self.e_stats = dv.zeros(B * STATS_DTYPE.itemsize, dtype=dv.torch.uint8)
        self.x_est, self.p_est = t(x_est), t(p_est)
        self.exs = t(mhe._x_scaling.master)
        self.eps_ = t(pes if npe else np.zeros(1))              # scaling of the estimated parameters (they ride as scaled states of the chain problem)
        self.t_mhe0, self.dt_mhe = te, float(mhe.settings.t_step)
        self.k = 0

    def _refresh_estimator(self):
        """_tvp / _p of the estimator at the current loop time -> device (same values for every sample); only the measurement columns
        of the estimator's window are data of the loop"""
        es, mhe, up = self.es, self.mhe, self.dv.to_dev
        te = self.t_mhe0 + self.k * self.dt_mhe
        mt = mhe.model.n_tvp
        if self.k > 0 and (mt or mhe.n_p_set):
            op = np.zeros((1, mhe.n_opt_p))
            op[:, mhe._po_pset:mhe._po_tvp] = mhe.p_fun(te).master
            op[:, mhe._po_tvp:mhe._po_y] = mhe.tvp_fun(te).master
            pc = mhe._p_to_chain(op)[0]
            if mt:
                tv = pc[es.p_off_tvp:es.p_off_p].reshape(self.N + 1, es.ntvp)[:, :mt]
                self.Pe[:, es.p_off_tvp:es.p_off_p].view(self.B, self.N + 1, es.ntvp)[:, :, :mt] = up(tv)
            if es.p_off_uprev > es.p_off_p:
                self.Pe[:, es.p_off_p:es.p_off_uprev] = up(pc[es.p_off_p:es.p_off_uprev])

    def step(self) -> dict:
        ctrl, plant, es, B, nx, npe, N = self.ctrl, self.plant, self.es, self.B, self.nx, self.npe, self.N
        stream = self.dv.stream()
        mt = self.mhe.model.n_tvp
        ctrl.refresh(self.k)
        plant.refresh(self.k)
        self._refresh_estimator()
        # 1. controller
        ctrl.solve(stream)
        ctrl.u0(out=self.U)
        # 2. plant: next true state and its measurement
        plant.step(self.U, stream)
        # 3. estimator: previous estimates <- `_x[1, -1]`, `_p_est` of ITS previous solution (initial guess before the first solve,
        #    _mhe.py:939-941), measurement window shifted by one stage, the new measurement last
        i1 = es.ix(1, 0, es.M)
        self.Pe[:, :nx] = self.Ge[:, i1:i1 + nx] * self.exs
        self.Pe[:, nx:nx + npe] = self.p_est
        TV = self.Pe[:, es.p_off_tvp:es.p_off_p].view(B, N + 1, es.ntvp)
        TV[:, :N - 1, mt:] = TV[:, 1:N, mt:].clone()
        TV[:, N - 1, mt:] = plant.Y
        self.mhe.S.solve_batch_device(B, self.Ge.data_ptr(), self.e_lbx.data_ptr(), self.e_ubx.data_ptr(), self.e_lbg.data_ptr(),
                                      self.e_ubg.data_ptr(), self.Pe.data_ptr(), self.e_sol.data_ptr(), 0, 0, 0, self.e_f.data_ptr(),
                                      self.e_stats.data_ptr(), stream=stream)
        iN = es.ix(N, 0, es.M)
        self.x_est = self.e_sol[:, iN:iN + nx] * self.exs
        i0 = es.ix(0, 0, es.M)
        # (physical units: the chain problem carries the parameter as a SCALED state; `_p_est_prev` of the arrival cost and the
        #  returned estimate are physical, _mhe.py: opt_x_num['_p_est'] * _p_est_scaling - ADVICE r3)
        self.p_est = self.e_sol[:, i0 + nx:i0 + nx + npe] * self.eps_[:npe] if npe else self.e_sol[:, i0 + nx:i0 + nx].clone()
        self.Ge.copy_(self.e_sol)                                  # warm start (unshifted, optimizer.py:754-768)
        # 4. next controller problem, from the estimate
        ctrl.next_problem(self.x_est, self.U)
        self.k += 1
        self.dv.sync()
        status, implicit = plant.status()
        return {"mpc_stats": ctrl.stats_host(), "mhe_stats": _stats_host(self.e_stats), "plant_status": status, "plant_implicit": implicit,
                "u0": self.U.cpu().numpy(), "x_true": plant.X.cpu().numpy(), "y": plant.Y.cpu().numpy(), "x_est": self.x_est.cpu().numpy(),
                "p_est": self.p_est.cpu().numpy()}


class BatchClosedLoopEKF:
    """B closed loops controller -> plant -> extended Kalman filter -> controller advancing together, everything resident in HBM: per
    control step ONE batched solve of the controller, ONE batched plant step (states and measurements) and ONE batched filter step
    (do_mpc_amd/ekf.py: estimates and covariances updated in place), plus index arithmetic on device tensors.  The per-sample loop of
    the reference is `u0 = mpc.make_step(x0)`, `y = simulator.make_step(u0)`, `x0 = ekf.make_step(y, u0, Q, R)`
    (/root/reference/examples/triple_tank_ekf/main.py:191-200 for the plant and the filter).
    X0_true: [B][nx] plant states; x0_est: [nx] or [B][nx]; P0: [nx][nx] or [B][nx][nx]; Q, R: one matrix or one per loop;
    V: measurement noise of the plant, None, [B][nv] (the same in every step) or a callable k -> [B][nv].
    A filter of a model with algebraic states (ekf.settings.dae_reduction) keeps a resident [B][nz] buffer: `ekf.z0` for every loop at
    the start, then the algebraic states of each step's last Newton solve as the guess of the next; step() returns it as `z_est`."""

    def __init__(self, mpc, simulator, ekf, X0_true, x0_est, P0, Q, R, V=None, device: int = 0):
        self.mpc, self.sim, self.ekf = mpc, simulator, ekf
        m, me = simulator.model, ekf.model
        ps = self.ps = mpc.structure
        dv = self.dv = _Device(device)
        t = dv.to_dev
        X0_true = np.asarray(X0_true, dtype=float).reshape(-1, m.n_x)
        self.B = B = X0_true.shape[0]
        nx, ny = m.n_x, m.n_y
        x_est = np.broadcast_to(np.asarray(x0_est, float).reshape(-1, nx), (B, nx)).copy()
        self.ctrl = _ControllerSide(mpc, dv, x_est)
        assert m.n_x == ps.nx and m.n_u == ps.nu, "controller and plant must share states and inputs"
        assert (me.n_x, me.n_u, me.n_y) == (m.n_x, m.n_u, m.n_y), "plant and filter must share states, inputs and measurements"
        P0 = np.asarray(P0, float)
        Pcov = np.broadcast_to(P0.reshape(-1, nx, nx), (B, nx, nx)).copy()
        Q, R = np.asarray(Q, float), np.asarray(R, float)
        assert Q.shape in ((nx, nx), (B, nx, nx)) and R.shape in ((ny, ny), (B, ny, ny)), "Q / R: one matrix or one per loop"
        self.mask = 2 | 4 | (8 if Q.ndim == 2 else 0) | (16 if R.ndim == 2 else 0)
        self.Q, self.R = t(Q), t(R)
        self._V = V
        self.plant = _PlantSide(simulator, dv, X0_true, measure=True, noise=V is not None)
        self.U = dv.empty(B, m.n_u)
        # ---- filter
        te = float(ekf._t0[0])
        self.x_est, self.Pcov = t(x_est), t(Pcov)
        self.p_ekf = t(ekf.p_fun(te).master if me.n_p else np.zeros(1))
        self.tvp_ekf = t(ekf.tvp_fun(te).master if me.n_tvp else np.zeros(1))
        self.estat = dv.zeros(B, dtype=dv.torch.int32)
        self.nz = me.n_z
        if self.nz:
            self.z_est = t(np.tile(ekf.z0.master, (B, 1)))
            self.enewton = dv.zeros(B, dtype=dv.torch.int32)
        self.t_ekf0, self.dt_ekf = te, float(ekf.settings.t_step)
        self.k = 0

    def _refresh_filter(self):
        """_tvp / _p of the filter at the current loop time -> device (same values for every loop)"""
        me = self.ekf.model
        te = self.t_ekf0 + self.k * self.dt_ekf
        if self.k > 0 and me.n_p:
            self.p_ekf.copy_(self.dv.to_dev(self.ekf.p_fun(te).master))
        if self.k > 0 and me.n_tvp:
            self.tvp_ekf.copy_(self.dv.to_dev(self.ekf.tvp_fun(te).master))

    def step(self) -> dict:
        ctrl, plant, B = self.ctrl, self.plant, self.B
        stream = self.dv.stream()
        ctrl.refresh(self.k)
        plant.refresh(self.k)
        self._refresh_filter()
        if plant.V is not None:
            v = self._V(self.k) if callable(self._V) else self._V
            plant.V.copy_(self.dv.to_dev(np.asarray(v, float).reshape(plant.V.shape)))
        # 1. controller
        ctrl.solve(stream)
        ctrl.u0(out=self.U)
        # 2. plant: next true state and its measurement (noise per loop)
        plant.step(self.U, stream, shared_mask=2 | 4 | 8)
        # 3. filter: estimate and covariance in place
        self.ekf.step_batch_device(B, self.x_est.data_ptr(), self.Pcov.data_ptr(), plant.Y.data_ptr(), self.U.data_ptr(),
                                   self.tvp_ekf.data_ptr(), self.p_ekf.data_ptr(), self.Q.data_ptr(), self.R.data_ptr(),
                                   status=self.estat.data_ptr(), shared_mask=self.mask, stream=stream,
                                   **({"z": self.z_est.data_ptr(), "newton": self.enewton.data_ptr()} if self.nz else {}))
        # 4. next controller problem, from the estimate
        ctrl.next_problem(self.x_est, self.U)
        self.k += 1
        self.dv.sync()
        out = {"mpc_stats": ctrl.stats_host(), "plant_status": plant.status()[0], "ekf_status": self.estat.cpu().numpy() & 0xFF,
               "u0": self.U.cpu().numpy(), "x_true": plant.X.cpu().numpy(), "y": plant.Y[:, :self.sim.model.n_y].cpu().numpy(),
               "x_est": self.x_est.cpu().numpy(), "P": self.Pcov.cpu().numpy()}
        if self.nz:
            out["z_est"], out["ekf_newton"] = self.z_est.cpu().numpy(), self.enewton.cpu().numpy()
        return out


class BatchClosedLoopLQR:
    """B closed loops LQR -> plant advancing together with the states resident in device memory: per control step the gain
    u = K (x - xss) + uss (+ u_prev in inputRatePenalization mode: LQR.make_step_batch, a torch expression) and ONE batched plant step.
    The per-sample loop of the reference is `u0 = lqr.make_step(x0)`, `x0 = simulator.make_step(u0)`
    (/root/reference/examples/lqr_examples/CSTR_lqr/main.py:75-78).  State feedback: the plant's measurement must be its state.
    X0: [B][nx]; K: None (lqr.K for every loop) or [B][nu][n], e.g. the schedule of LQR.gains_at; XSS / USS: None (the set-point of
    set_setpoint), one set-point or one per loop, of the model's size; U_prev0: [B][nu] (default 0, like lqr.u0 after reset).
    `run(n, fused=True)` runs the steps inside the general plant rollout instead, the gain as its law: one launch per chunk of steps.
    device: index of the HIP device, or "cpu" with a controller and a plant on the host emulation (tests)."""

    def __init__(self, lqr, simulator, X0, K=None, XSS=None, USS=None, device=0, U_prev0=None):
        self.lqr, self.sim = lqr, simulator
        assert lqr.flags["setup"] is True, "LQR is not setup. run setup() function."
        m = simulator.model
        ml = lqr.model
        assert (m.n_x, m.n_u) == (ml.n_x, ml.n_u), "controller and plant must share states and inputs"
        X0 = np.asarray(X0, dtype=float).reshape(-1, m.n_x)
        self.B = B = X0.shape[0]
        dv = self.dv = _Device(device, host_ok=True)
        t = dv.to_dev
        self.plant = _PlantSide(simulator, dv, X0)
        rate = lqr.mode == "inputRatePenalization"
        if XSS is None and USS is None and hasattr(lqr, "xss"):
            xs = np.asarray(lqr.xss, float).ravel()
            XSS, USS = xs[:m.n_x], (xs[m.n_x:] if rate else np.asarray(lqr.uss, float).ravel())
        self.xss = t(np.zeros((1, m.n_x)) if XSS is None else np.asarray(XSS, float).reshape(-1, m.n_x))
        self.uss = t(np.zeros((1, m.n_u)) if USS is None else np.asarray(USS, float).reshape(-1, m.n_u))
        self.K = t(np.asarray(lqr.K if K is None else K, float).reshape(-1, m.n_u, lqr.n_design))
        assert self.K.shape[0] in (1, B) and self.xss.shape[0] in (1, B) and self.uss.shape[0] in (1, B), "one gain / set-point or one per loop"
        self.U = t(np.zeros((B, m.n_u)) if U_prev0 is None else np.asarray(U_prev0, float).reshape(B, m.n_u))
        self.k = 0

    def _noise(self, w):
        """process noise of one step or of several, host array or tensor -> device tensor [...][B][nw] (None stays None)"""
        if w is None:
            return None
        nw = self.sim.model.n_w
        assert nw > 0, "process noise for a plant whose model has none (set_rhs(..., process_noise=True))"
        w = w if type(w).__module__.startswith("torch") else self.dv.to_dev(w)
        return w.to(self.dv.dev).reshape(-1, self.B, nw).contiguous()

    def step(self, w=None) -> dict:
        """one control step of all B loops; returns the inputs applied, the new states and the plant status.  w: [B][nw], the process
        noise of this step (default: none)"""
        plant = self.plant
        plant.refresh(self.k)
        w = self._noise(w)
        self.U = self.lqr.make_step_batch(plant.X, K=self.K, XSS=self.xss, USS=self.uss, U_prev=self.U).contiguous()
        plant.step(self.U, self.dv.stream(), W=None if w is None else w[0])
        self.k += 1
        self.dv.sync()
        return {"u0": self.U.cpu().numpy(), "x": plant.X.cpu().numpy(), "plant_status": plant.status()[0]}

    def _law(self):
        """The loop's gain as a law of the general plant rollout, formed once: (record, G, up_ref, tensors that own the memory).  A
        shared gain or set-point is expanded to the batch (ld = B); x_scale = 1, max_dx = inf, no clip.  Standard mode: x_ref = xss,
        u_ref = uss, M = K.  inputRatePenalization mode, u = u_prev + Kx (x - xss) + Ku (u_prev - uss) with K = [Kx Ku]: x_ref = xss,
        u_ref = up_ref = uss, M = Kx, G = I + Ku."""
        if getattr(self, "_law_rec", None) is None:
            from .asmpc import AffineLaw
            torch, B, m = self.dv.torch, self.B, self.sim.model
            nx, nu = m.n_x, m.n_u
            K = self.K.expand(B, nu, self.K.shape[2])
            keep = {"x_ref": self.xss.expand(B, nx).t().contiguous(), "u_ref": self.uss.expand(B, nu).t().contiguous(),
                    "M": K[:, :, :nx].permute(1, 2, 0).contiguous(), "x_scale": self.dv.to_dev(np.ones(nx))}
            G = None
            if self.lqr.mode == "inputRatePenalization":
                eye = torch.eye(nu, dtype=torch.float64, device=self.dv.dev)
                G = keep["G"] = (eye[None] + K[:, :, nx:]).permute(1, 2, 0).contiguous()
            rec = AffineLaw(x_ref=keep["x_ref"].data_ptr(), u_ref=keep["u_ref"].data_ptr(), M=keep["M"].data_ptr(), flags=None, lb=None,
                            ub=None, x_scale=keep["x_scale"].data_ptr(), ld=B, max_dx=float("inf"), clip=0, pad=0)
            self._law_rec = (rec, G, keep["u_ref"] if G is not None else None, keep)
        return self._law_rec[:3]

    def _rollout(self, K, W):
        """K control steps in one launch, one synchronisation and one copy to the host; W: [K][B][nw] on the device, or None.
        Returns (x [K][B][nx], u [K][B][nu], plant status [K][B])"""
        dv, plant, m, B = self.dv, self.plant, self.sim.model, self.B
        torch = dv.torch
        nX, nU = (K + 1) * B * m.n_x, K * B * m.n_u
        buf = dv.empty(nX + nU + (K * B + 1) // 2)             # states, inputs and the status words behind one another: one copy
        Xt, Ut = buf[:nX].view(K + 1, B, m.n_x), buf[nX:nX + nU].view(K, B, m.n_u)
        pst = buf[nX + nU:].view(torch.int32)[:K * B].view(K, B)
        tv, pp = (dv.to_dev(a) for a in plant.rows(self.k, K))
        Xt[0].copy_(plant.X)
        law, G, up_ref = self._law()
        self.sim.rollout_device(B, K, Xt.data_ptr(), Ut.data_ptr(), law=law, G=G.data_ptr() if G is not None else 0,
                                up_ref=up_ref.data_ptr() if G is not None else 0, U_prev0=self.U.data_ptr() if G is not None else 0,
                                W_traj=W.data_ptr() if W is not None else 0, tvp_rows=tv.data_ptr() if m.n_tvp else 0,
                                p_rows=pp.data_ptr() if m.n_p else 0, plant_status=pst.data_ptr(), stream=dv.stream())
        plant.X.copy_(Xt[K])
        self.U = Ut[K - 1].clone()
        plant.pstat.copy_(pst[K - 1])
        self.k += K
        dv.sync()
        host = buf.cpu().numpy()
        st = host[nX + nU:].view(np.int32)[:K * B].reshape(K, B)
        return host[B * m.n_x:nX].reshape(K, B, m.n_x), host[nX:nX + nU].reshape(K, B, m.n_u), st & 1

    def run(self, n: int, fused: bool = False, chunk=None, W=None) -> dict:
        """n control steps; returns the records 'x' [n + 1][B][nx] (with the start), 'u' [n][B][nu] and the plant status of every step.
        W: process noise of the plant, [n][B][nw] or a callable k -> [B][nw] (k = 0 .. n - 1: the step of this run).
        fused=True: the steps run as ceil(n / chunk) launches of the general plant rollout (`Simulator.rollout_device`) with the gain as
        its law (`_law`), one synchronisation and one copy to the host after each launch - instead of a handful of launches, a
        synchronisation and three copies per step.  chunk=None: one launch.  Device memory per launch: (chunk + 1) B nx + chunk B nu
        float64 and chunk B int32 for the records, chunk B nw float64 more with noise, chunk rows of the plant's `_tvp` and `_p`.  The
        inputs differ from those of the step-wise path by the order of the additions in K (x - xss) (an fma chain here, a torch
        product there).  `k`, the states and the inputs applied last are left where n calls of step() leave them: the two can be
        mixed.  Plants with algebraic states are served."""
        n = int(n)
        m = self.sim.model
        if W is not None and not callable(W):
            W = self._noise(W)
            assert W.shape[0] == n, f"W must hold the noise of {n} steps"

        def noise(i, K):
            """W of the steps i .. i + K - 1 on the device: [K][B][nw], or None"""
            if W is None:
                return None
            return self._noise(np.stack([np.asarray(W(i + j), float) for j in range(K)])) if callable(W) else W[i:i + K]
        if not fused and W is None:
            return _record_run(self, n)
        xs, us, st = [self.plant.X.cpu().numpy().copy()[None]], [], []
        i = 0
        while i < n:
            if fused:
                K = n - i if chunk is None else min(int(chunk), n - i)
                x, u, s = self._rollout(K, noise(i, K))
            else:
                K = 1
                r = self.step(w=noise(i, 1)[0])
                x, u, s = r["x"].copy()[None], r["u0"].copy()[None], r["plant_status"][None]
            xs.append(x); us.append(u); st.append(s)
            i += K
        cat = lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dtype=dt)      # noqa: E731
        return {"x": np.concatenate(xs), "u": cat(us, (0, self.B, m.n_u), float), "plant_status": cat(st, (0, self.B), np.int32)}


class BatchClosedLoopTVLQR:
    """B closed loops that track a trajectory under the time-varying LQR law u_k = u*_k + K_k (x_k - x*_k), states, reference and gains
    resident in device memory.  X0: [B][nx]; X_ref: [K + 1][B or 1][nx] (only the first K rows are knots), U_ref: [K][B or 1][nu] - e.g. a
    record of `Simulator.simulate_batch`; K_traj: the gains [K][B or 1][nu][nx], or None: `design()` forms them on the resident
    reference (`LQR.gains_along_device` on the plant's model with the controller's weights, the gains written by the kernel in the
    layout of the law record).  `step()` is one control step - two launches: the law step at the step's record (`asmpc.LawStep`), then
    the plant step -, `run()` the steps inside the general plant rollout with a law record per step
    (`Simulator.rollout_device(law_step=)`).  The loop ends at step K: a step past it raises.  Standard mode only.  State
    feedback: the plant's measurement must be its state.  The pairs are formed with the plant's `_tvp` at the K loop times and its `_p`
    at the first one.  device: index of the HIP device, or "cpu" with a controller and a plant on the host emulation (tests; TEST-ONLY
    `_law_lib`: the host-emulation library of the law-step kernel, as `asmpc.LawStep` takes it)."""

    def __init__(self, lqr, simulator, X0, X_ref, U_ref, K_traj=None, device=0, _law_lib=None):
        if lqr.mode == "inputRatePenalization":
            raise NotImplementedError("BatchClosedLoopTVLQR: a controller in inputRatePenalization mode is not served (the time-varying "
                                      "input-rate law is not built); use the standard mode")
        self.lqr, self.sim = lqr, simulator
        m, ml = simulator.model, lqr.model
        assert (m.n_x, m.n_u) == (ml.n_x, ml.n_u), "controller and plant must share states and inputs"
        X0 = np.asarray(X0, dtype=float).reshape(-1, m.n_x)
        self.B = B = X0.shape[0]
        U_ref = np.asarray(U_ref, dtype=float)
        self.K = K = int(U_ref.shape[0])
        if K < 1:
            raise ValueError("BatchClosedLoopTVLQR: U_ref must hold at least one step")
        U_ref = np.ascontiguousarray(np.broadcast_to(U_ref.reshape(K, -1, m.n_u), (K, B, m.n_u)))
        X_ref = np.asarray(X_ref, dtype=float)
        if X_ref.shape[0] != K + 1:
            raise ValueError(f"BatchClosedLoopTVLQR: X_ref must have {K + 1} rows for the {K} rows of U_ref, got {X_ref.shape[0]}")
        X_ref = np.ascontiguousarray(np.broadcast_to(X_ref.reshape(K + 1, -1, m.n_x), (K + 1, B, m.n_x)))
        dv = self.dv = _Device(device, host_ok=True)
        t = dv.to_dev
        self.plant = _PlantSide(simulator, dv, X0)
        self.X_ref, self.U_ref = t(X_ref), t(U_ref)                           # step-major: the knots of the pairs launch
        # the law arrays, loop index fastest: x_ref [K][nx][B], u_ref [K][nu][B], M [K][nu][nx][B], flags [K][B]
        self.x_ref, self.u_ref = self.X_ref[:K].permute(0, 2, 1).contiguous(), self.U_ref.permute(0, 2, 1).contiguous()
        self.M = dv.zeros(K, m.n_u, m.n_x, B)
        self.flags = dv.zeros(K, B, dtype=dv.torch.int32)
        self.x_scale = t(np.ones(m.n_x))
        self.U = dv.zeros(B, m.n_u)
        self.lstat = dv.zeros(B, dtype=dv.torch.int32)
        self._law_lib, self._law_step = _law_lib, None
        self.k = 0
        self.design_status = None
        if K_traj is None:
            self.design()
        else:
            Kt = np.asarray(K_traj, dtype=float)
            Kt = np.broadcast_to(Kt.reshape(K, -1, m.n_u, m.n_x), (K, B, m.n_u, m.n_x))
            self.M.copy_(t(np.ascontiguousarray(Kt.transpose(0, 2, 3, 1))))

    def design(self) -> dict:
        """the gains along the resident reference, two launches and no transposition: pairs, then the recursion writing M.  Returns
        {'status' [B], 'step' [B], 'pair_status' [K][B]} (LQR.gains_along) and keeps it in `design_status`; a trajectory that failed at
        step k replays U_ref up to k."""
        dv, m, B, K, lqr = self.dv, self.sim.model, self.B, self.K, self.lqr
        torch = dv.torch
        Qd, Rd, Pd, mask = lqr._weights(None, None, None, B, finite="tv")
        Q, R, P = dv.to_dev(Qd), dv.to_dev(Rd), dv.to_dev(Pd)
        A, Bm, P0 = dv.empty(K, B, m.n_x, m.n_x), dv.empty(K, B, m.n_x, m.n_u), dv.empty(B, m.n_x, m.n_x)
        st, ps = dv.zeros(B, dtype=torch.int32), dv.zeros(K, B, dtype=torch.int32)
        tv, pp = self.plant.rows(0, K)
        tvp, p = dv.to_dev(tv), dv.to_dev(pp[0])
        z = None
        if m.n_z:
            z0 = np.asarray(self.sim._z0.master, float)            # (the Newton start of the plant)
            z = dv.to_dev(np.ascontiguousarray(np.broadcast_to(z0.reshape(1, 1, m.n_z), (K, B, m.n_z))))
        lqr.gains_along_device(m, B, K, self.X_ref.data_ptr(), self.U_ref.data_ptr(), A.data_ptr(), Bm.data_ptr(), Q.data_ptr(), R.data_ptr(),
                               P.data_ptr(), P0.data_ptr(), tvp=tvp.data_ptr() if m.n_tvp else 0, p=p.data_ptr() if m.n_p else 0,
                               z=z.data_ptr() if z is not None else 0, law_M=self.M.data_ptr(), ld=B, pair_status=ps.data_ptr(),
                               status=st.data_ptr(), shared_mask=mask | 8 | 16, stream=dv.stream())
        dv.sync()
        s = st.cpu().numpy()
        self.design_status = {"status": s & 0xFF, "step": (s >> 8) & 0xFFFF, "pair_status": ps.cpu().numpy() & 0xFF}
        return self.design_status

    _noise = BatchClosedLoopLQR._noise

    def _law(self, k: int):
        """the law record of step k: the arrays advanced by hand (what law_step does inside the rollout)"""
        from .asmpc import AffineLaw
        return AffineLaw(x_ref=self.x_ref[k].data_ptr(), u_ref=self.u_ref[k].data_ptr(), M=self.M[k].data_ptr(), flags=self.flags[k].data_ptr(),
                         lb=None, ub=None, x_scale=self.x_scale.data_ptr(), ld=self.B, max_dx=float("inf"), clip=0, pad=0)

    def _rollout(self, K, W):
        """K control steps from step self.k in one launch of the general rollout with a law record per step, one synchronisation and
        one copy to the host; W: [K][B][nw] on the device, or None.  Returns (x [K][B][nx], u [K][B][nu], plant status [K][B], law
        status [K][B])"""
        dv, plant, m, B = self.dv, self.plant, self.sim.model, self.B
        if self.k + K > self.K:
            raise ValueError(f"BatchClosedLoopTVLQR: step {self.k + K} is past the end of the reference ({self.K} steps)")
        torch = dv.torch
        nX, nU = (K + 1) * B * m.n_x, K * B * m.n_u
        buf = dv.empty(nX + nU + K * B)                        # states, inputs and the two status words behind one another: one copy
        Xt, Ut = buf[:nX].view(K + 1, B, m.n_x), buf[nX:nX + nU].view(K, B, m.n_u)
        stw = buf[nX + nU:].view(torch.int32)[:2 * K * B].view(2, K, B)
        tv, pp = (dv.to_dev(a) for a in plant.rows(self.k, K))
        Xt[0].copy_(plant.X)
        self.sim.rollout_device(B, K, Xt.data_ptr(), Ut.data_ptr(), law=self._law(self.k), W_traj=W.data_ptr() if W is not None else 0,
                                tvp_rows=tv.data_ptr() if m.n_tvp else 0, p_rows=pp.data_ptr() if m.n_p else 0,
                                plant_status=stw[0].data_ptr(), law_status=stw[1].data_ptr(), stream=dv.stream(), law_step=B)
        plant.X.copy_(Xt[K])
        self.U = Ut[K - 1].clone()
        plant.pstat.copy_(stw[0, K - 1])
        self.lstat.copy_(stw[1, K - 1])
        self.k += K
        dv.sync()
        host = buf.cpu().numpy()
        st = host[nX + nU:].view(np.int32)[:2 * K * B].reshape(2, K, B)
        return host[B * m.n_x:nX].reshape(K, B, m.n_x), host[nX:nX + nU].reshape(K, B, m.n_u), st[0] & 1, st[1].copy()

    def step(self, w=None) -> dict:
        """one control step of all B loops, two launches: the law step of dompc_affine.h at the record of step `k` (the arrays advanced
        by hand), then the batched plant step.  w: [B][nw], the process noise of this step"""
        if self.k >= self.K:
            raise ValueError(f"BatchClosedLoopTVLQR: step {self.k + 1} is past the end of the reference ({self.K} steps)")
        plant, m = self.plant, self.sim.model
        if self._law_step is None:
            from .asmpc import LawStep
            self._law_step = LawStep(m.n_x, m.n_u, 0 if self.dv.dev.type == "cpu" else self.dv.dev.index, _lib_path=self._law_lib)
        plant.refresh(self.k)
        w = self._noise(w)
        stream = self.dv.stream()
        self._law_step.step_device(self._law(self.k), self.B, plant.X.data_ptr(), self.U.data_ptr(), self.lstat.data_ptr(), stream)
        plant.step(self.U, stream, W=None if w is None else w[0])
        self.k += 1
        self.dv.sync()
        return {"u0": self.U.cpu().numpy(), "x": plant.X.cpu().numpy(), "plant_status": plant.status()[0], "law_status": self.lstat.cpu().numpy()}

    def run(self, n=None, fused: bool = True, chunk=None, W=None) -> dict:
        """n control steps (default: to the end of the reference); returns the records 'x' [n + 1][B][nx] (with the start), 'u'
        [n][B][nu], 'plant_status' and 'law_status' [n][B].  fused=True: ceil(n / chunk) launches of the rollout with a law record per
        step, one synchronisation and one copy each (chunk=None: one launch); fused=False: n calls of step().  W: process noise,
        [n][B][nw] or a callable k -> [B][nw].  Both leave `k`, the states and the inputs where n calls of step() leave them."""
        n = self.K - self.k if n is None else int(n)
        m = self.sim.model
        if self.k + n > self.K:
            raise ValueError(f"BatchClosedLoopTVLQR: step {self.k + n} is past the end of the reference ({self.K} steps)")
        if W is not None and not callable(W):
            W = self._noise(W)
            assert W.shape[0] == n, f"W must hold the noise of {n} steps"

        def noise(i, K):
            if W is None:
                return None
            return self._noise(np.stack([np.asarray(W(i + j), float) for j in range(K)])) if callable(W) else W[i:i + K]
        xs, us, st, ls = [self.plant.X.cpu().numpy().copy()[None]], [], [], []
        i = 0
        while i < n:
            if fused:
                K = n - i if chunk is None else min(int(chunk), n - i)
                x, u, s, l = self._rollout(K, noise(i, K))
            else:
                K, w = 1, noise(i, 1)
                r = self.step(w=None if w is None else w[0])
                x, u, s, l = r["x"].copy()[None], r["u0"].copy()[None], r["plant_status"][None], r["law_status"][None]
            xs.append(x); us.append(u); st.append(s); ls.append(l)
            i += K
        cat = lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dtype=dt)      # noqa: E731
        return {"x": np.concatenate(xs), "u": cat(us, (0, self.B, m.n_u), float), "plant_status": cat(st, (0, self.B), np.int32),
                "law_status": cat(ls, (0, self.B), np.int32)}


class BatchClosedLoopAMPC:
    """B closed loops approximate MPC -> plant advancing together with X and U resident in device memory (float64): per control step
    TWO launches, the network kernel (ApproxMPC.make_step_batch_device) and ONE batched plant step.  The per-sample loop of the
    reference is `u0 = approx_mpc.make_step(x0)`, `x0 = simulator.make_step(u0)`
    (/root/reference/examples/CSTR_approximate_mpc/main.py:164-170).  State feedback: the network acts on the plant's state.
    X0: [B][nx]; U_prev0: [B][nu], the inputs before the first step (default: ampc.u0 for every loop; read only when the controller
    has an rterm).  device: index of the HIP device, or "cpu" with a controller and a plant on the host emulation (tests).
    `run(n, fused=True)` runs the steps inside the fused loop kernel of the pair (plant, network shape) instead: one launch per chunk
    of steps, with process noise and plant parameters per loop if asked for."""

    def __init__(self, ampc, simulator, X0, U_prev0=None, device=0, clip_to_bounds=True):
        self.ampc, self.sim, self.clip = ampc, simulator, bool(clip_to_bounds)
        assert ampc.flags["setup"] == True, "MPC was not setup yet. Please call ApproxMPC.setup()."      # noqa: E712
        m = simulator.model
        mc = ampc.mpc.model
        assert (m.n_x, m.n_u) == (mc.n_x, mc.n_u), "controller and plant must share states and inputs"
        X0 = np.asarray(X0, dtype=float).reshape(-1, m.n_x)
        self.B = B = X0.shape[0]
        dv = self.dv = _Device(device, host_ok=True)
        # (a plant whose measurement is not its state: the network is a law on the STATE, the loop validates it on the true states; the
        #  step-wise path then keeps the measurement of the last step in plant.Y)
        self.plant = _PlantSide(simulator, dv, X0, measure=m.n_y != m.n_x)
        if U_prev0 is None:
            u0 = ampc.u0
            U_prev0 = np.tile(np.asarray(u0.master if hasattr(u0, "master") else u0, dtype=float).reshape(1, m.n_u), (B, 1))
        self.U = dv.to_dev(np.asarray(U_prev0, float).reshape(B, m.n_u))
        self.Un = dv.torch.empty_like(self.U)
        self.P = None                     # [B][np]: the plant's `_p` per loop (run(P=...)); None: the row of the plant's p_fun
        self.k = 0

    def _noise(self, w):
        """process noise of one step or of several, host array or tensor -> device tensor [...][B][nw] (None stays None)"""
        if w is None:
            return None
        nw = self.sim.model.n_w
        assert nw > 0, "process noise for a plant whose model has none (set_rhs(..., process_noise=True))"
        w = w if type(w).__module__.startswith("torch") else self.dv.to_dev(w)
        return w.to(self.dv.dev).reshape(-1, self.B, nw).contiguous()

    def step(self, w=None) -> dict:
        """one control step of all B loops; returns the inputs applied, the new states and the plant status.  w: [B][nw], the process
        noise of this step (default: none)"""
        plant, stream = self.plant, self.dv.stream()
        plant.refresh(self.k)
        w = self._noise(w)
        self.ampc.make_step_batch_device(self.B, plant.X.data_ptr(), self.U.data_ptr() if self.ampc.rterm else 0, self.Un.data_ptr(),
                                         stream=stream, clip_to_bounds=self.clip)
        self.U, self.Un = self.Un, self.U
        plant.step(self.U, stream, W=None if w is None else w[0], P=self.P)
        self.k += 1
        self.dv.sync()
        return {"u0": self.U.cpu().numpy(), "x": plant.X.cpu().numpy(), "plant_status": plant.status()[0]}

    def _rollout(self, K, W):
        """K control steps in one launch (`Simulator.rollout_ampc_device`), one synchronisation and one copy to the host; W: [K][B][nw]
        on the device, or None.  Returns (x [K + 1][B][nx] with the state the launch started from, u [K][B][nu], plant status [K][B]);
        x and u are views of the one host buffer of the copy - on a GPU page-locked memory, which the copy fills at the bus's rate
        and torch hands out again once the records of an earlier run are dropped"""
        dv, plant, m, B = self.dv, self.plant, self.sim.model, self.B
        torch = dv.torch
        nX, nU = (K + 1) * B * m.n_x, K * B * m.n_u
        buf = dv.empty(nX + nU + (K * B + 1) // 2)             # states, inputs and the status words behind one another: one copy
        Xt, Ut = buf[:nX].view(K + 1, B, m.n_x), buf[nX:nX + nU].view(K, B, m.n_u)
        pst = buf[nX + nU:].view(torch.int32)[:K * B].view(K, B)
        tv, pp = (dv.to_dev(a) for a in plant.rows(self.k, K))
        Xt[0].copy_(plant.X)
        per_loop = self.P is not None
        self.sim.rollout_ampc_device(self.ampc, B, K, Xt.data_ptr(), Ut.data_ptr(), U_prev0=self.U.data_ptr() if self.ampc.rterm else 0,
                                     W_traj=W.data_ptr() if W is not None else 0, tvp_rows=tv.data_ptr() if m.n_tvp else 0,
                                     p_rows=pp.data_ptr() if m.n_p and not per_loop else 0, p_loops=self.P.data_ptr() if per_loop else 0,
                                     plant_status=pst.data_ptr(), clip_to_bounds=self.clip, stream=dv.stream())
        plant.X.copy_(Xt[K])
        self.U.copy_(Ut[K - 1])
        plant.pstat.copy_(pst[K - 1])
        self.k += K
        if dv.dev.type == "cuda":
            host_t = torch.empty(buf.shape, dtype=buf.dtype, pin_memory=True)
            host_t.copy_(buf, non_blocking=True)
        else:
            host_t = buf
        dv.sync()
        host = host_t.numpy()
        st = host[nX + nU:].view(np.int32)[:K * B].reshape(K, B)
        return host[:nX].reshape(K + 1, B, m.n_x), host[nX:nX + nU].reshape(K, B, m.n_u), st & 1

    def run(self, n: int, fused: bool = False, chunk=None, W=None, P=None) -> dict:
        """n control steps; returns the records 'x' [n + 1][B][nx] (with the start), 'u' [n][B][nu] and the plant status of every step.
        W: process noise of the plant, [n][B][nw] or a callable k -> [B][nw] (k = 0 .. n - 1: the step of this run).
        P: [B][np], the plant's `_p` per loop - validation under parametric uncertainty; it replaces the row of the plant's p_fun and
        stays the loop's from then on (step() applies it too; None: no change).
        fused=True: the steps run as ceil(n / chunk) launches of the fused loop kernel (`Simulator.rollout_ampc_device`,
        csrc/dompc_ampc_loop.hip: the network step and the plant step alternate inside one launch), one synchronisation and one copy to
        the host after each launch - instead of two launches, a synchronisation and three copies per step.  chunk=None: one launch.
        Device memory per launch: (chunk + 1) B nx + chunk B nu float64 and chunk B int32 for the records, chunk B nw float64 more with
        noise, chunk rows of the plant's `_tvp` and `_p`.  The records equal those of the step-wise path bit for bit: both run the
        same functions on the same operands.  `k`, the states, the inputs applied last, the plant status and - for a plant with
        algebraic states - the Newton starts are left where n calls of step() leave them: the two can be mixed."""
        n = int(n)
        m = self.sim.model
        if P is not None:
            assert m.n_p > 0, "per-loop parameters for a plant whose model has none"
            P = P if type(P).__module__.startswith("torch") else self.dv.to_dev(P)
            self.P = P.to(self.dv.dev).reshape(self.B, m.n_p).contiguous()
        if W is not None and not callable(W):
            W = self._noise(W)
            assert W.shape[0] == n, f"W must hold the noise of {n} steps"

        def noise(i, K):
            """W of the steps i .. i + K - 1 on the device: [K][B][nw], or None"""
            if W is None:
                return None
            return self._noise(np.stack([np.asarray(W(i + j), float) for j in range(K)])) if callable(W) else W[i:i + K]
        if not fused and W is None:
            return _record_run(self, n)
        xs, us, st = [], [], []
        if not fused or n <= 0:
            xs.append(self.plant.X.cpu().numpy().copy()[None])
        i = 0
        while i < n:
            if fused:
                K = n - i if chunk is None else min(int(chunk), n - i)
                x, u, s = self._rollout(K, noise(i, K))
                x = x if i == 0 else x[1:]                     # (the first launch's record starts with the start of the run)
            else:
                K = 1
                r = self.step(w=noise(i, 1)[0])
                x, u, s = r["x"].copy()[None], r["u0"].copy()[None], r["plant_status"][None]
            xs.append(x); us.append(u); st.append(s)
            i += K
        # (one launch: its records as they came from the device, not copied once more)
        cat = lambda parts, shape, dt: (parts[0] if len(parts) == 1 else np.concatenate(parts)) if parts else np.zeros(shape, dtype=dt)      # noqa: E731
        return {"x": cat(xs, None, float), "u": cat(us, (0, self.B, m.n_u), float), "plant_status": cat(st, (0, self.B), np.int32)}


class BatchClosedLoopASMPC:
    """B closed loops sensitivity-based MPC -> plant advancing together, everything resident in device memory (do_mpc_amd/asmpc.py).  On
    every `asmpc.settings.resolve_every`-th control step the controller is solved at the current states - the problem, its warm start,
    u_prev and _tvp / _p refresh are the _ControllerSide of BatchClosedLoop -, differentiated and the law prepared
    (`ASMPC.solve_device`: three device calls on one stream, no host copy); every step then applies the law
    u = sat(u_ref + M (x - x_ref)) and the plant step.  With resolve_every = 1 this is the MPC loop (the law at x = x_ref adds an exact
    zero).  Between two solves the law needs nothing from the host: `run(n, fused=True)` covers those steps with ONE launch each
    (`Simulator.rollout_affine_device`).
    With `asmpc.settings.event_triggered` a step whose law status carries a bit of `settings.event_mask` for some members (far from the
    expansion point, or a fallback law) solves THOSE members again at once, as a sub-batch with their own previous solutions as warm
    start, writes their columns of the law and applies the law again; the period counter goes on.  The step's record names them in
    'resolved' and marks them with bit 4 of 'law_status'.  Such a loop is stepped (`run(n, fused=False)`): a rollout would have to be
    rewound to the first event.
    X0: [B][nx]; U_prev0: [B][nu], the inputs before the first step (default 0).  device: index of the HIP device, or "cpu" with a
    controller, a law and a plant on the host emulation (tests).  State feedback: the plant's measurement must be its state."""

    def __init__(self, asmpc, simulator, X0, U_prev0=None, device=0):
        self.asmpc, self.sim = asmpc, simulator
        mpc = self.mpc = asmpc.mpc
        ps = self.ps = mpc.structure
        dv = self.dv = _Device(device, host_ok=True)
        self.dev = dv.dev
        X0 = np.asarray(X0, dtype=float).reshape(-1, ps.nx)
        self.B = B = X0.shape[0]
        self.ctrl = _ControllerSide(mpc, dv, X0, U_prev0, lam_g=True)
        m = simulator.model
        assert m.n_x == ps.nx and m.n_u == ps.nu, "controller and plant must share states and inputs"
        self.plant = _PlantSide(simulator, dv, X0)
        self.U = dv.empty(B, ps.nu).copy_(self.ctrl.P[:, ps.p_off_uprev:])      # the inputs applied last (u_prev of the next solve)
        self.Un = dv.torch.empty_like(self.U)
        self.lstat = dv.zeros(B, dtype=dv.torch.int32)
        self.k = 0
        self._since = None                                    # control steps since the last solve (None: never solved)
        self.ev_idx = dv.zeros(B, dtype=dv.torch.int32)       # event-triggered re-solves: the members selected at a step
        self.ev_count = dv.zeros(1, dtype=dv.torch.int32)

    # the tensors and times of the two sides under the names they had on the loop (tests rebuild a solve's parameters from them)
    X = property(lambda self: self.plant.X)
    P = property(lambda self: self.ctrl.P)
    guess = property(lambda self: self.ctrl.guess)
    _p_row = property(lambda self: self.ctrl._p_row)
    t_mpc0 = property(lambda self: self.ctrl.t0)
    dt_mpc = property(lambda self: self.ctrl.dt)

    def resolve(self) -> None:
        """forces a solve at the next step"""
        self._since = None

    def _due(self) -> bool:
        return self._since is None or self._since >= int(self.asmpc.settings.resolve_every)

    def _solve(self):
        """the solve of BatchClosedLoop.step at the current states, then sensitivities and law"""
        c = self.ctrl
        self._refresh_P()
        self.asmpc.solve_device(c.guess, c.P, c.sol, c.lam_g, c.f, c.stats)
        c.guess.copy_(c.sol)
        self._since = 0

    def _refresh_P(self):
        """the parameters of a solve at the current states: _tvp / _p at the loop time, x0 <- plant state, u_prev <- applied input"""
        self.ctrl.refresh(self.k)
        self.ctrl.set_x0(self.plant.X, self.U)

    def _resolve_events(self, stream):
        """after the law step: the members whose status carries a bit of settings.event_mask are solved again at their states (a
        sub-batch solve from their own previous solutions), their law columns written, and the law applied again for the whole batch -
        the other members see an untouched law and get the same bits, the selected ones their new u0 (the law at x = x_ref adds an
        exact zero).  Returns the members (host array, empty if none)."""
        torch, a, c = self.dv.torch, self.asmpc, self.ctrl
        a.select_device(self.B, self.lstat.data_ptr(), self.ev_idx.data_ptr(), self.ev_count.data_ptr(), stream=stream)
        n = int(self.ev_count.item())                         # (4 bytes; the step synchronises anyway)
        if n == 0:
            return np.zeros(0, dtype=np.int64)
        self._refresh_P()                                     # (self.U still holds the inputs applied last: the law step wrote self.Un)
        a.solve_members_device(self.ev_idx, n, c.guess, c.P, c.sol, c.lam_g, c.f, c.stats)
        ix = self.ev_idx[:n].to(torch.int64)
        c.guess.index_copy_(0, ix, c.sol.index_select(0, ix))
        a.make_step_batch_device(self.B, self.plant.X.data_ptr(), self.Un.data_ptr(), self.lstat.data_ptr(), stream=stream)
        return self.ev_idx[:n].cpu().numpy().astype(np.int64)

    def step(self) -> dict:
        """one control step of all B loops; returns the inputs applied, the new states, the plant status, the law status, whether the
        step solved and - then - the solver statistics.  With settings.event_triggered also 'resolved': the members (int array, empty
        if none) that an event solved again at this step; they carry bit 4 in 'law_status', and 'stats' is there when there are any."""
        plant = self.plant
        solved = self._due()
        if solved:
            self._solve()
        plant.refresh(self.k)
        stream = self.dv.stream()
        self.asmpc.make_step_batch_device(self.B, plant.X.data_ptr(), self.Un.data_ptr(), self.lstat.data_ptr(), stream=stream)
        event = bool(self.asmpc.settings.event_triggered)
        # (on a step that has just solved the whole batch dx = 0: only a member whose solve failed there can be selected, and gets a
        #  second solve from the iterate the first one ended at)
        resolved = self._resolve_events(stream) if event else None
        self.U, self.Un = self.Un, self.U
        plant.step(self.U, stream)
        self.k += 1
        self._since += 1
        self.dv.sync()
        out = {"u0": self.U.cpu().numpy(), "x": plant.X.cpu().numpy(), "plant_status": plant.status()[0],
               "law_status": self.lstat.cpu().numpy().copy(), "solved": solved}
        if event:
            out["law_status"][resolved] |= 16                 # bit 4: re-solved by an event at this step
            out["resolved"] = resolved
        if solved or (event and resolved.size):
            out["stats"] = self.ctrl.stats_host()
        return out

    def _rollout(self, K):
        """K control steps between two solves in one launch; returns (x [K][B][nx], u [K][B][nu], plant status, law status)"""
        dv, plant, m, B = self.dv, self.plant, self.sim.model, self.B
        if m.n_z:
            raise NotImplementedError("BatchClosedLoopASMPC.run(fused=True): plants with algebraic states are not served by the rollout "
                                      "(run(n, fused=False) steps them)")
        tv, pp = (dv.to_dev(a) for a in plant.rows(self.k, K))
        Xt, Ut = dv.empty(K + 1, B, m.n_x), dv.empty(K, B, m.n_u)
        ps_, ls_ = (dv.zeros(K, B, dtype=dv.torch.int32) for _ in range(2))
        Xt[0].copy_(plant.X)
        law = self.asmpc.law_record()
        self.sim.rollout_affine_device(B, K, law, Xt.data_ptr(), Ut.data_ptr(), tv.data_ptr(), pp.data_ptr(), ps_.data_ptr(), ls_.data_ptr(),
                                       stream=dv.stream())
        plant.X.copy_(Xt[K])
        self.U.copy_(Ut[K - 1])
        self.k += K
        self._since += K
        dv.sync()
        return Xt[1:].cpu().numpy(), Ut.cpu().numpy(), ps_.cpu().numpy() & 1, ls_.cpu().numpy()

    def run(self, n: int, fused: bool = True) -> dict:
        """n control steps.  fused=True: the steps between two solves in one launch each; fused=False: step() n times - the same
        numbers bit for bit.  Returns the records 'x' [n + 1][B][nx] (with the start), 'u' [n][B][nu], 'plant_status' and 'law_status'
        [n][B], 'solve_steps' (indices of the steps that solved) and 'stats' (their solver statistics, one record array each).  With
        settings.event_triggered only fused=False, and 'events' is there too: per step the members an event solved again."""
        n = int(n)
        m = self.sim.model
        event = bool(self.asmpc.settings.event_triggered)
        if event and fused:
            raise NotImplementedError("BatchClosedLoopASMPC.run(fused=True): event-triggered re-solves are not served by the rollout, which "
                                      "would have to be rewound to the first event (run(n, fused=False) steps them)")
        events = []
        xs, us, pst, lst, solve_steps, stats = [self.plant.X.cpu().numpy().copy()[None]], [], [], [], [], []
        i = 0
        while i < n:
            if not fused:
                r = self.step()
                xs.append(r["x"].copy()[None]); us.append(r["u0"].copy()[None])
                pst.append(r["plant_status"][None]); lst.append(r["law_status"][None])
                if r["solved"]:
                    solve_steps.append(i); stats.append(r["stats"])
                if event:
                    events.append(r["resolved"])
                i += 1
                continue
            if self._due():
                self._solve()
                self.dv.sync()
                solve_steps.append(i); stats.append(self.ctrl.stats_host())
            K = min(int(self.asmpc.settings.resolve_every) - self._since, n - i)
            x, u, p_, l_ = self._rollout(K)
            xs.append(x); us.append(u); pst.append(p_); lst.append(l_)
            i += K
        cat = lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dtype=dt)      # noqa: E731
        out = {"x": np.concatenate(xs), "u": cat(us, (0, self.B, m.n_u), float), "plant_status": cat(pst, (0, self.B), np.int32),
               "law_status": cat(lst, (0, self.B), np.int32), "solve_steps": solve_steps, "stats": stats}
        if event:
            out["events"] = events
        return out
