"""Batched closed loop with the whole x0 batch resident in HBM.

The reference closes the loop one sample at a time on the host - `u0 = mpc.make_step(x0)`, `y = simulator.make_step(u0)`,
`x0 = estimator.make_step(y)` (/root/reference/examples/industrial_poly/main.py:105-108) - and fans batches of such loops
out over processes (`do_mpc.sampling.Sampler`, /root/reference/do_mpc/sampling/_sampler.py:198-228).  Here B loops
advance together: one `dompc_solve_batch_device` launch (structured IPM, B problems) and one
`dompc_plant_step_batch_device` launch (plant integrator, B samples) per control step on the same stream; states,
inputs, parameters and the warm-start solution stay in device memory (torch tensors are only the allocator).
State feedback (`StateFeedback.make_step` returns y, estimator/_base.py:63-72), measurement = state.
"""
from __future__ import annotations

import numpy as np

from .solver import STATS_DTYPE


class BatchClosedLoop:
    def __init__(self, mpc, simulator, X0, device: int = 0, U_prev0=None):
        import torch
        self.torch = torch
        self.mpc, self.sim = mpc, simulator
        ps = self.ps = mpc.structure
        if getattr(ps, "open_loop_stack", False):
            raise NotImplementedError("structured HIP backend: the device-resident closed loop with open_loop and several scenarios "
                                      "(the controller's vectors live in the stacked chain layout there; use make_step_batch)")
        if getattr(mpc.S, "row_mapped", False):
            raise NotImplementedError("structured HIP backend: the device-resident closed loop with rows appended to nlp_cons (internal row "
                                      "layout, solver.RowMappedSolver); use make_step_batch")
        m = simulator.model
        assert m.n_x == ps.nx and m.n_u == ps.nu, "controller and plant must share states and inputs"
        assert m.n_y == m.n_x, "state feedback: the plant's measurement must be its state"
        X0 = np.asarray(X0, dtype=float).reshape(-1, ps.nx)
        self.B = B = X0.shape[0]
        dev = self.dev = torch.device("cuda", device)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)      # noqa: E731
        t0 = float(mpc._t0[0])
        P = np.tile(mpc.opt_p_num.master, (B, 1))
        P[:, :ps.nx] = X0
        P[:, ps.p_off_tvp:ps.p_off_p] = mpc.tvp_fun(t0).master
        P[:, ps.p_off_p:ps.p_off_uprev] = mpc.p_fun(t0).master
        P[:, ps.p_off_uprev:] = 0.0 if U_prev0 is None else np.asarray(U_prev0, float).reshape(B, ps.nu)
        Xi = np.zeros((B, ps.n_opt_x))
        Xi[:, :ps.off_z].reshape(B, -1, ps.nx)[:] = (X0 / mpc._x_scaling.master)[:, None, :]
        Xi[:, ps.off_u:ps.off_eps].reshape(B, -1, ps.nu)[:] = (P[:, ps.p_off_uprev:] / mpc._u_scaling.master)[:, None, :]   # (mpc.u0 = u_prev; set_initial_guess)
        self.P, self.guess = t(P), t(Xi)                      # opt_p per sample; initial guess = set_initial_guess semantics
        self.X = t(X0)                                        # plant states
        self.lbx, self.ubx = t(mpc._lb_opt_x.master), t(mpc._ub_opt_x.master)
        self.lbg, self.ubg = t(mpc._nlp_cons_lb), t(mpc._nlp_cons_ub)
        self.sol = torch.empty((B, ps.n_opt_x), dtype=torch.float64, device=dev)
        self.f = torch.empty(B, dtype=torch.float64, device=dev)
        self.stats = torch.zeros(B * STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.U = torch.empty((B, ps.nu), dtype=torch.float64, device=dev)
        self.Xn = torch.empty_like(self.X)
        self.pstat = torch.zeros(B, dtype=torch.int32, device=dev)
        self.xs, self.us = t(mpc._x_scaling.master), t(mpc._u_scaling.master)
        ts = float(simulator._t0[0])
        self.p_plant = t(simulator.p_fun(ts).master if m.n_p else np.zeros(1))
        self.tvp_plant = t(simulator.tvp_fun(ts).master if m.n_tvp else np.zeros(1))
        self.k = 0
        # loop time: the reference's per-sample loop re-evaluates tvp_fun / p_fun at the current time in EVERY make_step of
        # controller and plant (_mpc.py:1009-1019, simulator.py:790-800) - a set-point staircase over the horizon moves along
        self.t_mpc0, self.t_sim0 = t0, ts
        self.dt_mpc, self.dt_sim = float(mpc.settings.t_step), float(simulator.settings.t_step)
        self._p_row = P[0].copy()                             # host image of one opt_p row (its _tvp / _p blocks are re-uploaded)

    def _refresh_time_varying(self):
        """_tvp / _p of controller and plant at the current loop time -> device (same values for every sample of the batch)"""
        ps, m, torch = self.ps, self.sim.model, self.torch
        tm, ts = self.t_mpc0 + self.k * self.dt_mpc, self.t_sim0 + self.k * self.dt_sim
        if ps.ntvp or ps.np_:
            row = self._p_row
            row[ps.p_off_tvp:ps.p_off_p] = self.mpc.tvp_fun(tm).master
            row[ps.p_off_p:ps.p_off_uprev] = self.mpc.p_fun(tm).master
            blk = torch.from_numpy(row[ps.p_off_tvp:ps.p_off_uprev].copy()).to(self.dev)
            self.P[:, ps.p_off_tvp:ps.p_off_uprev] = blk
        if m.n_p:
            self.p_plant.copy_(torch.from_numpy(np.ascontiguousarray(self.sim.p_fun(ts).master, dtype=np.float64)).to(self.dev))
        if m.n_tvp:
            self.tvp_plant.copy_(torch.from_numpy(np.ascontiguousarray(self.sim.tvp_fun(ts).master, dtype=np.float64)).to(self.dev))

    def step(self) -> dict:
        """one control step of all B loops; returns the solver statistics (numpy record array) and the plant status"""
        torch, ps, S = self.torch, self.ps, self.mpc.S
        stream = torch.cuda.current_stream()
        if self.k > 0:
            self._refresh_time_varying()
        S.solve_batch_device(self.B, self.guess.data_ptr(), self.lbx.data_ptr(), self.ubx.data_ptr(), self.lbg.data_ptr(),
                             self.ubg.data_ptr(), self.P.data_ptr(), self.sol.data_ptr(), 0, 0, 0, self.f.data_ptr(),
                             self.stats.data_ptr(), stream=stream.cuda_stream)
        iu = ps.iu(0, 0)
        torch.mul(self.sol[:, iu:iu + ps.nu], self.us, out=self.U)                      # u0 in physical units
        self.sim.step_batch_device(self.B, self.X.data_ptr(), self.U.data_ptr(), self.tvp_plant.data_ptr(),
                                   self.p_plant.data_ptr(), self.Xn.data_ptr(), 0, self.pstat.data_ptr(),
                                   shared_mask=2 | 4 | 8 | 16, stream=stream.cuda_stream)
        # next problem: x0 <- plant state, u_prev <- applied input, initial guess <- previous solution (optimizer.py:754-768)
        self.X, self.Xn = self.Xn, self.X
        self.P[:, :ps.nx] = self.X
        self.P[:, ps.p_off_uprev:] = self.U
        self.guess.copy_(self.sol)
        self.k += 1
        torch.cuda.synchronize()
        st = np.frombuffer(self.stats.cpu().numpy().tobytes(), dtype=STATS_DTYPE).copy()
        return {"stats": st, "plant_status": (self.pstat.cpu().numpy() & 1), "plant_implicit": ((self.pstat.cpu().numpy() >> 1) & 1), "u0": self.U.cpu().numpy(), "x": self.X.cpu().numpy()}


class BatchClosedLoopMHE:
    """B closed loops controller -> plant -> moving horizon estimator -> controller advancing together, everything resident in HBM
    (the loop of examples/rotating_oscillating_masses_mhe_mpc/main.py, one sample at a time on the host there): per control step
    ONE batched solve of the controller (B problems), ONE batched plant step (states and measurements), ONE batched solve of the
    estimator (B estimation problems), plus index arithmetic on device tensors - the estimator's parameter vectors (previous
    estimates, sliding measurement window) and initial guesses are assembled from the previous device results.
    The controller's and the estimator's problems live in their chain layouts (do_mpc_amd/estimator.py); torch is the allocator
    and does the slicing."""

    def __init__(self, mpc, simulator, mhe, X0_true, x0_est=None, p_est0=None, device: int = 0):
        import torch
        self.torch = torch
        self.mpc, self.sim, self.mhe = mpc, simulator, mhe
        m = simulator.model
        ps, es = mpc.structure, mhe._ps                     # controller / estimator chain structures
        if getattr(ps, "open_loop_stack", False):
            raise NotImplementedError("structured HIP backend: the device-resident closed loop with open_loop and several scenarios")
        if getattr(mpc.S, "row_mapped", False):
            raise NotImplementedError("structured HIP backend: the device-resident closed loop with rows appended to nlp_cons")
        self.ps, self.es = ps, es
        X0_true = np.asarray(X0_true, dtype=float).reshape(-1, m.n_x)
        self.B = B = X0_true.shape[0]
        dev = self.dev = torch.device("cuda", device)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)      # noqa: E731
        nx, nu, ny, npe = m.n_x, m.n_u, m.n_y, mhe.n_p_est
        self.nx, self.nu, self.ny, self.npe = nx, nu, ny, npe
        x_est = np.zeros((B, nx)) if x0_est is None else np.broadcast_to(np.asarray(x0_est, float).reshape(-1, nx), (B, nx)).copy()
        p_est = np.zeros((B, npe)) if p_est0 is None else np.broadcast_to(np.asarray(p_est0, float).reshape(-1, npe), (B, npe)).copy()
        # ---- controller: opt_p rows, initial guess (set_initial_guess semantics), bounds
        t0 = float(mpc._t0[0])
        Pc = np.tile(mpc.opt_p_num.master, (B, 1))
        Pc[:, :nx] = x_est
        Pc[:, ps.p_off_tvp:ps.p_off_p] = mpc.tvp_fun(t0).master
        Pc[:, ps.p_off_p:ps.p_off_uprev] = mpc.p_fun(t0).master
        Pc[:, ps.p_off_uprev:] = 0.0
        Gc = np.zeros((B, ps.n_opt_x))
        Gc[:, :ps.off_z].reshape(B, -1, ps.nx)[:] = (x_est / mpc._x_scaling.master)[:, None, :]
        self.Pc, self.Gc = t(Pc), t(Gc)
        self.c_lbx, self.c_ubx = t(mpc._lb_opt_x.master), t(mpc._ub_opt_x.master)
        self.c_lbg, self.c_ubg = t(mpc._nlp_cons_lb), t(mpc._nlp_cons_ub)
        self.c_sol = torch.empty((B, ps.n_opt_x), dtype=torch.float64, device=dev)
        self.c_f = torch.empty(B, dtype=torch.float64, device=dev)
        self.c_stats = torch.zeros(B * STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.xs, self.us = t(mpc._x_scaling.master), t(mpc._u_scaling.master)
        # ---- plant
        self.X = t(X0_true)
        self.Xn = torch.empty_like(self.X)
        self.U = torch.empty((B, nu), dtype=torch.float64, device=dev)
        self.Y = torch.empty((B, ny), dtype=torch.float64, device=dev)
        self.pstat = torch.zeros(B, dtype=torch.int32, device=dev)
        ts = float(simulator._t0[0])
        self.p_plant = t(simulator.p_fun(ts).master if m.n_p else np.zeros(1))
        self.tvp_plant = t(simulator.tvp_fun(ts).master if m.n_tvp else np.zeros(1))
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
        self.e_sol = torch.empty((B, es.n_opt_x), dtype=torch.float64, device=dev)
        self.e_f = torch.empty(B, dtype=torch.float64, device=dev)
        self.e_stats = torch.zeros(B * STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.x_est, self.p_est = t(x_est), t(p_est)
        self.exs = t(mhe._x_scaling.master)
        self.eps_ = t(pes if npe else np.zeros(1))              # scaling of the estimated parameters (they ride as scaled states of the chain problem)
        self.t_mpc0, self.dt = t0, float(mpc.settings.t_step)
        self.t_sim0, self.dt_sim = ts, float(simulator.settings.t_step)
        self.t_mhe0, self.dt_mhe = te, float(mhe.settings.t_step)
        self._pc_row = Pc[0].copy()
        self.k = 0

    def _refresh_time_varying(self):
        """_tvp / _p of controller, plant AND estimator at the current loop time -> device (same values for every sample).  The
        reference's per-sample loop re-evaluates all of them in every make_step (_mpc.py:1009-1019, simulator.py:790-800,
        _mhe.py:940-950); only the measurement columns of the estimator's window are data of the loop."""
        torch, ps, es, m, mhe = self.torch, self.ps, self.es, self.sim.model, self.mhe
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)      # noqa: E731
        tm, ts, te = self.t_mpc0 + self.k * self.dt, self.t_sim0 + self.k * self.dt_sim, self.t_mhe0 + self.k * self.dt_mhe
        if ps.ntvp or ps.np_:
            row = self._pc_row
            row[ps.p_off_tvp:ps.p_off_p] = self.mpc.tvp_fun(tm).master
            row[ps.p_off_p:ps.p_off_uprev] = self.mpc.p_fun(tm).master
            self.Pc[:, ps.p_off_tvp:ps.p_off_uprev] = up(row[ps.p_off_tvp:ps.p_off_uprev].copy())
        if m.n_p:
            self.p_plant.copy_(up(self.sim.p_fun(ts).master))
        if m.n_tvp:
            self.tvp_plant.copy_(up(self.sim.tvp_fun(ts).master))
        mt = mhe.model.n_tvp
        if mt or mhe.n_p_set:
            op = np.zeros((1, mhe.n_opt_p))
            op[:, mhe._po_pset:mhe._po_tvp] = mhe.p_fun(te).master
            op[:, mhe._po_tvp:mhe._po_y] = mhe.tvp_fun(te).master
            pc = mhe._p_to_chain(op)[0]
            if mt:
                tv = pc[es.p_off_tvp:es.p_off_p].reshape(self.N + 1, es.ntvp)[:, :mt]
                self.Pe[:, es.p_off_tvp:es.p_off_p].view(self.B, self.N + 1, es.ntvp)[:, :, :mt] = up(tv.copy())
            if es.p_off_uprev > es.p_off_p:
                self.Pe[:, es.p_off_p:es.p_off_uprev] = up(pc[es.p_off_p:es.p_off_uprev].copy())

    def step(self) -> dict:
        torch, ps, es, B, nx, nu, ny, npe, N = self.torch, self.ps, self.es, self.B, self.nx, self.nu, self.ny, self.npe, self.N
        stream = torch.cuda.current_stream()
        mt = self.mhe.model.n_tvp
        if self.k > 0:
            self._refresh_time_varying()
        # 1. controller
        self.mpc.S.solve_batch_device(B, self.Gc.data_ptr(), self.c_lbx.data_ptr(), self.c_ubx.data_ptr(), self.c_lbg.data_ptr(),
                                      self.c_ubg.data_ptr(), self.Pc.data_ptr(), self.c_sol.data_ptr(), 0, 0, 0, self.c_f.data_ptr(),
                                      self.c_stats.data_ptr(), stream=stream.cuda_stream)
        iu = ps.iu(0, 0)
        torch.mul(self.c_sol[:, iu:iu + nu], self.us, out=self.U)
        # 2. plant: next true state and its measurement
        self.sim.step_batch_device(B, self.X.data_ptr(), self.U.data_ptr(), self.tvp_plant.data_ptr(), self.p_plant.data_ptr(),
                                   self.Xn.data_ptr(), self.Y.data_ptr(), self.pstat.data_ptr(), shared_mask=2 | 4 | 8 | 16,
                                   stream=stream.cuda_stream)
        self.X, self.Xn = self.Xn, self.X
        # 3. estimator: previous estimates <- `_x[1, -1]`, `_p_est` of ITS previous solution (initial guess before the first solve,
        #    _mhe.py:939-941), measurement window shifted by one stage, the new measurement last
        i1 = es.ix(1, 0, es.M)
        self.Pe[:, :nx] = self.Ge[:, i1:i1 + nx] * self.exs
        self.Pe[:, nx:nx + npe] = self.p_est
        TV = self.Pe[:, es.p_off_tvp:es.p_off_p].view(B, N + 1, es.ntvp)
        TV[:, :N - 1, mt:] = TV[:, 1:N, mt:].clone()
        TV[:, N - 1, mt:] = self.Y
        self.mhe.S.solve_batch_device(B, self.Ge.data_ptr(), self.e_lbx.data_ptr(), self.e_ubx.data_ptr(), self.e_lbg.data_ptr(),
                                      self.e_ubg.data_ptr(), self.Pe.data_ptr(), self.e_sol.data_ptr(), 0, 0, 0, self.e_f.data_ptr(),
                                      self.e_stats.data_ptr(), stream=stream.cuda_stream)
        iN = es.ix(N, 0, es.M)
        self.x_est = self.e_sol[:, iN:iN + nx] * self.exs
        i0 = es.ix(0, 0, es.M)
        # (physical units: the chain problem carries the parameter as a SCALED state; `_p_est_prev` of the arrival cost and the
        #  returned estimate are physical, _mhe.py: opt_x_num['_p_est'] * _p_est_scaling - ADVICE r3)
        self.p_est = self.e_sol[:, i0 + nx:i0 + nx + npe] * self.eps_[:npe] if npe else self.e_sol[:, i0 + nx:i0 + nx].clone()
        self.Ge.copy_(self.e_sol)                                  # warm start (unshifted, optimizer.py:754-768)
        # 4. next controller problem: x0 <- estimate, u_prev <- applied input, initial guess <- previous solution
        self.Pc[:, :nx] = self.x_est
        self.Pc[:, ps.p_off_uprev:] = self.U
        self.Gc.copy_(self.c_sol)
        self.k += 1
        torch.cuda.synchronize()
        cs = np.frombuffer(self.c_stats.cpu().numpy().tobytes(), dtype=STATS_DTYPE).copy()
        est = np.frombuffer(self.e_stats.cpu().numpy().tobytes(), dtype=STATS_DTYPE).copy()
        return {"mpc_stats": cs, "mhe_stats": est, "plant_status": (self.pstat.cpu().numpy() & 1), "plant_implicit": ((self.pstat.cpu().numpy() >> 1) & 1), "u0": self.U.cpu().numpy(),
                "x_true": self.X.cpu().numpy(), "y": self.Y.cpu().numpy(), "x_est": self.x_est.cpu().numpy(), "p_est": self.p_est.cpu().numpy()}


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
        import torch
        self.torch = torch
        self.mpc, self.sim, self.ekf = mpc, simulator, ekf
        m = simulator.model
        ps = self.ps = mpc.structure
        if getattr(ps, "open_loop_stack", False):
            raise NotImplementedError("structured HIP backend: the device-resident closed loop with open_loop and several scenarios")
        if getattr(mpc.S, "row_mapped", False):
            raise NotImplementedError("structured HIP backend: the device-resident closed loop with rows appended to nlp_cons")
        me = ekf.model
        assert m.n_x == ps.nx and m.n_u == ps.nu, "controller and plant must share states and inputs"
        assert (me.n_x, me.n_u, me.n_y) == (m.n_x, m.n_u, m.n_y), "plant and filter must share states, inputs and measurements"
        X0_true = np.asarray(X0_true, dtype=float).reshape(-1, m.n_x)
        self.B = B = X0_true.shape[0]
        dev = self.dev = torch.device("cuda", device)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)      # noqa: E731
        nx, nu, ny = m.n_x, m.n_u, m.n_y
        self.nx, self.nu, self.ny = nx, nu, ny
        x_est = np.broadcast_to(np.asarray(x0_est, float).reshape(-1, nx), (B, nx)).copy()
        P0 = np.asarray(P0, float)
        Pcov = np.broadcast_to(P0.reshape(-1, nx, nx), (B, nx, nx)).copy()
        Q, R = np.asarray(Q, float), np.asarray(R, float)
        assert Q.shape in ((nx, nx), (B, nx, nx)) and R.shape in ((ny, ny), (B, ny, ny)), "Q / R: one matrix or one per loop"
        self.mask = 2 | 4 | (8 if Q.ndim == 2 else 0) | (16 if R.ndim == 2 else 0)
        self.Q, self.R = t(Q), t(R)
        # ---- controller: opt_p rows, initial guess (set_initial_guess semantics), bounds
        t0 = float(mpc._t0[0])
        Pc = np.tile(mpc.opt_p_num.master, (B, 1))
        Pc[:, :nx] = x_est
        Pc[:, ps.p_off_tvp:ps.p_off_p] = mpc.tvp_fun(t0).master
        Pc[:, ps.p_off_p:ps.p_off_uprev] = mpc.p_fun(t0).master
        Pc[:, ps.p_off_uprev:] = 0.0
        Gc = np.zeros((B, ps.n_opt_x))
        Gc[:, :ps.off_z].reshape(B, -1, ps.nx)[:] = (x_est / mpc._x_scaling.master)[:, None, :]
        self.Pc, self.Gc = t(Pc), t(Gc)
        self.c_lbx, self.c_ubx = t(mpc._lb_opt_x.master), t(mpc._ub_opt_x.master)
        self.c_lbg, self.c_ubg = t(mpc._nlp_cons_lb), t(mpc._nlp_cons_ub)
        self.c_sol = torch.empty((B, ps.n_opt_x), dtype=torch.float64, device=dev)
        self.c_f = torch.empty(B, dtype=torch.float64, device=dev)
        self.c_stats = torch.zeros(B * STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.us = t(mpc._u_scaling.master)
        # ---- plant
        self.X = t(X0_true)
        self.Xn = torch.empty_like(self.X)
        self.U = torch.empty((B, nu), dtype=torch.float64, device=dev)
        self.Y = torch.empty((B, max(ny, 1)), dtype=torch.float64, device=dev)
        self.pstat = torch.zeros(B, dtype=torch.int32, device=dev)
        ts = float(simulator._t0[0])
        self.p_plant = t(simulator.p_fun(ts).master if m.n_p else np.zeros(1))
        self.tvp_plant = t(simulator.tvp_fun(ts).master if m.n_tvp else np.zeros(1))
        self._V = V
        self.V = torch.zeros((B, max(m.n_v, 1)), dtype=torch.float64, device=dev)
        # ---- filter
        te = float(ekf._t0[0])
        self.x_est, self.Pcov = t(x_est), t(Pcov)
        self.p_ekf = t(ekf.p_fun(te).master if me.n_p else np.zeros(1))
        self.tvp_ekf = t(ekf.tvp_fun(te).master if me.n_tvp else np.zeros(1))
        self.estat = torch.zeros(B, dtype=torch.int32, device=dev)
        self.nz = me.n_z
        if self.nz:
            self.z_est = t(np.tile(ekf.z0.master, (B, 1)))
            self.enewton = torch.zeros(B, dtype=torch.int32, device=dev)
        self.t_mpc0, self.dt = t0, float(mpc.settings.t_step)
        self.t_sim0, self.dt_sim = ts, float(simulator.settings.t_step)
        self.t_ekf0, self.dt_ekf = te, float(ekf.settings.t_step)
        self._pc_row = Pc[0].copy()
        self.k = 0

    def _refresh_time_varying(self):
        """_tvp / _p of controller, plant and filter at the current loop time -> device (same values for every loop): the per-sample
        loop re-evaluates all of them in every make_step (_mpc.py:1009-1019, simulator.py:790-800, _ekf.py:268-270)"""
        torch, ps, m, me = self.torch, self.ps, self.sim.model, self.ekf.model
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)      # noqa: E731
        tm, ts, te = self.t_mpc0 + self.k * self.dt, self.t_sim0 + self.k * self.dt_sim, self.t_ekf0 + self.k * self.dt_ekf
        if ps.ntvp or ps.np_:
            row = self._pc_row
            row[ps.p_off_tvp:ps.p_off_p] = self.mpc.tvp_fun(tm).master
            row[ps.p_off_p:ps.p_off_uprev] = self.mpc.p_fun(tm).master
            self.Pc[:, ps.p_off_tvp:ps.p_off_uprev] = up(row[ps.p_off_tvp:ps.p_off_uprev].copy())
        if m.n_p:
            self.p_plant.copy_(up(self.sim.p_fun(ts).master))
        if m.n_tvp:
            self.tvp_plant.copy_(up(self.sim.tvp_fun(ts).master))
        if me.n_p:
            self.p_ekf.copy_(up(self.ekf.p_fun(te).master))
        if me.n_tvp:
            self.tvp_ekf.copy_(up(self.ekf.tvp_fun(te).master))

    def step(self) -> dict:
        torch, ps, B, nx, nu = self.torch, self.ps, self.B, self.nx, self.nu
        stream = torch.cuda.current_stream()
        if self.k > 0:
            self._refresh_time_varying()
        nv = self.sim.model.n_v
        if self._V is not None and nv:
            v = self._V(self.k) if callable(self._V) else self._V
            self.V.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(v, float).reshape(B, nv))).to(self.dev))
        # 1. controller
        self.mpc.S.solve_batch_device(B, self.Gc.data_ptr(), self.c_lbx.data_ptr(), self.c_ubx.data_ptr(), self.c_lbg.data_ptr(),
                                      self.c_ubg.data_ptr(), self.Pc.data_ptr(), self.c_sol.data_ptr(), 0, 0, 0, self.c_f.data_ptr(),
                                      self.c_stats.data_ptr(), stream=stream.cuda_stream)
        iu = ps.iu(0, 0)
        torch.mul(self.c_sol[:, iu:iu + nu], self.us, out=self.U)
        # 2. plant: next true state and its measurement
        self.sim.step_batch_device(B, self.X.data_ptr(), self.U.data_ptr(), self.tvp_plant.data_ptr(), self.p_plant.data_ptr(),
                                   self.Xn.data_ptr(), self.Y.data_ptr(), self.pstat.data_ptr(),
                                   v=(self.V.data_ptr() if (self._V is not None and nv) else 0), shared_mask=2 | 4 | 8,
                                   stream=stream.cuda_stream)
        self.X, self.Xn = self.Xn, self.X
        # 3. filter: estimate and covariance in place
        self.ekf.step_batch_device(B, self.x_est.data_ptr(), self.Pcov.data_ptr(), self.Y.data_ptr(), self.U.data_ptr(),
                                   self.tvp_ekf.data_ptr(), self.p_ekf.data_ptr(), self.Q.data_ptr(), self.R.data_ptr(),
                                   status=self.estat.data_ptr(), shared_mask=self.mask, stream=stream.cuda_stream,
                                   **({"z": self.z_est.data_ptr(), "newton": self.enewton.data_ptr()} if self.nz else {}))
        # 4. next controller problem: x0 <- estimate, u_prev <- applied input, initial guess <- previous solution
        self.Pc[:, :nx] = self.x_est
        self.Pc[:, ps.p_off_uprev:] = self.U
        self.Gc.copy_(self.c_sol)
        self.k += 1
        torch.cuda.synchronize()
        cs = np.frombuffer(self.c_stats.cpu().numpy().tobytes(), dtype=STATS_DTYPE).copy()
        est = self.estat.cpu().numpy()
        out = {"mpc_stats": cs, "plant_status": (self.pstat.cpu().numpy() & 1), "ekf_status": est & 0xFF, "u0": self.U.cpu().numpy(),
               "x_true": self.X.cpu().numpy(), "y": self.Y[:, :self.ny].cpu().numpy(), "x_est": self.x_est.cpu().numpy(),
               "P": self.Pcov.cpu().numpy()}
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
    device: index of the HIP device, or "cpu" with a controller and a plant on the host emulation (tests)."""

    def __init__(self, lqr, simulator, X0, K=None, XSS=None, USS=None, device=0, U_prev0=None):
        import torch
        self.torch = torch
        self.lqr, self.sim = lqr, simulator
        assert lqr.flags["setup"] is True, "LQR is not setup. run setup() function."
        m = simulator.model
        ml = lqr.model
        assert (m.n_x, m.n_u) == (ml.n_x, ml.n_u), "controller and plant must share states and inputs"
        assert m.n_y == m.n_x, "state feedback: the plant's measurement must be its state"
        X0 = np.asarray(X0, dtype=float).reshape(-1, m.n_x)
        self.B = B = X0.shape[0]
        dev = self.dev = torch.device("cpu") if device == "cpu" else torch.device("cuda", device)
        t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), device=dev)      # noqa: E731  (a copy, also on the host)
        rate = lqr.mode == "inputRatePenalization"
        if XSS is None and USS is None and hasattr(lqr, "xss"):
            xs = np.asarray(lqr.xss, float).ravel()
            XSS, USS = xs[:m.n_x], (xs[m.n_x:] if rate else np.asarray(lqr.uss, float).ravel())
        self.xss = t(np.zeros((1, m.n_x)) if XSS is None else np.asarray(XSS, float).reshape(-1, m.n_x))
        self.uss = t(np.zeros((1, m.n_u)) if USS is None else np.asarray(USS, float).reshape(-1, m.n_u))
        self.K = t(np.asarray(lqr.K if K is None else K, float).reshape(-1, m.n_u, lqr.n_design))
        assert self.K.shape[0] in (1, B) and self.xss.shape[0] in (1, B) and self.uss.shape[0] in (1, B), "one gain / set-point or one per loop"
        self.X = t(X0)
        self.Xn = torch.empty_like(self.X)
        self.U = t(np.zeros((B, m.n_u)) if U_prev0 is None else np.asarray(U_prev0, float).reshape(B, m.n_u))
        self.pstat = torch.zeros(B, dtype=torch.int32, device=dev)
        ts = float(simulator._t0[0])
        self.p_plant = t(simulator.p_fun(ts).master if m.n_p else np.zeros(1))
        self.tvp_plant = t(simulator.tvp_fun(ts).master if m.n_tvp else np.zeros(1))
        self.t_sim0, self.dt_sim = ts, float(simulator.settings.t_step)
        self.k = 0

    def step(self) -> dict:
        """one control step of all B loops; returns the inputs applied, the new states and the plant status"""
        torch, m = self.torch, self.sim.model
        cuda = self.dev.type == "cuda"
        if self.k > 0 and (m.n_p or m.n_tvp):      # the plant's parameters at the current loop time (simulator.py:790-800)
            ts = self.t_sim0 + self.k * self.dt_sim
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)      # noqa: E731
            if m.n_p:
                self.p_plant.copy_(up(self.sim.p_fun(ts).master))
            if m.n_tvp:
                self.tvp_plant.copy_(up(self.sim.tvp_fun(ts).master))
        self.U = self.lqr.make_step_batch(self.X, K=self.K, XSS=self.xss, USS=self.uss, U_prev=self.U).contiguous()
        self.sim.step_batch_device(self.B, self.X.data_ptr(), self.U.data_ptr(), self.tvp_plant.data_ptr(), self.p_plant.data_ptr(),
                                   self.Xn.data_ptr(), 0, self.pstat.data_ptr(), shared_mask=2 | 4 | 8 | 16,
                                   stream=(torch.cuda.current_stream().cuda_stream if cuda else 0))
        self.X, self.Xn = self.Xn, self.X
        self.k += 1
        if cuda:
            torch.cuda.synchronize()
        return {"u0": self.U.cpu().numpy(), "x": self.X.cpu().numpy(), "plant_status": (self.pstat.cpu().numpy() & 1)}

    def run(self, n: int) -> dict:
        """n control steps; returns the records 'x' [n + 1][B][nx] (with the start), 'u' [n][B][nu] and the plant status of every step"""
        xs, us, st = [self.X.cpu().numpy().copy()], [], []
        for _ in range(int(n)):
            r = self.step()
            xs.append(r["x"].copy())
            us.append(r["u0"].copy())
            st.append(r["plant_status"])
        return {"x": np.stack(xs), "u": np.stack(us) if us else np.zeros((0, self.B, self.sim.model.n_u)),
                "plant_status": np.stack(st) if st else np.zeros((0, self.B), dtype=np.int32)}


class BatchClosedLoopAMPC:
    """B closed loops approximate MPC -> plant advancing together with X and U resident in device memory (float64): per control step
    TWO launches, the network kernel (ApproxMPC.make_step_batch_device) and ONE batched plant step.  The per-sample loop of the
    reference is `u0 = approx_mpc.make_step(x0)`, `x0 = simulator.make_step(u0)`
    (/root/reference/examples/CSTR_approximate_mpc/main.py:164-170).  State feedback: the plant's measurement must be its state.
    X0: [B][nx]; U_prev0: [B][nu], the inputs before the first step (default: ampc.u0 for every loop; read only when the controller
    has an rterm).  device: index of the HIP device, or "cpu" with a controller and a plant on the host emulation (tests)."""

    def __init__(self, ampc, simulator, X0, U_prev0=None, device=0, clip_to_bounds=True):
        import torch
        self.torch = torch
        self.ampc, self.sim, self.clip = ampc, simulator, bool(clip_to_bounds)
        assert ampc.flags["setup"] == True, "MPC was not setup yet. Please call ApproxMPC.setup()."      # noqa: E712
        m = simulator.model
        mc = ampc.mpc.model
        assert (m.n_x, m.n_u) == (mc.n_x, mc.n_u), "controller and plant must share states and inputs"
        assert m.n_y == m.n_x, "state feedback: the plant's measurement must be its state"
        X0 = np.asarray(X0, dtype=float).reshape(-1, m.n_x)
        self.B = B = X0.shape[0]
        dev = self.dev = torch.device("cpu") if device == "cpu" else torch.device("cuda", device)
        t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), device=dev)      # noqa: E731  (a copy, also on the host)
        self.X = t(X0)
        self.Xn = torch.empty_like(self.X)
        if U_prev0 is None:
            u0 = ampc.u0
            U_prev0 = np.tile(np.asarray(u0.master if hasattr(u0, "master") else u0, dtype=float).reshape(1, m.n_u), (B, 1))
        self.U = t(np.asarray(U_prev0, float).reshape(B, m.n_u))
        self.Un = torch.empty_like(self.U)
        self.pstat = torch.zeros(B, dtype=torch.int32, device=dev)
        ts = float(simulator._t0[0])
        self.p_plant = t(simulator.p_fun(ts).master if m.n_p else np.zeros(1))
        self.tvp_plant = t(simulator.tvp_fun(ts).master if m.n_tvp else np.zeros(1))
        self.t_sim0, self.dt_sim = ts, float(simulator.settings.t_step)
        self.k = 0

    def step(self) -> dict:
        """one control step of all B loops; returns the inputs applied, the new states and the plant status"""
        torch, m = self.torch, self.sim.model
        cuda = self.dev.type == "cuda"
        if self.k > 0 and (m.n_p or m.n_tvp):      # the plant's parameters at the current loop time
            ts = self.t_sim0 + self.k * self.dt_sim
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)      # noqa: E731
            if m.n_p:
                self.p_plant.copy_(up(self.sim.p_fun(ts).master))
            if m.n_tvp:
                self.tvp_plant.copy_(up(self.sim.tvp_fun(ts).master))
        stream = torch.cuda.current_stream().cuda_stream if cuda else 0
        self.ampc.make_step_batch_device(self.B, self.X.data_ptr(), self.U.data_ptr() if self.ampc.rterm else 0, self.Un.data_ptr(),
                                         stream=stream, clip_to_bounds=self.clip)
        self.U, self.Un = self.Un, self.U
        self.sim.step_batch_device(self.B, self.X.data_ptr(), self.U.data_ptr(), self.tvp_plant.data_ptr(), self.p_plant.data_ptr(),
                                   self.Xn.data_ptr(), 0, self.pstat.data_ptr(), shared_mask=2 | 4 | 8 | 16, stream=stream)
        self.X, self.Xn = self.Xn, self.X
        self.k += 1
        if cuda:
            torch.cuda.synchronize()
        return {"u0": self.U.cpu().numpy(), "x": self.X.cpu().numpy(), "plant_status": (self.pstat.cpu().numpy() & 1)}

    def run(self, n: int) -> dict:
        """n control steps; returns the records 'x' [n + 1][B][nx] (with the start), 'u' [n][B][nu] and the plant status of every step"""
        xs, us, st = [self.X.cpu().numpy().copy()], [], []
        for _ in range(int(n)):
            r = self.step()
            xs.append(r["x"].copy())
            us.append(r["u0"].copy())
            st.append(r["plant_status"])
        return {"x": np.stack(xs), "u": np.stack(us) if us else np.zeros((0, self.B, self.sim.model.n_u)),
                "plant_status": np.stack(st) if st else np.zeros((0, self.B), dtype=np.int32)}


class BatchClosedLoopASMPC:
    """B closed loops sensitivity-based MPC -> plant advancing together, everything resident in device memory (do_mpc_amd/asmpc.py).  On
    every `asmpc.settings.resolve_every`-th control step the controller is solved at the current states - warm start, u_prev and the
    _tvp / _p refresh exactly those of BatchClosedLoop.step -, differentiated and the law prepared (`ASMPC.solve_device`: three device
    calls on one stream, no host copy); every step then applies the law u = sat(u_ref + M (x - x_ref)) and the plant step.  With
    resolve_every = 1 this is the MPC loop (the law at x = x_ref adds an exact zero).  Between two solves the law needs nothing from the
    host: `run(n, fused=True)` covers those steps with ONE launch each (`Simulator.rollout_affine_device`).
    With `asmpc.settings.event_triggered` a step whose law status carries a bit of `settings.event_mask` for some members (far from the
    expansion point, or a fallback law) solves THOSE members again at once, as a sub-batch with their own previous solutions as warm
    start, writes their columns of the law and applies the law again; the period counter goes on.  The step's record names them in
    'resolved' and marks them with bit 4 of 'law_status'.  Such a loop is stepped (`run(n, fused=False)`): a rollout would have to be
    rewound to the first event.
    X0: [B][nx]; U_prev0: [B][nu], the inputs before the first step (default 0).  device: index of the HIP device, or "cpu" with a
    controller, a law and a plant on the host emulation (tests).  State feedback: the plant's measurement must be its state."""

    def __init__(self, asmpc, simulator, X0, U_prev0=None, device=0):
        import torch
        self.torch = torch
        self.asmpc, self.sim = asmpc, simulator
        mpc = self.mpc = asmpc.mpc
        ps = self.ps = mpc.structure
        if getattr(ps, "open_loop_stack", False):
            raise NotImplementedError("structured HIP backend: the device-resident closed loop with open_loop and several scenarios")
        if getattr(mpc.S, "row_mapped", False):
            raise NotImplementedError("structured HIP backend: the device-resident closed loop with rows appended to nlp_cons")
        m = simulator.model
        assert m.n_x == ps.nx and m.n_u == ps.nu, "controller and plant must share states and inputs"
        assert m.n_y == m.n_x, "state feedback: the plant's measurement must be its state"
        X0 = np.asarray(X0, dtype=float).reshape(-1, ps.nx)
        self.B = B = X0.shape[0]
        dev = self.dev = torch.device("cpu") if device == "cpu" else torch.device("cuda", device)
        t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), device=dev)      # noqa: E731  (a copy, also on the host)
        t0 = float(mpc._t0[0])
        P = np.tile(mpc.opt_p_num.master, (B, 1))
        P[:, :ps.nx] = X0
        P[:, ps.p_off_tvp:ps.p_off_p] = mpc.tvp_fun(t0).master
        P[:, ps.p_off_p:ps.p_off_uprev] = mpc.p_fun(t0).master
        P[:, ps.p_off_uprev:] = 0.0 if U_prev0 is None else np.asarray(U_prev0, float).reshape(B, ps.nu)
        Xi = np.zeros((B, ps.n_opt_x))
        Xi[:, :ps.off_z].reshape(B, -1, ps.nx)[:] = (X0 / mpc._x_scaling.master)[:, None, :]
        Xi[:, ps.off_u:ps.off_eps].reshape(B, -1, ps.nu)[:] = (P[:, ps.p_off_uprev:] / mpc._u_scaling.master)[:, None, :]
        self.P, self.guess = t(P), t(Xi)
        self.X = t(X0)
        self.Xn = torch.empty_like(self.X)
        self.U = t(P[:, ps.p_off_uprev:])                     # the inputs applied last (u_prev of the next solve)
        self.Un = torch.empty_like(self.U)
        self.sol = torch.empty((B, ps.n_opt_x), dtype=torch.float64, device=dev)
        self.lam_g = torch.empty((B, ps.n_g), dtype=torch.float64, device=dev)
        self.f = torch.empty(B, dtype=torch.float64, device=dev)
        self.stats = torch.zeros(B * STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.pstat = torch.zeros(B, dtype=torch.int32, device=dev)
        self.lstat = torch.zeros(B, dtype=torch.int32, device=dev)
        ts = float(simulator._t0[0])
        self.p_plant = t(simulator.p_fun(ts).master if m.n_p else np.zeros(1))
        self.tvp_plant = t(simulator.tvp_fun(ts).master if m.n_tvp else np.zeros(1))
        self.t_mpc0, self.t_sim0 = t0, ts
        self.dt_mpc, self.dt_sim = float(mpc.settings.t_step), float(simulator.settings.t_step)
        self._p_row = P[0].copy()
        self.k = 0
        self._since = None                                    # control steps since the last solve (None: never solved)
        self.ev_idx = torch.zeros(B, dtype=torch.int32, device=dev)       # event-triggered re-solves: the members selected at a step
        self.ev_count = torch.zeros(1, dtype=torch.int32, device=dev)

    def resolve(self) -> None:
        """forces a solve at the next step"""
        self._since = None

    def _stream(self):
        return self.torch.cuda.current_stream(self.dev).cuda_stream if self.dev.type == "cuda" else 0

    def _sync(self):
        if self.dev.type == "cuda":
            self.torch.cuda.synchronize(self.dev)

    def _due(self) -> bool:
        return self._since is None or self._since >= int(self.asmpc.settings.resolve_every)

    def _solve(self):
        """the solve of BatchClosedLoop.step at the current states, then sensitivities and law: x0 <- plant state, u_prev <- applied
        input, initial guess <- previous solution, the controller's _tvp / _p at the current loop time"""
        self._refresh_P()
        self.asmpc.solve_device(self.guess, self.P, self.sol, self.lam_g, self.f, self.stats)
        self.guess.copy_(self.sol)
        self._since = 0

    def _refresh_P(self):
        """the parameters of a solve at the current states: x0 <- plant state, u_prev <- applied input, _tvp / _p at the loop time"""
        torch, ps = self.torch, self.ps
        if self.k > 0 and (ps.ntvp or ps.np_):
            tm = self.t_mpc0 + self.k * self.dt_mpc
            row = self._p_row
            row[ps.p_off_tvp:ps.p_off_p] = self.mpc.tvp_fun(tm).master
            row[ps.p_off_p:ps.p_off_uprev] = self.mpc.p_fun(tm).master
            self.P[:, ps.p_off_tvp:ps.p_off_uprev] = torch.from_numpy(row[ps.p_off_tvp:ps.p_off_uprev].copy()).to(self.dev)
        self.P[:, :ps.nx] = self.X
        self.P[:, ps.p_off_uprev:] = self.U

    def _resolve_events(self, stream):
        """after the law step: the members whose status carries a bit of settings.event_mask are solved again at their states (a
        sub-batch solve from their own previous solutions), their law columns written, and the law applied again for the whole batch -
        the other members see an untouched law and get the same bits, the selected ones their new u0 (the law at x = x_ref adds an
        exact zero).  Returns the members (host array, empty if none)."""
        torch, a = self.torch, self.asmpc
        a.select_device(self.B, self.lstat.data_ptr(), self.ev_idx.data_ptr(), self.ev_count.data_ptr(), stream=stream)
        n = int(self.ev_count.item())                         # (4 bytes; the step synchronises anyway)
        if n == 0:
            return np.zeros(0, dtype=np.int64)
        self._refresh_P()                                     # (self.U still holds the inputs applied last: the law step wrote self.Un)
        a.solve_members_device(self.ev_idx, n, self.guess, self.P, self.sol, self.lam_g, self.f, self.stats)
        ix = self.ev_idx[:n].to(torch.int64)
        self.guess.index_copy_(0, ix, self.sol.index_select(0, ix))
        a.make_step_batch_device(self.B, self.X.data_ptr(), self.Un.data_ptr(), self.lstat.data_ptr(), stream=stream)
        return self.ev_idx[:n].cpu().numpy().astype(np.int64)

    def _plant_rows(self, K):
        """the plant's _tvp / _p at the K loop times ahead: [K][n] each (one zero per row without such parameters)"""
        m = self.sim.model
        ts = [self.t_sim0 + (self.k + j) * self.dt_sim for j in range(K)]
        # (a copy per row: a tvp_fun / p_fun usually fills and returns one template)
        tv = np.array([np.array(self.sim.tvp_fun(s).master, dtype=float).reshape(-1) for s in ts]) if m.n_tvp else np.zeros((K, 1))
        pp = np.array([np.array(self.sim.p_fun(s).master, dtype=float).reshape(-1) for s in ts]) if m.n_p else np.zeros((K, 1))
        return tv, pp

    def _stats_host(self):
        return np.frombuffer(self.stats.cpu().numpy().tobytes(), dtype=STATS_DTYPE).copy()

    def step(self) -> dict:
        """one control step of all B loops; returns the inputs applied, the new states, the plant status, the law status, whether the
        step solved and - then - the solver statistics.  With settings.event_triggered also 'resolved': the members (int array, empty
        if none) that an event solved again at this step; they carry bit 4 in 'law_status', and 'stats' is there when there are any."""
        torch, m = self.torch, self.sim.model
        solved = self._due()
        if solved:
            self._solve()
        if self.k > 0 and (m.n_p or m.n_tvp):      # the plant's parameters at the current loop time (simulator.py:790-800)
            tv, pp = self._plant_rows(1)
            if m.n_p:
                self.p_plant.copy_(torch.from_numpy(np.ascontiguousarray(pp[0])).to(self.dev))
            if m.n_tvp:
                self.tvp_plant.copy_(torch.from_numpy(np.ascontiguousarray(tv[0])).to(self.dev))
        stream = self._stream()
        self.asmpc.make_step_batch_device(self.B, self.X.data_ptr(), self.Un.data_ptr(), self.lstat.data_ptr(), stream=stream)
        event = bool(self.asmpc.settings.event_triggered)
        # (on a step that has just solved the whole batch dx = 0: only a member whose solve failed there can be selected, and gets a
        #  second solve from the iterate the first one ended at)
        resolved = self._resolve_events(stream) if event else None
        self.U, self.Un = self.Un, self.U
        self.sim.step_batch_device(self.B, self.X.data_ptr(), self.U.data_ptr(), self.tvp_plant.data_ptr(), self.p_plant.data_ptr(),
                                   self.Xn.data_ptr(), 0, self.pstat.data_ptr(), shared_mask=2 | 4 | 8 | 16, stream=stream)
        self.X, self.Xn = self.Xn, self.X
        self.k += 1
        self._since += 1
        self._sync()
        out = {"u0": self.U.cpu().numpy(), "x": self.X.cpu().numpy(), "plant_status": (self.pstat.cpu().numpy() & 1),
               "law_status": self.lstat.cpu().numpy().copy(), "solved": solved}
        if event:
            out["law_status"][resolved] |= 16                 # bit 4: re-solved by an event at this step
            out["resolved"] = resolved
        if solved or (event and resolved.size):
            out["stats"] = self._stats_host()
        return out

    def _rollout(self, K):
        """K control steps between two solves in one launch; returns (x [K][B][nx], u [K][B][nu], plant status, law status)"""
        torch, m, B = self.torch, self.sim.model, self.B
        if m.n_z:
            raise NotImplementedError("BatchClosedLoopASMPC.run(fused=True): plants with algebraic states are not served by the rollout "
                                      "(run(n, fused=False) steps them)")
        tv, pp = self._plant_rows(K)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)      # noqa: E731
        tv, pp = up(tv), up(pp)
        Xt = torch.empty((K + 1, B, m.n_x), dtype=torch.float64, device=self.dev)
        Ut = torch.empty((K, B, m.n_u), dtype=torch.float64, device=self.dev)
        ps_, ls_ = (torch.zeros((K, B), dtype=torch.int32, device=self.dev) for _ in range(2))
        Xt[0].copy_(self.X)
        law = self.asmpc.law_record()
        self.sim.rollout_affine_device(B, K, law, Xt.data_ptr(), Ut.data_ptr(), tv.data_ptr(), pp.data_ptr(), ps_.data_ptr(), ls_.data_ptr(),
                                       stream=self._stream())
        self.X.copy_(Xt[K])
        self.U.copy_(Ut[K - 1])
        self.k += K
        self._since += K
        self._sync()
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
        xs, us, pst, lst, solve_steps, stats = [self.X.cpu().numpy().copy()[None]], [], [], [], [], []
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
                self._sync()
                solve_steps.append(i); stats.append(self._stats_host())
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
