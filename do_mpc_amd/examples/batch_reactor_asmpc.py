"""Sensitivity-based approximate MPC for B loops at once: the controller of the reference's examples/batch_reactor_differentiator
(/root/reference/examples/batch_reactor_differentiator/main.py:87-177, class ASMPC) on top of `MPC.make_step_batch(..., sensitivities=True)`.

Between two solves the optimal input is continued to first order in the state,

    u ~ (I - G)^-1 (u0 + J (x - x_prev) - G u0),      J = du0/dx0, G = du0/du_prev at the last solution (main.py:170-172),

x_prev the states the batch was last solved at and u0 its inputs.  The reference differentiates the one solution stored in the
controller; here `solve` solves and differentiates B problems in two device calls and `make_step_batch` is B small matrix products.
The model and the controller are those of examples/batch_reactor.py."""
import numpy as np

from . import batch_reactor

X0 = batch_reactor.X0
build_model = batch_reactor.build_model
build_mpc = batch_reactor.build_mpc


class ASMPC:
    def __init__(self, mpc):
        self.mpc = mpc
        self.last = None                 # result of the last solve: x_prev, u0, du0dx0, du0du_prev, ok

    def solve(self, X0, U_prev=None) -> dict:
        """B cold solves at the states X0 [B, n_x] with their sensitivities; the expansion point of `make_step_batch` from now on"""
        r = self.mpc.make_step_batch(X0, U_prev=U_prev, sensitivities=True)
        self.last = {"x_prev": np.asarray(X0, float).reshape(-1, self.mpc.model.n_x).copy(), "u0": r["u0"].copy(),
                     "du0dx0": r["du0dx0"].copy(), "du0du_prev": r["du0du_prev"].copy(), "ok": r["ok"].copy()}
        return r

    def make_step_batch(self, X) -> np.ndarray:
        """inputs [B, n_u] for the states X [B, n_x] from the last solve; NaN rows for the loops whose solve or sensitivities failed"""
        if self.last is None:
            raise RuntimeError("ASMPC.make_step_batch: no solution to expand about (call solve first)")
        L = self.last
        X = np.asarray(X, float).reshape(L["x_prev"].shape)
        J, G, u0 = L["du0dx0"], L["du0du_prev"], L["u0"]
        rhs = u0 + np.einsum("bij,bj->bi", J, X - L["x_prev"]) - np.einsum("bij,bj->bi", G, u0)
        A = np.eye(u0.shape[1])[None] - G
        U = np.full_like(u0, np.nan)
        ok = L["ok"] & np.all(np.isfinite(A.reshape(len(A), -1)), axis=1)
        if ok.any():
            U[ok] = np.linalg.solve(A[ok], rhs[ok][:, :, None])[:, :, 0]
        return U
