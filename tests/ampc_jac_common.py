"""TEST-ONLY helpers of the tests of the network Jacobian (ApproxMPC.jacobian_batch, csrc/dompc_ampc.hip:dompc_ampc_jac_kernel): a numpy
float64 twin of the Jacobian in the network's scaled coordinates, the accuracy bound measured against torch's float32 autograd on the
CPU, and the checks the CPU (host emulation) and the GPU suite share, each with a `hostemu=` switch."""
import numpy as np
import torch

import ampc_common as ac
from do_mpc_amd.ampc import FeedforwardNN

_SLOPE64 = {"relu": lambda a: (a > 0).astype(np.float64), "tanh": lambda a: 1.0 - a * a, "leaky_relu": lambda a: np.where(a > 0, 1.0, 0.01),
            "sigmoid": lambda a: a * (1.0 - a), "linear": lambda a: np.ones_like(a)}


def twin_jacobian(state_dict, cfg, X, U_prev):
    """numpy float64 analytic Jacobian of the scaled network output with respect to the scaled input, [B][n_out][n_in]; like ac.twin
    it keeps the float32 rounding of the input and of xs"""
    h = ac.scaled_input(cfg, X, U_prev).astype(np.float64)
    T = np.broadcast_to(np.eye(h.shape[1]), (h.shape[0], h.shape[1], h.shape[1]))
    idx = sorted({int(k.split(".")[1]) for k in state_dict if k.endswith(".weight")})
    for n, i in enumerate(idx):
        W, b = (state_dict[f"layers.{i}.{w}"].detach().cpu().numpy().astype(np.float64) for w in ("weight", "bias"))
        last = n == len(idx) - 1 and cfg["n_hidden_layers"] > 0
        act = cfg["output_act_fn"] if last else cfg["act_fn"]
        h = ac._ACT64[act](h @ W.T + b)
        T = _SLOPE64[act](h)[:, :, None] * (W @ T)
    return T


def e_ref_jacobian(ampc, cfg, X, U_prev, Js):
    """the reference's own error: max |torch float32 CPU autograd Jacobian of FeedforwardNN at scaled_input - twin|"""
    net = FeedforwardNN(ampc.net.n_in, ampc.net.n_out, cfg["n_hidden_layers"], ampc.net.n_neurons, cfg["act_fn"], cfg["output_act_fn"])
    net.load_state_dict({k: v.detach().cpu() for k, v in ampc.net.state_dict().items()})
    xs = torch.from_numpy(ac.scaled_input(cfg, X, U_prev))
    J32 = torch.stack([torch.autograd.functional.jacobian(net, x) for x in xs]).numpy().astype(np.float64)
    return float(np.max(np.abs(J32 - Js)))


def full(ampc, r):
    """[B][n_u][n_in] of a jacobian_batch result"""
    return np.concatenate((r["du_dx"], r["du_du_prev"]), axis=2) if ampc.rterm else r["du_dx"]


def to_network_coordinates(cfg, J):
    """J[i][k] range[k] / (ubu - lbu)[i] (nothing without scaling)"""
    if not cfg["scaling"]:
        return J
    return J * (cfg["ub_in"] - cfg["lb_in"])[None, None, :] / (cfg["ubu"] - cfg["lbu"])[None, :, None]


def check_jacobian(ampc, X, U_prev, label=""):
    """The kernel's Jacobian, scaled back to the network's coordinates, against the twin within 8 max(E_ref_J, 2^-23 max|Js|); u of
    the same call = make_step_batch bit for bit, with and without clipping.  Returns (error, E_ref_J, bound, result)."""
    cfg = ac.cfg_of(ampc)
    m = ampc.mpc.model
    Js = twin_jacobian(ampc.net.state_dict(), cfg, X, U_prev)
    E = e_ref_jacobian(ampc, cfg, X, U_prev, Js)
    bound = 8.0 * max(E, 2.0 ** -23 * float(np.max(np.abs(Js))))
    r = ampc.jacobian_batch(X, U_prev)
    B = X.shape[0]
    assert set(r) == {"u", "du_dx", "du_du_prev"}
    assert r["du_dx"].shape == (B, m.n_u, m.n_x) and r["du_dx"].dtype == np.float64 and r["u"].shape == (B, m.n_u)
    if ampc.rterm:
        assert r["du_du_prev"].shape == (B, m.n_u, m.n_u) and r["du_du_prev"].dtype == np.float64
    else:
        assert r["du_du_prev"] is None
    J = to_network_coordinates(cfg, full(ampc, r))
    assert np.all(np.isfinite(J))
    err = float(np.max(np.abs(J - Js)))
    print(f"{label}: |J - twin| = {err:.3e}, E_ref_J = {E:.3e}, max|Js| = {np.max(np.abs(Js)):.3e}, bound = {bound:.3e}, "
          f"ratio to E_ref_J = {err / max(E, 1e-300):.2f}")
    assert err <= bound, (label, err, E, bound)
    for clip in (False, True):
        rc = r if not clip else ampc.jacobian_batch(X, U_prev, clip_to_bounds=True)
        assert np.array_equal(rc["u"], ampc.make_step_batch(X, U_prev, clip_to_bounds=clip)), (label, clip)
    return err, E, bound, r


def check_family(case, hostemu):
    nx, nu, rterm, st = case
    ampc = ac.network(nx, nu, rterm, hostemu, seed=3, **st)
    X, Up = ac.inputs(ampc, 33, seed=5)
    return check_jacobian(ampc, X, Up, ac.family_id(case))


def check_clipping(hostemu):
    """the stored network on inputs up to 1.5 x the box: clip_to_bounds=True gives the unclipped Jacobian with the rows of the clipped
    outputs set to zero, and nothing else changes"""
    ampc = ac.stored_cstr(hostemu)
    X, Up = ac.inputs(ampc, 257, seed=11, spread=1.5)
    lbu, ubu = np.asarray(ac.CSTR_BOX["lbu"]), np.asarray(ac.CSTR_BOX["ubu"])
    free = ampc.jacobian_batch(X, Up, clip_to_bounds=False)
    assert np.array_equal(free["u"], ampc.make_step_batch(X, Up, clip_to_bounds=False))
    outside = (free["u"] < lbu) | (free["u"] > ubu)
    assert outside.any() and not outside.all(), "choose inputs so that some outputs clip and some do not"
    clipped = ampc.jacobian_batch(X, Up, clip_to_bounds=True)
    assert np.array_equal(clipped["u"], ampc.make_step_batch(X, Up, clip_to_bounds=True))
    for key in ("du_dx", "du_du_prev"):
        assert np.all(free[key][~outside] != 0.0) or key == "du_du_prev"        # (the rows that stay carry a signal)
        assert np.array_equal(clipped[key], np.where(outside[:, :, None], 0.0, free[key])), key
    return int(outside.sum())


def check_position_independence(hostemu):
    """equal samples give bitwise equal Jacobians wherever they sit in the batch and in the wavefront"""
    ampc = ac.network(4, 2, True, hostemu, seed=3, n_hidden_layers=1, n_neurons=32, act_fn="tanh", output_act_fn="linear")
    X, Up = ac.inputs(ampc, 97, seed=8)
    rows = [0, 31, 32, 63, 64, 96]
    X[rows], Up[rows] = X[5], Up[5]
    J = full(ampc, ampc.jacobian_batch(X, Up))
    for r in rows:
        assert np.array_equal(J[r], J[5])
    assert len({J[r].tobytes() for r in range(97)}) == 97 - len(rows)          # (the other rows differ)


def check_weight_refresh(hostemu):
    """the Jacobian after an in-place change of one weight, and after an optimiser step, is that of the new weights"""
    ampc = ac.stored_cstr(hostemu)
    X, Up = ac.inputs(ampc, 33, seed=4)
    before = full(ampc, ampc.jacobian_batch(X, Up))
    with torch.no_grad():
        ampc.net.layers[2].weight[1, 7] += 0.25
    err, E, bound, r = check_jacobian(ampc, X, Up, "after the in-place change")
    after = full(ampc, r)
    assert np.array_equal(after[:, 0], before[:, 0]) and not np.array_equal(after[:, 1], before[:, 1])
    cfg = ac.cfg_of(ampc)
    assert np.max(np.abs(to_network_coordinates(cfg, after - before))) > 100 * bound
    opt = torch.optim.SGD(ampc.net.parameters(), lr=0.1)
    loss = ampc.net(torch.from_numpy(ac.scaled_input(cfg, X, Up))).square().sum()
    loss.backward()
    opt.step()
    _, _, bound, r = check_jacobian(ampc, X, Up, "after optimizer.step()")
    assert np.max(np.abs(to_network_coordinates(cfg, full(ampc, r) - after))) > 100 * bound


def check_no_rterm(hostemu, buffers):
    """without an rterm du_du_prev is None, and the device-pointer entry takes null pointers for u_prev and du_du_prev.
    `buffers(arrays) -> (addresses, read)`: the arrays on the side the entry reads (host emulation: the host)"""
    ampc = ac.network(4, 2, False, hostemu, seed=3, n_hidden_layers=0, n_neurons=2, act_fn="tanh", output_act_fn="linear")
    X, Up = ac.inputs(ampc, 33, seed=5)
    assert Up is None
    err, E, bound, r = check_jacobian(ampc, X, None, "no rterm")
    assert r["du_du_prev"] is None
    (px, pu, pj), read = buffers([X, np.full((33, 2), np.nan), np.full((33, 2, 4), np.nan)])
    ampc.jacobian_batch_device(33, px, 0, pu, pj, 0)
    _, U, J = read()
    assert np.array_equal(U, r["u"]) and np.array_equal(J, r["du_dx"])


def host_buffers(arrays):
    """`buffers` of check_no_rterm on the host emulation, whose device is the host"""
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]
    return [a.ctypes.data for a in arrays], lambda: arrays
