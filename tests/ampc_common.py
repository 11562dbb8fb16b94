"""TEST-ONLY helpers of the approximate-MPC tests: the host emulation of csrc/dompc_ampc.hip (g++ -DDOMPC_HOST_EMU, the text that
ships), a numpy float64 twin of one step, the accuracy bound measured against the reference's own arithmetic, and the checks the CPU
and the GPU suite share (each with a `hostemu=` switch)."""
import os
from types import SimpleNamespace

import numpy as np
import torch

from ampc_hostemu import ampc_hostemu_library
from do_mpc_amd.ampc import ApproxMPC, FeedforwardNN

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STORED = os.path.join(GOLDEN, "ampc_reference_cstr.pt")

# the box of the reference's CSTR_approximate_mpc/template_mpc.py
CSTR_BOX = dict(lbx=[0.1, 0.1, 50.0, 50.0], ubx=[2.0, 2.0, 140.0, 140.0], lbu=[5.0, -8500.0], ubu=[100.0, 0.0])


def setup_ampc(ampc, hostemu):
    """ampc.setup() on the host-emulated kernel or on the GPU"""
    if hostemu:
        ampc.setup(_lib_path=ampc_hostemu_library, _code_object="")
    else:
        ampc.setup()
    return ampc


def setup_ampc_with(setup, ampc):
    """an un-patched ApproxMPC.setup (`setup`) on the host emulation"""
    return setup(ampc, _lib_path=ampc_hostemu_library, _code_object="")


def stub_mpc(nx, nu, rterm, lbx=None, ubx=None, lbu=None, ubu=None):
    """what ApproxMPC reads of a controller: the model's sizes, the bounds, flags['set_rterm'], x0 / u0"""
    f = lambda v, n, d: np.full(n, d) if v is None else np.asarray(v, float)      # noqa: E731
    return SimpleNamespace(model=SimpleNamespace(n_x=nx, n_u=nu), _x_lb=f(lbx, nx, -1.0), _x_ub=f(ubx, nx, 3.0), _u_lb=f(lbu, nu, -2.0),
                           _u_ub=f(ubu, nu, 5.0), flags={"set_rterm": bool(rterm)}, x0=np.zeros(nx), u0=np.zeros(nu))


def network(nx, nu, rterm, hostemu, seed=0, box=None, **settings):
    """an ApproxMPC on a stub controller with torch's initial weights under `seed`; the biases are drawn from [-0.5, 0.5] too, so that
    a lost bias shows"""
    ampc = ApproxMPC(stub_mpc(nx, nu, rterm, **(box or {})))
    for k, v in settings.items():
        setattr(ampc.settings, k, v)
    g = torch.Generator().manual_seed(seed)
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        setup_ampc(ampc, hostemu)
    with torch.no_grad():
        for name, p in ampc.net.named_parameters():
            if name.endswith("bias"):
                p.copy_(torch.rand(p.shape, generator=g) - 0.5)
    return ampc


def stored_cstr(hostemu, mpc=None):
    """the reference's stored trained network (tests/golden/ampc_reference_cstr.pt: one hidden layer of 50, tanh) on the CSTR box"""
    ampc = ApproxMPC(mpc if mpc is not None else stub_mpc(4, 2, True, **CSTR_BOX))
    ampc.settings.n_hidden_layers, ampc.settings.n_neurons = 1, 50
    if mpc is not None:
        ampc.settings.ubx = np.asarray(CSTR_BOX["ubx"], float).reshape(-1, 1)
    setup_ampc(ampc, hostemu)
    ampc.load_from_state_dict(STORED)
    return ampc


def cfg_of(ampc):
    st = ampc.settings
    lb, ub, lbu, ubu = ampc._box()
    return dict(act_fn=st.act_fn, output_act_fn=st.output_act_fn, n_hidden_layers=st.n_hidden_layers, scaling=st.scaling, lb_in=lb, ub_in=ub,
                lbu=lbu, ubu=ubu)


def inputs(ampc, B, seed=1, spread=1.0):
    """B samples uniform in the bounds box (spread > 1: beyond it) -> (X, U_prev or None)"""
    rng = np.random.default_rng(seed)
    m = ampc.mpc.model
    lb, ub, lbu, ubu = ampc._box()
    mid, half = (lb + ub) / 2, (ub - lb) / 2 * spread
    Z = rng.uniform(mid - half, mid + half, (B, lb.size))
    return np.ascontiguousarray(Z[:, :m.n_x]), (np.ascontiguousarray(Z[:, m.n_x:]) if ampc.rterm else None)


# ---------------------------------------------------------------------------------------------- the twin
_ACT64 = {"relu": lambda v: np.maximum(v, 0.0), "tanh": np.tanh, "leaky_relu": lambda v: np.where(v > 0, v, 0.01 * v),
          "sigmoid": lambda v: 1.0 / (1.0 + np.exp(-v)), "linear": lambda v: v}


def scaled_input(cfg, X, U_prev):
    """xs = f32((f64(f32(x)) - shift) / range), the reference's promotions"""
    Z = X if U_prev is None else np.concatenate((X, U_prev), axis=1)
    z32 = np.asarray(Z, np.float64).astype(np.float32)
    if not cfg["scaling"]:
        return z32
    return ((z32.astype(np.float64) - cfg["lb_in"]) / (cfg["ub_in"] - cfg["lb_in"])).astype(np.float32)


def twin(state_dict, cfg, X, U_prev, clip=False):
    """numpy float64 evaluation of one step: the float32 rounding of the input and of xs kept, the network in float64 ->
    (ys, u): the scaled network output and the (rescaled, optionally clipped) input"""
    h = scaled_input(cfg, X, U_prev).astype(np.float64)
    idx = sorted({int(k.split(".")[1]) for k in state_dict if k.endswith(".weight")})
    for n, i in enumerate(idx):
        W, b = (state_dict[f"layers.{i}.{w}"].detach().cpu().numpy().astype(np.float64) for w in ("weight", "bias"))
        last = n == len(idx) - 1 and cfg["n_hidden_layers"] > 0
        h = _ACT64[cfg["output_act_fn"] if last else cfg["act_fn"]](h @ W.T + b)
    u = h * (cfg["ubu"] - cfg["lbu"]) + cfg["lbu"] if cfg["scaling"] else h.copy()
    if clip:
        u = np.minimum(np.maximum(u, cfg["lbu"]), cfg["ubu"])
    return h, u


def e_ref(ampc, cfg, X, U_prev, ys):
    """the reference's own error: max |torch float32 CPU forward - twin| on the scaled output, same weights and inputs"""
    with torch.no_grad():
        net = FeedforwardNN(ampc.net.n_in, ampc.net.n_out, cfg["n_hidden_layers"], ampc.net.n_neurons, cfg["act_fn"], cfg["output_act_fn"])
        net.load_state_dict({k: v.detach().cpu() for k, v in ampc.net.state_dict().items()})
        y32 = net(torch.from_numpy(scaled_input(cfg, X, U_prev))).numpy().astype(np.float64)
    return float(np.max(np.abs(y32 - ys)))


def check_step(ampc, X, U_prev, label=""):
    """The kernel's scaled output against the twin within 8 max(E_ref, 2^-23 max|ys|), u relative to ubu - lbu within the same bound,
    and clip_to_bounds=True = the clipped unclipped result, exactly.  Returns (error, E_ref, bound, U clipped)."""
    cfg = cfg_of(ampc)
    ys, u = twin(ampc.net.state_dict(), cfg, X, U_prev)
    E = e_ref(ampc, cfg, X, U_prev, ys)
    bound = 8.0 * max(E, 2.0 ** -23 * float(np.max(np.abs(ys))))
    U = ampc.make_step_batch(X, U_prev, clip_to_bounds=False)
    assert U.shape == u.shape and U.dtype == np.float64 and np.all(np.isfinite(U))
    rng = (cfg["ubu"] - cfg["lbu"]) if cfg["scaling"] else np.ones_like(cfg["lbu"])
    err_u = float(np.max(np.abs(U - u) / rng))
    err_ys = float(np.max(np.abs(((U - cfg["lbu"]) / rng if cfg["scaling"] else U) - ys)))
    print(f"{label}: |ys - twin| = {err_ys:.3e}, |u - twin| / (ubu - lbu) = {err_u:.3e}, E_ref = {E:.3e}, bound = {bound:.3e}, "
          f"ratio to E_ref = {err_ys / max(E, 1e-300):.2f}")
    assert err_ys <= bound and err_u <= bound, (label, err_ys, err_u, E, bound)
    Uc = ampc.make_step_batch(X, U_prev, clip_to_bounds=True)
    assert np.array_equal(Uc, np.minimum(np.maximum(U, cfg["lbu"]), cfg["ubu"]))
    return err_ys, E, bound, Uc


# ---------------------------------------------------------------------------------------------- the shape family
# (n_x, n_u, rterm, settings): every hidden and output activation, 0 / 1 / 3 / 8 hidden layers, 1 ... 128 neurons around the tile of 32,
# n_in 1 / 6 / 64, n_out 1 / 2 / 32, scaling on and off, with and without rterm; sigmoid with 33 neurons: live padded neurons show
FAMILY = [
    (4, 2, True, dict(n_hidden_layers=1, n_neurons=50, act_fn="tanh", output_act_fn="linear")),
    (4, 2, True, dict(n_hidden_layers=3, n_neurons=50, act_fn="tanh", output_act_fn="linear")),
    (4, 2, True, dict(n_hidden_layers=1, n_neurons=1, act_fn="tanh", output_act_fn="linear")),
    (4, 2, True, dict(n_hidden_layers=1, n_neurons=32, act_fn="relu", output_act_fn="linear")),
    (4, 2, True, dict(n_hidden_layers=3, n_neurons=33, act_fn="sigmoid", output_act_fn="sigmoid")),
    (4, 2, True, dict(n_hidden_layers=3, n_neurons=128, act_fn="leaky_relu", output_act_fn="tanh")),
    (4, 2, False, dict(n_hidden_layers=0, n_neurons=2, act_fn="tanh", output_act_fn="linear")),
    (4, 2, True, dict(n_hidden_layers=8, n_neurons=50, act_fn="tanh", output_act_fn="linear", scaling=False)),
    (32, 32, True, dict(n_hidden_layers=3, n_neurons=65, act_fn="tanh", output_act_fn="relu")),
    # host emulation only (the GPU suite keeps to the prebuilt objects above)
    (4, 2, True, dict(n_hidden_layers=1, n_neurons=31, act_fn="leaky_relu", output_act_fn="leaky_relu")),
    (4, 2, True, dict(n_hidden_layers=3, n_neurons=64, act_fn="relu", output_act_fn="linear")),
    (1, 1, False, dict(n_hidden_layers=1, n_neurons=33, act_fn="sigmoid", output_act_fn="linear")),
    (5, 1, True, dict(n_hidden_layers=3, n_neurons=50, act_fn="tanh", output_act_fn="linear", scaling=False)),
    (64, 32, False, dict(n_hidden_layers=1, n_neurons=128, act_fn="tanh", output_act_fn="linear")),
    (1, 1, False, dict(n_hidden_layers=0, n_neurons=1, act_fn="sigmoid", output_act_fn="linear")),
]
N_PREBUILT = 9                # FAMILY[:N_PREBUILT] = the shapes of __graft_entry__.PREBUILT_AMPC


def family_id(case):
    nx, nu, rterm, st = case
    return (f"{nx + (nu if rterm else 0)}-{nu}-{st['n_hidden_layers']}x{st['n_neurons']}-{st['act_fn']}-{st['output_act_fn']}"
            f"{'' if st.get('scaling', True) else '-unscaled'}{'' if rterm else '-no_rterm'}")


def family_shape(case):
    """the arguments of lowering.lower_ampc of a family member"""
    nx, nu, rterm, st = case
    return (nx + (nu if rterm else 0), nu, st["n_hidden_layers"], st["n_neurons"], st["act_fn"], st["output_act_fn"], st.get("scaling", True))


def check_family(case, hostemu):
    nx, nu, rterm, st = case
    ampc = network(nx, nu, rterm, hostemu, seed=3, **st)
    X, Up = inputs(ampc, 33, seed=5)
    return check_step(ampc, X, Up, family_id(case))


# ---------------------------------------------------------------------------------------------- shared checks
def check_stored(hostemu, mpc=None):
    """the stored network on the CSTR box, B = 257 with U_prev; inputs up to 1.5 x the box so that rows clip"""
    ampc = stored_cstr(hostemu, mpc)
    X, Up = inputs(ampc, 257, seed=11, spread=1.5)
    err, E, bound, Uc = check_step(ampc, X, Up, "stored CSTR network")
    lbu, ubu = np.asarray(CSTR_BOX["lbu"]), np.asarray(CSTR_BOX["ubu"])
    U = ampc.make_step_batch(X, Up, clip_to_bounds=False)
    below, above = U < lbu, U > ubu
    assert below.any() or above.any(), "choose inputs so that at least one row clips"
    assert np.all(Uc[below] == np.broadcast_to(lbu, U.shape)[below]) and np.all(Uc[above] == np.broadcast_to(ubu, U.shape)[above])
    assert np.all((Uc >= lbu) & (Uc <= ubu))
    return ampc, err, E


def check_make_step(hostemu):
    """make_step = row 0 of make_step_batch bit for bit; u0 is stored and reused as u_prev; an explicit u_prev overrides it"""
    ampc = stored_cstr(hostemu)
    X, Up = inputs(ampc, 3, seed=2)
    ref = ampc.make_step_batch(X, Up)
    ampc.u0 = Up[0].reshape(-1, 1)
    u = ampc.make_step(X[0].reshape(-1, 1))
    assert u.shape == (2, 1) and np.array_equal(u.ravel(), ref[0])
    assert np.array_equal(np.asarray(ampc.u0).ravel(), ref[0])
    u2 = ampc.make_step(X[1].reshape(-1, 1))                   # u_prev = the stored u0 of the step before
    assert np.array_equal(u2.ravel(), ampc.make_step_batch(X[1:2], ref[0:1])[0])
    u3 = ampc.make_step(X[2].reshape(-1, 1), u_prev=Up[2].reshape(-1, 1))
    assert np.array_equal(u3.ravel(), ref[2])
    ampc.step_return_type = "torch"
    ut = ampc.make_step(X[2].reshape(-1, 1), u_prev=Up[2].reshape(-1, 1))
    assert torch.is_tensor(ut) and np.array_equal(ut.numpy().ravel(), ref[2])
    return ampc


def check_weight_refresh(hostemu):
    """a step after an in-place change of one weight uses the new weights"""
    ampc = stored_cstr(hostemu)
    X, Up = inputs(ampc, 33, seed=4)
    before = ampc.make_step_batch(X, Up, clip_to_bounds=False)
    with torch.no_grad():
        ampc.net.layers[2].weight[1, 7] += 0.25
    err, E, bound, _ = check_step(ampc, X, Up, "after the in-place change")
    after = ampc.make_step_batch(X, Up, clip_to_bounds=False)
    assert np.max(np.abs(after - before)[:, 1]) / 8500.0 > 100 * bound and np.array_equal(after[:, 0], before[:, 0])
    opt = torch.optim.SGD(ampc.net.parameters(), lr=0.1)       # ... and after an optimiser step
    loss = ampc.net(torch.from_numpy(scaled_input(cfg_of(ampc), X, Up))).square().sum()
    loss.backward()
    opt.step()
    check_step(ampc, X, Up, "after optimizer.step()")


def check_closed_loop(hostemu, n_steps=10, B=5):
    """B copies of one start give B identical trajectories = the single loop ampc.make_step -> simulator.make_step"""
    from do_mpc_amd.closed_loop import BatchClosedLoopAMPC
    from do_mpc_amd.examples import cstr_ampc as ex
    from lqr_common import plant_on
    model = ex.build_model()
    ampc = stored_cstr(hostemu)
    sim = plant_on(ex.build_simulator(model, setup=False), hostemu)
    sim.x0 = ex.X0
    ampc.u0 = ex.U0.reshape(-1, 1)
    loop = BatchClosedLoopAMPC(ampc, sim, np.tile(ex.X0, (B, 1)), device="cpu" if hostemu else 0)
    rec = loop.run(n_steps)
    assert rec["x"].shape == (n_steps + 1, B, 4) and rec["u"].shape == (n_steps, B, 2) and not rec["plant_status"].any()
    for b in range(1, B):
        assert np.array_equal(rec["x"][:, b], rec["x"][:, 0]) and np.array_equal(rec["u"][:, b], rec["u"][:, 0])
    x0 = ex.X0.reshape(-1, 1)
    for k in range(n_steps):
        u0 = ampc.make_step(x0)
        x0 = sim.make_step(u0)
        assert np.array_equal(u0.ravel(), rec["u"][k, 0]) and np.array_equal(np.asarray(x0).ravel(), rec["x"][k + 1, 0])
    return rec
