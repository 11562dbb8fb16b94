"""Approximate MPC on the host emulation of csrc/dompc_ampc.hip (g++ -DDOMPC_HOST_EMU): the step against the float64 twin within the
bound measured on the reference's own arithmetic (tests/ampc_common.py), the shape family, the kernel's limits, the reference's
make_step semantics and file formats, the trainer, the weight refresh and the resident closed loop.  No GPU, no solver."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import ampc_common as ac
import hostemu
from do_mpc_amd.ampc import ApproxMPC, FeedforwardNN, Trainer


@pytest.fixture(scope="module")
def cstr_mpc():
    """the controller of examples/cstr_ampc.py, built on the host emulation of the solver"""
    from do_mpc_amd.examples import cstr_ampc as ex
    with hostemu.patched():
        return ex.build_mpc(ex.build_model())


def test_stored_network_on_the_cstr_controller(cstr_mpc):
    ampc, err, E = ac.check_stored(hostemu=True, mpc=cstr_mpc)
    assert ampc.rterm and ampc.net.n_in == 6


@pytest.mark.parametrize("case", ac.FAMILY, ids=[ac.family_id(c) for c in ac.FAMILY])
def test_shape_family(case):
    ac.check_family(case, hostemu=True)


@pytest.mark.parametrize("nx, nu, settings, text", [
    (4, 2, dict(n_neurons=129), "n_neurons = 129"), (65, 2, {}, "n_in = 65"), (4, 33, {}, "n_out = 33"),
    (4, 2, dict(n_hidden_layers=9), "n_hidden_layers = 9")])
def test_networks_beyond_the_limits_are_refused_by_name(nx, nu, settings, text):
    ampc = ApproxMPC(ac.stub_mpc(nx, nu, False))
    for k, v in settings.items():
        setattr(ampc.settings, k, v)
    with pytest.raises(NotImplementedError, match=text):
        ac.setup_ampc(ampc, hostemu=True)


def test_unknown_activation_raises_the_references_error():
    for key in ("act_fn", "output_act_fn"):
        ampc = ApproxMPC(ac.stub_mpc(4, 2, False))
        setattr(ampc.settings, key, "gelu")
        with pytest.raises(ValueError, match="Activation function not implemented."):
            ac.setup_ampc(ampc, hostemu=True)
    with pytest.raises(ValueError, match="Activation function not implemented."):
        FeedforwardNN(4, 2, 1, 8, "linear", "linear")


def test_make_step_is_the_batch_of_one_and_iterates_u0():
    ampc = ac.check_make_step(hostemu=True)
    with pytest.raises(AssertionError, match="x0 must be a numpy array"):
        ampc.make_step([0.5, 0.5, 100.0, 100.0])
    with pytest.raises(AssertionError, match="u_prev must be a numpy array or None"):
        ampc.make_step(np.ones((4, 1)), u_prev=[5.0, 0.0])
    with pytest.raises(AssertionError, match="Setup can only be once."):
        ampc.setup()
    with pytest.raises(AssertionError, match="MPC was not setup yet. Please call ApproxMPC.setup()."):
        ApproxMPC(ac.stub_mpc(4, 2, True)).make_step(np.ones((4, 1)))


@pytest.mark.parametrize("which, text", [
    ("lbx", "There are missing lower bounds for state variables that are required for clipping and scaling."),
    ("ubx", "There are missing upper bounds for state variables that are required for clipping and scaling."),
    ("lbu", "There are missing lower bounds for input variables that are required for clipping and scaling."),
    ("ubu", "There are missing upper bounds for input variables that are required for clipping and scaling.")])
def test_infinite_bounds_raise_the_references_assertions(which, text):
    ampc = ApproxMPC(ac.stub_mpc(4, 2, True))
    getattr(ampc.settings, which)[1] = np.inf if which[0] == "u" else -np.inf
    with pytest.raises(AssertionError, match=text):
        ac.setup_ampc(ampc, hostemu=True)


def test_cstr_controller_without_the_references_box_lacks_a_bound(cstr_mpc):
    """examples/cstr.py bounds T_R by a soft constraint: the box of the reference's template has to be set (examples/cstr_ampc.py:box)"""
    with pytest.raises(AssertionError, match="missing upper bounds for state variables"):
        ApproxMPC(cstr_mpc).setup()


def test_pinned_hashes_are_those_of_the_shape_headers():
    """tests/golden/ampc_template_hashes.json pins the generated shape headers (sizes, activations, scaling) of the stored network and
    of the default network - not the kernel text, which every build digests by itself"""
    from do_mpc_amd import lowering
    pinned = json.load(open(os.path.join(ac.GOLDEN, "ampc_template_hashes.json")))
    for key, shape in (("stored_cstr_network", (6, 2, 1, 50, "tanh", "linear", True)), ("default_network", (6, 2, 3, 50, "tanh", "linear", True))):
        assert lowering.lower_ampc(*shape).rsplit('AMPC_MODEL_HASH "', 1)[1].split('"')[0] == pinned[key]
    # without a hidden layer output_act_fn is not used: the same header whatever it names
    assert lowering.lower_ampc(4, 2, 0, 2, "tanh", "linear", True).split("\n#define AMPC_MODEL_HASH")[0].replace("(linear)", "(relu)") == \
        lowering.lower_ampc(4, 2, 0, 2, "tanh", "relu", True).split("\n#define AMPC_MODEL_HASH")[0]


class _Plain(torch.nn.Module):
    """a module with the reference's slot layout, written out independently of do_mpc_amd.ampc: linear layers on the even slots of
    `layers`, activation layers on the odd ones, none behind a linear output"""

    def __init__(self, sizes, act, out_act):
        super().__init__()
        slots = []
        for k, (a, b) in enumerate(zip(sizes[:-1], sizes[1:])):
            slots.append(torch.nn.Linear(a, b))
            last = k == len(sizes) - 2
            if not last or out_act is not None:
                slots.append((out_act if last else act)())
        self.layers = torch.nn.ModuleList(slots)

    def forward(self, x):
        return torch.nn.Sequential(*self.layers)(x)


def test_state_dicts_load_on_either_side(tmp_path):
    ours = ac.network(4, 2, True, hostemu=True, n_hidden_layers=3, n_neurons=20, act_fn="tanh", output_act_fn="sigmoid")
    assert list(ours.net.state_dict()) == [f"layers.{i}.{w}" for i in (0, 2, 4, 6) for w in ("weight", "bias")]
    ours.save_to_state_dict(tmp_path / "ours.pth")
    plain = _Plain([6, 20, 20, 20, 2], torch.nn.Tanh, torch.nn.Sigmoid)
    plain.load_state_dict(torch.load(tmp_path / "ours.pth", weights_only=True), strict=True)
    x = torch.rand(7, 6)
    assert torch.equal(plain(x), ours.predict(x))
    other = _Plain([6, 20, 20, 20, 2], torch.nn.Tanh, torch.nn.Sigmoid)
    torch.save(other.state_dict(), tmp_path / "theirs.pth")
    ours.load_from_state_dict(tmp_path / "theirs.pth")
    assert torch.equal(other(x), ours.predict(x))
    # a "linear" output adds no layer; the stored reference file loads strictly
    net = FeedforwardNN(6, 2, 1, 50, "tanh", "linear")
    assert len(net.layers) == 3
    net.load_state_dict(torch.load(ac.STORED, weights_only=True), strict=True)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {
        "layers.0.weight": (50, 6), "layers.0.bias": (50,), "layers.2.weight": (2, 50), "layers.2.bias": (2,)}


# ---------------------------------------------------------------------------------------------- trainer
K_LAW = np.array([[0.8, -0.5, 0.01, -0.02], [30.0, 100.0, -0.3, 0.5]])


def _dataset(tmp_path, name="law", n=512):
    """data_<name>_opt.pkl the way AMPCSampler writes it: a table of columns x0, u_prev, u0 (column vectors) and status"""
    import pandas as pd
    rng = np.random.default_rng(0)
    box = ac.CSTR_BOX
    rows = []
    for _ in range(n):
        x0 = rng.uniform(box["lbx"], box["ubx"]).reshape(-1, 1)
        u_prev = rng.uniform(box["lbu"], box["ubu"]).reshape(-1, 1)
        u0 = np.clip(K_LAW @ x0 + np.array([[20.0], [-4000.0]]), np.reshape(box["lbu"], (-1, 1)), np.reshape(box["ubu"], (-1, 1)))
        rows.append({"x0": x0, "u_prev": u_prev, "u0": u0, "status": True})
    d = tmp_path / "sampling" / name
    d.mkdir(parents=True)
    pd.DataFrame(rows).to_pickle(d / f"data_{name}_opt.pkl")
    with open(d / f"data_{name}_opt.pkl", "rb") as f:
        assert len(pickle.load(f)) == n
    return name


def _trainer(tmp_path, ampc, name, n_epochs):
    tr = Trainer(ampc)
    st = tr.settings
    st.dataset_name, st.n_epochs, st.batch_size = name, n_epochs, 128
    st.data_dir, st.results_dir = str(tmp_path / "sampling"), str(tmp_path / "training")
    return tr


def test_trainer_learns_a_known_law_and_writes_the_references_files(tmp_path):
    name = _dataset(tmp_path)
    torch.manual_seed(42)
    ampc = ApproxMPC(ac.stub_mpc(4, 2, True, **ac.CSTR_BOX))
    ampc.settings.n_hidden_layers, ampc.settings.n_neurons = 1, 50
    ac.setup_ampc(ampc, hostemu=True)
    X, Up = ac.inputs(ampc, 33, seed=9)
    before = ampc.make_step_batch(X, Up)
    tr = _trainer(tmp_path, ampc, name, 30)
    tr.settings.save_history = True
    tr.setup()
    tr.generator.manual_seed(42)
    tr.default_training()
    h = tr.history
    assert set(h) == {"epoch", "train_loss", "lr", "val_loss"} and h["epoch"] == list(range(30))
    print(f"validation loss {h['val_loss'][0]:.3e} -> {h['val_loss'][-1]:.3e}")
    assert h["val_loss"][-1] < 0.5 * h["val_loss"][0]
    res = tmp_path / "training" / f"results_{name}"
    assert sorted(os.listdir(res)) == ["approx_mpc.pth", "hyperparameters.json", "training_history.json"]
    assert json.load(open(res / "training_history.json")) == h
    hp = json.load(open(res / "hyperparameters.json"))
    assert set(hp) == set(json.load(open(os.path.join(ac.GOLDEN, "ampc_reference_cstr_hyperparameters.json"))))
    sd = torch.load(res / "approx_mpc.pth", weights_only=True)
    assert all(torch.equal(v, ampc.net.state_dict()[k].cpu()) for k, v in sd.items())
    # the step after the training runs the trained weights
    ac.check_step(ampc, X, Up, "after training")
    assert not np.array_equal(before, ampc.make_step_batch(X, Up))


def test_scheduler_reduces_the_learning_rate_on_a_plateau(tmp_path):
    name = _dataset(tmp_path, n=64)
    ampc = ac.network(4, 2, True, hostemu=True, box=ac.CSTR_BOX, n_hidden_layers=1, n_neurons=8)
    tr = _trainer(tmp_path, ampc, name, 8)
    tr.settings.scheduler_flag = True
    tr.scheduler_settings.patience = 2
    tr.setup()
    tr.validation_epoch = lambda loader: 1.0                   # a loss that never improves
    tr.default_training()
    lr = tr.history["lr"]
    assert lr[0] == tr.settings.learning_rate and min(lr) < lr[0]
    first = next(v for v in lr if v < lr[0])
    assert first == pytest.approx(lr[0] * tr.scheduler_settings.factor, rel=1e-12)
    assert tr.lr_scheduler.min_lrs == [pytest.approx(tr.scheduler_settings.min_lr * 0.1)]


def test_figures_fail_by_name_without_matplotlib(tmp_path, monkeypatch):
    import builtins
    real = builtins.__import__

    def no_matplotlib(name, *a, **k):
        if name.startswith("matplotlib"):
            raise ImportError("No module named 'matplotlib'")
        return real(name, *a, **k)
    name = _dataset(tmp_path, n=64)
    ampc = ac.network(4, 2, True, hostemu=True, box=ac.CSTR_BOX, n_hidden_layers=1, n_neurons=8)
    tr = _trainer(tmp_path, ampc, name, 1)
    tr.settings.save_fig = True
    tr.setup()
    monkeypatch.setattr(builtins, "__import__", no_matplotlib)
    with pytest.raises(ImportError, match="matplotlib is required"):
        tr.default_training()


def test_a_step_after_a_weight_change_uses_the_new_weights():
    ac.check_weight_refresh(hostemu=True)


def test_batch_closed_loop_of_copies_is_the_single_loop():
    ac.check_closed_loop(hostemu=True)
