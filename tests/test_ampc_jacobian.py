"""The batched network Jacobian (ApproxMPC.jacobian_batch) on the host emulation of csrc/dompc_ampc.hip, and Sobolev training
(TrainerSettings.sobolev_weight, Trainer.sensitivity_error) on a synthetic data file with exact Jacobian labels.  No GPU, no solver."""
import numpy as np
import pytest
import torch

import ampc_common as ac
import ampc_jac_common as jc
from do_mpc_amd.ampc import ApproxMPC, Trainer, network_jacobian


# ---------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("case", ac.FAMILY, ids=[ac.family_id(c) for c in ac.FAMILY])
def test_shape_family(case):
    jc.check_family(case, hostemu=True)


def test_u_of_the_jacobian_call_is_the_step_and_clipped_rows_are_zero():
    assert jc.check_clipping(hostemu=True) > 0


def test_equal_inputs_give_equal_jacobians_wherever_they_sit():
    jc.check_position_independence(hostemu=True)


def test_the_jacobian_after_a_weight_change_is_that_of_the_new_weights():
    jc.check_weight_refresh(hostemu=True)


def test_without_rterm_du_du_prev_is_none_and_null_pointers_are_accepted():
    jc.check_no_rterm(True, jc.host_buffers)


def test_u_prev_is_required_with_an_rterm():
    ampc = ac.stored_cstr(hostemu=True)
    with pytest.raises(ValueError, match="U_prev is required"):
        ampc.jacobian_batch(np.ones((3, 4)))


# ---------------------------------------------------------------------------------------------- the trainer
K_LAW = np.array([[0.8, -0.5, 0.6, -0.4, 0.3, 0.2], [-0.6, 0.9, -0.3, 0.5, -0.2, 0.4]])


def _law(Z):
    """a smooth saturated feedback on the CSTR box, lbu + (ubu - lbu) (0.5 + 0.5 tanh(2 (z - mid) K^T)) with z = the input scaled to
    [0, 1], and its exact Jacobian in physical units -> (u [N][2], J [N][2][6])"""
    box = ac.CSTR_BOX
    lb, ub = np.concatenate((box["lbx"], box["lbu"])), np.concatenate((box["ubx"], box["ubu"]))
    lbu, ubu = np.asarray(box["lbu"]), np.asarray(box["ubu"])
    t = np.tanh(2.0 * ((Z - lb) / (ub - lb) - 0.5) @ K_LAW.T)
    u = lbu + (ubu - lbu) * (0.5 + 0.5 * t)
    J = ((ubu - lbu) * (1.0 - t * t))[:, :, None] * K_LAW[None] / (ub - lb)[None, None, :]
    return u, J


def _points(n, seed):
    box = ac.CSTR_BOX
    lb, ub = np.concatenate((box["lbx"], box["lbu"])), np.concatenate((box["ubx"], box["ubu"]))
    return np.random.default_rng(seed).uniform(lb, ub, (n, 6))


def _dataset(tmp_path, name, n, sensitivities=True, nan_rows=(), seed=0):
    """data_<name>_opt.pkl the way AMPCSampler writes it: columns x0, u_prev, u0 (column vectors), status and, with
    store_sensitivities, du0dx0 [n_u][n_x] and du0du_prev [n_u][n_u] (NaN where the differentiation failed)"""
    import pandas as pd
    Z = _points(n, seed)
    U, J = _law(Z)
    rows = []
    for i in range(n):
        row = {"x0": Z[i, :4].reshape(-1, 1), "u_prev": Z[i, 4:].reshape(-1, 1), "u0": U[i].reshape(-1, 1), "status": True}
        if sensitivities:
            row["du0dx0"], row["du0du_prev"] = J[i, :, :4].copy(), J[i, :, 4:].copy()
            if i in nan_rows:
                row["du0dx0"][:] = np.nan
                row["du0du_prev"][:] = np.nan
        rows.append(row)
    d = tmp_path / "sampling" / name
    d.mkdir(parents=True)
    pd.DataFrame(rows).to_pickle(d / f"data_{name}_opt.pkl")
    return name


def _ampc(seed, n_neurons=20):
    torch.manual_seed(seed)
    ampc = ApproxMPC(ac.stub_mpc(4, 2, True, **ac.CSTR_BOX))
    ampc.settings.n_hidden_layers, ampc.settings.n_neurons = 1, n_neurons
    return ac.setup_ampc(ampc, hostemu=True)


def _trainer(tmp_path, ampc, name, n_epochs, weight, **settings):
    tr = Trainer(ampc)
    st = tr.settings
    st.dataset_name, st.n_epochs, st.batch_size, st.sobolev_weight = name, n_epochs, 128, weight
    st.data_dir, st.results_dir = str(tmp_path / "sampling"), str(tmp_path / "training")
    for k, v in settings.items():
        setattr(st, k, v)
    tr.setup()
    tr.generator.manual_seed(7)
    return tr


def _scaled(ampc, Z):
    """(xs, us, Js) of points of the law in the network's coordinates, float64"""
    U, J = _law(Z)
    xr, yr = ampc.x_range.numpy().ravel(), ampc.y_range.numpy().ravel()
    return (Z - ampc.x_shift.numpy().ravel()) / xr, (U - ampc.y_shift.numpy().ravel()) / yr, J * xr[None, None, :] / yr[None, :, None]


@pytest.mark.parametrize("act, out_act", [("tanh", "linear"), ("sigmoid", "tanh"), ("relu", "sigmoid"), ("leaky_relu", "linear")])
def test_the_torch_recursion_is_autograds_jacobian(act, out_act):
    ampc = ac.network(4, 2, True, hostemu=True, seed=2, n_hidden_layers=2, n_neurons=9, act_fn=act, output_act_fn=out_act)
    xs = torch.rand(5, 6, generator=torch.Generator().manual_seed(1))
    y, J = network_jacobian(ampc.net, xs)
    assert torch.equal(y, ampc.net(xs))
    ref = torch.stack([torch.autograd.functional.jacobian(ampc.net, x) for x in xs])
    assert J.shape == (5, 2, 6) and torch.allclose(J, ref, rtol=1e-5, atol=1e-7)


@pytest.mark.filterwarnings("ignore:Length of split at index 1 is 0")
def test_loss_is_mse_u_plus_weight_times_mse_j_over_the_labelled_rows(tmp_path):
    lam = 0.37
    name = _dataset(tmp_path, "loss", 64, nan_rows=(3, 17, 40))
    ampc = _ampc(1)
    tr = _trainer(tmp_path, ampc, name, 1, lam, val=0.0, batch_size=64, shuffle=False)
    train_loader, _, _ = tr.load_data()
    (xs, us, js), = list(train_loader)
    assert xs.shape == (64, 6) and js.shape == (64, 2, 6) and js.dtype == torch.float32
    labelled = torch.isfinite(js).all(dim=2).all(dim=1)
    assert int(labelled.sum()) == 61
    # the labels are the law's Jacobian in the network's coordinates (same row set: the split may permute the rows)
    xs64, _, Js64 = _scaled(ampc, _points(64, 0))
    order = [int(np.argmin(np.abs(xs64 - x.numpy()).sum(axis=1))) for x in xs]
    assert sorted(order) == list(range(64))
    assert np.allclose(js[labelled].numpy(), Js64[order][labelled.numpy()], rtol=1e-5, atol=1e-6)

    def expected(rows_j):
        J = torch.stack([torch.autograd.functional.jacobian(ampc.net, x) for x in xs])
        mse_u = torch.nn.functional.mse_loss(ampc.net(xs), us)
        return mse_u.item(), torch.nn.functional.mse_loss(J[rows_j], js[rows_j]).item()
    mse_u, mse_j = expected(labelled)
    loss = tr._loss(xs, us, js).item()
    print(f"loss {loss:.6e}, mse_u {mse_u:.6e}, mse_j {mse_j:.6e}")
    assert mse_j > 0 and loss == pytest.approx(mse_u + lam * mse_j, rel=1e-5)
    # rows with a NaN label count in the first term only: other u labels there move the loss by the first term's change alone
    us2 = us.clone()
    us2[~labelled] += 0.5
    mse_u2 = torch.nn.functional.mse_loss(ampc.net(xs), us2).item()
    assert mse_u2 != mse_u and tr._loss(xs, us2, js).item() == pytest.approx(mse_u2 + lam * mse_j, rel=1e-5)
    # a mini-batch without any labelled row has a zero second term
    none = ~labelled
    assert tr._loss(xs[none], us[none], js[none]).item() == pytest.approx(torch.nn.functional.mse_loss(ampc.net(xs[none]), us[none]).item(), rel=1e-6)
    # autograd reaches the weights through the second term
    ampc.net.zero_grad()
    (tr._loss(xs, us, js) - torch.nn.functional.mse_loss(ampc.net(xs), us)).backward()
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for n, p in ampc.net.named_parameters() if n != "layers.2.bias")


def test_weight_zero_is_todays_training_with_or_without_the_columns(tmp_path):
    runs = []
    for name, sens in (("with", True), ("without", False)):
        _dataset(tmp_path, name, 300, sensitivities=sens, nan_rows=(5,))
        ampc = _ampc(3)
        tr = _trainer(tmp_path, ampc, name, 3, 0.0)
        assert tr.settings.sobolev_weight == 0.0
        loaders = tr.load_data()
        assert all(len(batch) == 2 for batch in loaders[0])            # (x, u) only: nothing of the columns is read
        ampc = _ampc(3)
        tr = _trainer(tmp_path, ampc, name, 3, 0.0)
        tr.default_training()
        runs.append((ampc.net.state_dict(), tr.history))
    (sd_a, h_a), (sd_b, h_b) = runs
    assert set(h_a) == {"epoch", "train_loss", "lr", "val_loss"} and len(h_a["epoch"]) == 3
    assert h_a == h_b
    assert list(sd_a) == list(sd_b) and all(torch.equal(sd_a[k], sd_b[k]) for k in sd_a)
    # ... and it is what the plain loop computes: the same split, the same shuffling, mse_loss, Adam
    ampc = _ampc(3)
    tr = _trainer(tmp_path, ampc, "without", 3, 0.0)
    train_loader, val_loader, optimizer = tr.load_data()
    for _ in range(3):
        for x, y in train_loader:
            loss = torch.nn.functional.mse_loss(ampc.net(x), y)
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
        with torch.no_grad():
            for x, y in val_loader:
                pass
    assert all(torch.equal(sd_a[k], v) for k, v in ampc.net.state_dict().items())


def test_positive_weight_without_the_columns_raises_by_name(tmp_path):
    name = _dataset(tmp_path, "plain", 32, sensitivities=False)
    tr = _trainer(tmp_path, _ampc(0), name, 1, 1.0)
    with pytest.raises(ValueError, match="store_sensitivities"):
        tr.default_training()
    with pytest.raises(ValueError, match="store_sensitivities"):
        tr.sensitivity_error()


def test_sobolev_history_carries_both_terms_and_sensitivity_error_is_the_jacobian_error(tmp_path):
    name = _dataset(tmp_path, "terms", 96, nan_rows=(0, 1))
    ampc = _ampc(5)
    tr = _trainer(tmp_path, ampc, name, 4, 0.5, batch_size=32)
    tr.default_training()
    h = tr.history
    assert set(h) == {"epoch", "train_loss", "lr", "val_loss", "train_loss_u", "train_loss_j", "val_loss_u", "val_loss_j"}
    for split in ("train_loss", "val_loss"):
        assert len(h[split]) == 4
        assert h[split] == pytest.approx([u + 0.5 * j for u, j in zip(h[split + "_u"], h[split + "_j"])], rel=1e-5)
    e = tr.sensitivity_error()
    xs, _, Js = _scaled(ampc, _points(96, 0)[2:])
    J = torch.stack([torch.autograd.functional.jacobian(ampc.net, x) for x in torch.tensor(xs, dtype=torch.float32)]).double().numpy()
    assert e["n_rows"] == 96 and e["n_labelled"] == 94
    assert e["mse"] == pytest.approx(float(np.mean((J - Js) ** 2)), rel=1e-4) and e["max_abs"] == pytest.approx(float(np.max(np.abs(J - Js))), rel=1e-4)


def test_sobolev_training_on_few_points_beats_plain_training(tmp_path):
    """16 training rows, 1 x 20 tanh, Adam 1e-2, full batch, 400 epochs: on 512 held-out points the Sobolev run's Jacobian mse and
    value mse are both lower than the plain run's (a comparison of two measured numbers)"""
    name = _dataset(tmp_path, "few", 20, seed=3)                   # val = 0.2 of 20 rows: 16 train
    Zh = _points(512, 99)
    result = {}
    for weight in (0.0, 1.0):
        ampc = _ampc(11)
        tr = _trainer(tmp_path, ampc, name, 400, weight, batch_size=16, learning_rate=1e-2, print_frequency=1000)
        train_loader, _, _ = tr.load_data()
        assert [len(batch[0]) for batch in train_loader] == [16]
        tr.generator.manual_seed(7)
        tr.default_training()
        xs, us, Js = _scaled(ampc, Zh)
        with torch.no_grad():
            y, J = network_jacobian(ampc.net, torch.tensor(xs, dtype=torch.float32))
        result[weight] = (float(np.mean((y.double().numpy() - us) ** 2)), float(np.mean((J.double().numpy() - Js) ** 2)))
    (v0, j0), (v1, j1) = result[0.0], result[1.0]
    print(f"held-out value mse: plain {v0:.3e}, Sobolev {v1:.3e}, ratio {v0 / v1:.1f}; "
          f"held-out Jacobian mse: plain {j0:.3e}, Sobolev {j1:.3e}, ratio {j0 / j1:.1f}")
    assert j1 < j0 and v1 < v0
