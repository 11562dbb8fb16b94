"""The batched network Jacobian on the MI355X (dompc_ampc_jac_kernel through the C ABI dompc_ampc_jacobian_batch*): the checks of
tests/test_ampc_jacobian.py on the device with the same bound (8 x torch's own float32 autograd error against the float64 twin, measured
at test time), the device-pointer entry, and the CSTR example end to end with stored sensitivities and Sobolev training.  Reads only
tests/golden/ and the prebuilt code objects."""
import copy

import numpy as np
import pytest
import torch

import ampc_common as ac
import ampc_jac_common as jc

pytestmark = pytest.mark.gpu
PREBUILT = ac.FAMILY[:ac.N_PREBUILT]


def device_buffers(arrays):
    """`buffers` of jc.check_no_rterm on the device"""
    dev = torch.device("cuda", 0)
    tensors = [torch.tensor(np.asarray(a, dtype=np.float64), device=dev) for a in arrays]

    def read():
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in tensors]
    return [t.data_ptr() for t in tensors], read


@pytest.mark.parametrize("case", PREBUILT, ids=[ac.family_id(c) for c in PREBUILT])
def test_shape_family(case):
    jc.check_family(case, hostemu=False)


def test_u_of_the_jacobian_call_is_the_step_and_clipped_rows_are_zero():
    assert jc.check_clipping(hostemu=False) > 0


def test_equal_inputs_give_equal_jacobians_wherever_they_sit():
    jc.check_position_independence(hostemu=False)


def test_the_jacobian_after_a_weight_change_is_that_of_the_new_weights():
    jc.check_weight_refresh(hostemu=False)


def test_without_rterm_du_du_prev_is_none_and_null_pointers_are_accepted():
    jc.check_no_rterm(False, device_buffers)


def test_device_pointer_entry_equals_the_host_entry():
    dev = torch.device("cuda", 0)
    ampc = ac.stored_cstr(hostemu=False)
    B = 4003                                               # not a multiple of the 32 samples of a wavefront
    X, Up = ac.inputs(ampc, B, seed=21, spread=1.2)
    for clip in (False, True):
        ref = ampc.jacobian_batch(X, Up, clip_to_bounds=clip)
        dX, dU = torch.tensor(X, device=dev), torch.tensor(Up, device=dev)
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)      # noqa: E731
        u, jx, ju = nan(B + 1, 2), nan(B + 1, 2, 4), nan(B + 1, 2, 2)                               # one row longer than needed
        ampc.jacobian_batch_device(B, dX.data_ptr(), dU.data_ptr(), u.data_ptr(), jx.data_ptr(), ju.data_ptr(),
                                   stream=torch.cuda.current_stream().cuda_stream, clip_to_bounds=clip)
        torch.cuda.synchronize()
        for out, key in ((u, "u"), (jx, "du_dx"), (ju, "du_du_prev")):
            assert np.array_equal(out[:B].cpu().numpy(), ref[key]), (key, clip)
            assert bool(torch.isnan(out[B]).all()), (key, clip)       # nothing behind row B is written


def test_cstr_example_end_to_end_with_sensitivities_and_sobolev_training(tmp_path):
    import pandas as pd
    from do_mpc_amd.ampc import network_jacobian
    from do_mpc_amd.examples import cstr_ampc as ex
    cstr_mpc = ex.build_mpc(ex.build_model(), max_batch=512)
    n = 256
    np.random.seed(42)
    sampler = ex.build_sampler(cstr_mpc, "e2e_sens", n, str(tmp_path / "sampling"), sensitivities=True)
    sampler.settings.chunk = n
    # the sampling box of the plain end-to-end test (tests/test_gpu_ampc.py): the operating region of the reactor
    sampler.settings.lbx = np.array([[0.5], [0.3], [125.0], [122.0]])
    sampler.settings.ubx = np.array([[1.2], [0.8], [138.0], [136.0]])
    sampler.default_sampling()
    data = pd.read_pickle(tmp_path / "sampling" / "e2e_sens" / "data_e2e_sens_opt.pkl")
    solved = len(data)
    finite = np.array([bool(np.all(np.isfinite(a)) and np.all(np.isfinite(b))) for a, b in zip(data["du0dx0"], data["du0du_prev"])])
    print(f"{solved} of {n} samples solved, {int(finite.sum())} of them with finite sensitivities")
    assert solved >= 0.9 * n and finite.sum() >= 0.8 * solved
    torch.manual_seed(42)
    ampc = ex.build_ampc(cstr_mpc)
    trainer = ex.build_trainer(ampc, "e2e_sens", 40, str(tmp_path / "sampling"), str(tmp_path / "training"), sobolev_weight=1.0)
    trainer.settings.batch_size = 128
    trainer.default_training()
    h = trainer.history
    print(f"validation loss {h['val_loss'][0]:.3e} -> {h['val_loss'][-1]:.3e} (u {h['val_loss_u'][-1]:.3e}, J {h['val_loss_j'][-1]:.3e})")
    assert h["val_loss"][-1] < h["val_loss"][0]
    e = trainer.sensitivity_error()
    print(f"sensitivity_error: {e}")
    assert e["n_labelled"] == int(finite.sum()) and np.isfinite(e["mse"]) and np.isfinite(e["max_abs"])
    # on the labelled rows: the device against the torch recursion of the trained network, within the bound of the shape family
    stack = lambda key: np.stack([np.asarray(v, float).reshape(-1) for v in data[key]])[finite]      # noqa: E731
    X, Up = stack("x0"), stack("u_prev")
    err, E, bound, r = jc.check_jacobian(ampc, X, Up, "trained CSTR network")
    cfg = ac.cfg_of(ampc)
    with torch.no_grad():
        J32 = network_jacobian(copy.deepcopy(ampc.net).cpu(), torch.from_numpy(ac.scaled_input(cfg, X, Up)))[1].double().numpy()
    diff = float(np.max(np.abs(jc.to_network_coordinates(cfg, jc.full(ampc, r)) - J32)))
    print(f"|device - torch recursion| = {diff:.3e}, bound = {bound:.3e}")
    assert diff <= bound
