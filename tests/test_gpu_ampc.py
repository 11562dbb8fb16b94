"""Approximate MPC on the MI355X (HIP path through the C ABI dompc_ampc_*): the checks of tests/test_ampc.py on the device with the same
bound (8 x the reference's own float32 error against the float64 twin, measured at test time), the device-pointer entry, the
device-resident closed loop and the example end to end: sample, train, run.  Reads only tests/golden/ and the prebuilt code objects."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import ampc_common as ac

pytestmark = pytest.mark.gpu
PREBUILT = ac.FAMILY[:ac.N_PREBUILT]


@pytest.fixture(scope="module")
def cstr_mpc():
    from do_mpc_amd.examples import cstr_ampc as ex
    return ex.build_mpc(ex.build_model(), max_batch=512)


def test_family_is_the_prebuilt_list():
    sys.path.insert(0, os.path.dirname(os.path.dirname(ac.GOLDEN)))
    import __graft_entry__ as g
    assert [ac.family_shape(c) for c in PREBUILT] == g.PREBUILT_AMPC and len(g.PREBUILT_AMPC) <= 16
    # the pinned hashes are those of the generated SHAPE headers (not of the kernel text) of the first two entries
    pinned = json.load(open(os.path.join(ac.GOLDEN, "ampc_template_hashes.json")))
    lowered = g.lowered_ampc(g.PREBUILT_AMPC[:2])
    assert [h for _, _, h in lowered] == [pinned["stored_cstr_network"], pinned["default_network"]]


def test_stored_network_on_the_cstr_controller_with_the_pinned_code_object(cstr_mpc):
    ampc, err, E = ac.check_stored(hostemu=False, mpc=cstr_mpc)
    assert ampc.model_hash == json.load(open(os.path.join(ac.GOLDEN, "ampc_template_hashes.json")))["stored_cstr_network"]


@pytest.mark.parametrize("case", PREBUILT, ids=[ac.family_id(c) for c in PREBUILT])
def test_shape_family(case):
    ac.check_family(case, hostemu=False)


def test_make_step_is_the_batch_of_one_and_iterates_u0():
    ac.check_make_step(hostemu=False)


def test_a_step_after_a_weight_change_uses_the_new_weights():
    ac.check_weight_refresh(hostemu=False)


def test_device_pointer_entry_equals_the_host_entry():
    dev = torch.device("cuda", 0)
    ampc = ac.stored_cstr(hostemu=False)
    B = 4003                                               # not a multiple of the 32 samples of a wavefront
    X, Up = ac.inputs(ampc, B, seed=21, spread=1.2)
    ref = ampc.make_step_batch(X, Up)
    dX, dU = torch.tensor(X, device=dev), torch.tensor(Up, device=dev)
    out = torch.full((B + 1, 2), float("nan"), dtype=torch.float64, device=dev)
    ampc.make_step_batch_device(B, dX.data_ptr(), dU.data_ptr(), out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(out[:B].cpu().numpy(), ref)
    assert bool(torch.isnan(out[B]).all())                 # nothing behind row B is written


def test_equal_inputs_give_equal_outputs_wherever_they_sit():
    ampc = ac.network(4, 2, True, hostemu=False, seed=3, n_hidden_layers=1, n_neurons=32, act_fn="relu", output_act_fn="linear")
    X, Up = ac.inputs(ampc, 97, seed=8)
    rows = [0, 31, 32, 63, 64, 96]
    X[rows], Up[rows] = X[5], Up[5]
    U = ampc.make_step_batch(X, Up, clip_to_bounds=False)
    for r in rows:
        assert np.array_equal(U[r], U[5])
    assert len({U[r].tobytes() for r in range(97)}) > 80   # (the other rows differ)


def test_batch_closed_loop_of_copies_is_the_single_loop():
    ac.check_closed_loop(hostemu=False)


def test_cstr_example_end_to_end_sample_train_run(cstr_mpc, tmp_path):
    from do_mpc_amd.closed_loop import BatchClosedLoopAMPC
    from do_mpc_amd.examples import cstr_ampc as ex
    n = 512
    np.random.seed(42)
    sampler = ex.build_sampler(cstr_mpc, "e2e", n, str(tmp_path / "sampling"))
    sampler.settings.chunk = n
    # the sampling box: the operating region of the reactor.  On the whole bounds box (T_R, T_K from 50 to 140) 358 of 512 cold solves
    # converge within the iteration limit; the condition below is one on the inputs, so the box is shrunk, not the threshold
    sampler.settings.lbx = np.array([[0.5], [0.3], [125.0], [122.0]])
    sampler.settings.ubx = np.array([[1.2], [0.8], [138.0], [136.0]])
    sampler.default_sampling()
    import pandas as pd
    solved = len(pd.read_pickle(tmp_path / "sampling" / "e2e" / "data_e2e_opt.pkl"))
    print(f"{solved} of {n} samples solved")
    assert solved >= 0.9 * n
    torch.manual_seed(42)
    ampc = ex.build_ampc(cstr_mpc)
    trainer = ex.build_trainer(ampc, "e2e", 40, str(tmp_path / "sampling"), str(tmp_path / "training"))
    trainer.settings.batch_size = 128
    trainer.default_training()
    val = trainer.history["val_loss"]
    print(f"validation loss {val[0]:.3e} -> {val[-1]:.3e}")
    assert val[-1] < val[0]
    sim = ex.build_simulator(ex.build_model())
    lb, ub, lbu, ubu = ampc._box()
    rng = np.random.default_rng(0)
    X0 = ex.X0 * rng.uniform(0.95, 1.05, (64, 4))
    rec = BatchClosedLoopAMPC(ampc, sim, X0, U_prev0=np.tile(ex.U0, (64, 1))).run(20)
    assert np.all(rec["u"] >= lbu) and np.all(rec["u"] <= ubu) and np.all(np.isfinite(rec["x"]))
    assert not rec["plant_status"].any()
