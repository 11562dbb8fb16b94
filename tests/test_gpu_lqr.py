"""LQR design on the MI355X (HIP path through the C ABI dompc_lqr_*): the checks of tests/test_lqr.py on the device with the bounds
established there on the host emulation, the device-pointer entries and the device-resident closed loop.  Reads only tests/golden/
and the prebuilt code objects."""
import json
import os

import numpy as np
import pytest

import lqr_common as lc

pytestmark = pytest.mark.gpu


def test_oscillating_masses_loop_reproduces_the_stored_run_with_the_pinned_code_object():
    ex_, eu_ = lc.replay("oscillating_masses_lqr", hostemu=False)
    assert ex_ < 1e-8 and eu_ < 1e-8
    _, _, lqr = lc.example("oscillating_masses_lqr", hostemu=False)
    d = next(iter(lqr._designs.values()))
    assert d.hash == json.load(open(os.path.join(lc.GOLDEN, "lqr_template_hashes.json")))["oscillating_masses_lqr"]


def test_cstr_loop_reproduces_the_stored_run():
    """bounds and their reasons: tests/test_lqr.py::test_cstr_loop_reproduces_the_stored_run"""
    ex_, eu_ = lc.replay("cstr_lqr", hostemu=False, abstol=1e-12)
    assert ex_ < 1e-8 and eu_ < 1.2e-7


@pytest.mark.parametrize("n_horizon", [None, 1, 10, 50])
@pytest.mark.parametrize("rate", [False, True], ids=["standard", "rate"])
@pytest.mark.parametrize("name", ["oscillating_masses_lqr", "cstr_lqr"])
def test_example_gains_against_the_twin(name, rate, n_horizon):
    lc.check_example_gains(name, rate, n_horizon, hostemu=False)


def test_family_a_random_systems_in_one_launch():
    lc.check_family_a(hostemu=False)


@pytest.mark.parametrize("rate", [False, True], ids=["standard", "rate"])
def test_the_largest_design_size(rate):
    lc.check_size_16(rate, hostemu=False)


def test_family_b_operating_points_of_the_cstr():
    lc.check_family_b(hostemu=False)


def test_status_bits_and_neighbours():
    lc.check_status(hostemu=False)


def test_device_pointer_entries_equal_the_host_entries():
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a, dt=torch.float64: torch.tensor(np.asarray(a), dtype=dt, device=dev)      # noqa: E731
    # gains_batch_device: 4 003 designs of family (a) (not a multiple of 4), per-member weights
    A, Bm, Q, R = (a[:4003] for a in lc.embed(lc.family_a()))
    Bn = A.shape[0]
    lqr = lc.model_free_lqr(12, 4, hostemu=False)
    ref = lqr.gains_batch(A, Bm, Q, R)
    K = torch.full((Bn + 1, 4, 12), float("nan"), dtype=torch.float64, device=dev)
    P = torch.full((Bn + 1, 12, 12), float("nan"), dtype=torch.float64, device=dev)
    st = torch.full((Bn + 1,), -7, dtype=torch.int32, device=dev)
    dA, dB, dQ, dR = t(A), t(Bm), t(Q), t(R)
    lqr.gains_batch_device(Bn, dA.data_ptr(), dB.data_ptr(), dQ.data_ptr(), dR.data_ptr(), K.data_ptr(), P.data_ptr(), status=st.data_ptr(),
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(K[:Bn].cpu().numpy(), ref["K"]) and np.array_equal(P[:Bn].cpu().numpy(), ref["P"])
    assert np.array_equal(st[:Bn].cpu().numpy() & 0xFF, ref["status"]) and int(st[Bn]) == -7
    assert bool(torch.isnan(K[Bn]).all()) and bool(torch.isnan(P[Bn]).all())          # nothing behind row Bn is written
    # gains_at_device: shared design-size weights
    ex, plant, lq = lc.example("cstr_lqr", hostemu=False)
    X, U = lc.family_b_points(ex, 257)
    ref = lq.gains_at(plant, X, U)
    Qd = np.block([[ex.Q, np.zeros((4, 2))], [np.zeros((2, 4)), ex.R]])
    K, P = torch.empty((257, 2, 6), dtype=torch.float64, device=dev), torch.empty((257, 6, 6), dtype=torch.float64, device=dev)
    Ad, Bd = torch.empty((257, 4, 4), dtype=torch.float64, device=dev), torch.empty((257, 4, 2), dtype=torch.float64, device=dev)
    dX, dU, dQ, dR = t(X), t(U), t(Qd), t(ex.R_DELTA)
    lq.gains_at_device(plant, 257, dX.data_ptr(), dU.data_ptr(), dQ.data_ptr(), dR.data_ptr(), K.data_ptr(), P.data_ptr(), P_term=dQ.data_ptr(),
                       A=Ad.data_ptr(), B=Bd.data_ptr(), shared_mask=1 | 2 | 4, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for have, want in ((K, ref["K"]), (P, ref["P"]), (Ad, ref["A"]), (Bd, ref["B"])):
        assert np.array_equal(have.cpu().numpy(), want)


@pytest.mark.parametrize("name", ["oscillating_masses_lqr", "cstr_lqr"])
def test_batch_closed_loop_of_copies_is_the_single_loop(name):
    lc.check_closed_loop_copies(name, hostemu=False)


def test_batch_closed_loop_with_a_gain_schedule():
    lc.check_closed_loop_schedule(hostemu=False)


@pytest.mark.parametrize("members", [None, [4, 5, 6, 7, 8, 9, 15]], ids=["B16", "B7-slowest-last"])
def test_zero_order_hold_with_mixed_squarings_in_a_wavefront(members):
    """the squaring loop of expm runs to the largest s of the wavefront: every member bit for bit against its single-member call"""
    lc.check_mixed_squarings(hostemu=False, members=members)


def test_failed_exponentials_beside_good_designs():
    lc.check_failed_exponential(hostemu=False)
