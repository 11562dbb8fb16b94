"""LQR for models with algebraic states on the MI355X (HIP path through the C ABI dompc_lqr_*): the checks of tests/test_lqr_dae.py on
the device with the same bounds, and the device-pointer entry.  Reads only tests/golden/ and the prebuilt code objects."""
import numpy as np
import pytest

import lqr_common as lc
import lqr_dae_common as dc

pytestmark = pytest.mark.gpu


def test_batch_reactor_dae_loop_reproduces_the_stored_run():
    """bound and its reason: tests/test_lqr_dae.py::test_batch_reactor_dae_loop_reproduces_the_stored_run"""
    (dx, du, dt), z_shape, z_stored = dc.replay(hostemu=False)
    assert dx < 1e-8 and du < 1e-8 and dt < 1e-8
    assert z_shape == z_stored == (50, 0)


def test_batch_reactor_designs_against_the_twin():
    dc.check_batch_reactor(hostemu=False)


def test_elimination_pivots_over_the_lanes():
    dc.check_pivoting(hostemu=False)


def test_newton_converges_member_by_member_inside_one_wavefront():
    dc.check_newton_in_one_wavefront(hostemu=False)


@pytest.mark.parametrize("name", ["nz16", "nx15_rate"])
def test_size_limits(name):
    dc.check_size_limits(False, name)


def test_batch_sizes_with_and_without_z_out():
    dc.check_batch_sizes_and_z_out(hostemu=False)


def test_the_oscillating_masses_dae_model_designs():
    dc.check_oscillating_masses_dae(hostemu=False)


def test_status_bit_2_and_neighbours():
    dc.check_status(hostemu=False)


def test_linearize_dae_is_the_host_statement_of_the_reduction():
    dc.check_linearize_dae(hostemu=False)


def test_batch_closed_loop_on_the_dae_plant():
    dc.check_closed_loop(hostemu=False)


def test_device_pointer_entry_equals_the_host_entry(tmp_path):
    import torch
    from do_mpc_amd import build
    dev = torch.device("cuda", 0)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64, device=dev)      # noqa: E731
    model, lqr = dc.design("newton", hostemu=False)
    X, U = dc.newton_points()
    Z0 = np.zeros((7, 2))
    ref = lqr.gains_at(model, X, U, Z0=Z0)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=dev)      # noqa: E731
    K, P, Ad, Bd, Zo = nan(8, 2, 4), nan(8, 4, 4), nan(8, 4, 4), nan(8, 4, 2), nan(8, 2)
    st = torch.full((8,), -7, dtype=torch.int32, device=dev)
    dX, dU, dZ, dQ, dR = t(X), t(U), t(Z0), t(np.eye(4)), t(np.eye(2))
    lqr.gains_at_device(model, 7, dX.data_ptr(), dU.data_ptr(), dQ.data_ptr(), dR.data_ptr(), K.data_ptr(), P.data_ptr(), A=Ad.data_ptr(),
                        B=Bd.data_ptr(), status=st.data_ptr(), shared_mask=1 | 2, stream=torch.cuda.current_stream().cuda_stream,
                        z=dZ.data_ptr(), z_out=Zo.data_ptr())
    torch.cuda.synchronize()
    for have, want in ((K, ref["K"]), (P, ref["P"]), (Ad, ref["A"]), (Bd, ref["B"]), (Zo, ref["Z"])):
        assert np.array_equal(have[:7].cpu().numpy(), want) and bool(torch.isnan(have[7]).all())      # nothing behind row 7 is written
    s = st.cpu().numpy()
    assert np.array_equal(s[:7] & 0xFF, ref["status"]) and np.array_equal(s[:7] >> 24, ref["newton"]) and s[7] == -7
    assert np.array_equal(dZ.cpu().numpy(), Z0)                                     # the guess is read only
    # the code objects of case (d): no scratch memory, no spilled VGPR
    import __graft_entry__ as ge
    for name, mode in (("nz16", "standard"), ("nx15_rate", "rate")):
        (label, hdr, h), = ge.lowered_lqr([("dae", name, mode)])
        meta = lc.kernel_metadata(build.lqr_code_object(hdr, h), tmp_path)
        assert meta in (None, (0, 0)), (label, meta)
