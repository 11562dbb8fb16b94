"""Extended Kalman filter for models with algebraic states on the MI355X (HIP path through the C ABI dompc_ekf_step_dae_*): the checks
of tests/test_ekf_dae.py on the device with the same bounds (equivalence with the ODE filter of a hand-eliminated model, or the twin
tests/ekf_dae_common.py:TwinDAE as oracle - no reference fixture can exist, the reference's EKF asserts n_alg == 0), the device-pointer
entry, the code objects' resources and the device-resident closed loop.  Reads only tests/golden/ and the prebuilt code objects."""
import numpy as np
import pytest

import ekf_common as ec
import ekf_dae_common as dc
import lqr_common as lc

pytestmark = pytest.mark.gpu


def test_discrete_filter_equals_the_filter_of_the_hand_eliminated_model():
    dc.check_masses_equivalence(hostemu=False)


def test_jacobians_are_evaluated_at_the_prior_estimate_of_the_reduced_system():
    dc.check_evaluation_points(hostemu=False)


@pytest.mark.parametrize("name", ["continuous", "dip"])
def test_continuous_models_against_the_twin(name):
    """the bound established on the CPU (tests/test_ekf_dae.py::test_continuous_models_against_the_twin)"""
    dc.check_continuous(name, hostemu=False)


def test_batch_reactor_equals_the_filter_of_the_hand_eliminated_model():
    dc.check_batch_reactor_equivalence(hostemu=False)


@pytest.fixture(scope="module")
def continuous_filter():
    return dc.make_filter("continuous", hostemu=False)


@pytest.mark.parametrize("B", [1, 3, 4, 5, 7, 9])
def test_a_filter_does_not_depend_on_its_neighbours_in_the_wavefront(continuous_filter, B):
    dc.check_one_wavefront_unequal_work(continuous_filter, B)


def test_status_bit_2_keeps_the_prior_and_leaves_the_neighbours_alone():
    dc.check_status_bit_2(hostemu=False)


def test_the_largest_filter_against_the_twin():
    dc.check_limit_sizes(hostemu=False)


def test_make_step_carries_z0_and_records_z():
    dc.check_make_step(hostemu=False)


def test_device_pointer_entry_equals_the_host_entry(continuous_filter):
    """x, P and z are updated in place; row b equals the host entry bit for bit; nothing behind row B is written"""
    import torch
    ekf = continuous_filter
    B, tail = 7, 2
    m, X, Pc, Y, U, Z0, _ = dc.unequal_filters(B)
    Q, R = 1e-3 * np.eye(2), 1e-2 * np.eye(2)
    host = ekf.step_batch(X, Pc, Y, U, Q, R, Z0=Z0)
    dev = torch.device("cuda", 0)
    pad = lambda a: np.concatenate([a, np.full((tail,) + a.shape[1:], ec.NAN_PATTERN)])      # noqa: E731
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)         # noqa: E731
    xd, Pd, zd, yd, ud, Qd, Rd, none = t(pad(X)), t(pad(Pc)), t(pad(Z0)), t(Y), t(U), t(Q), t(R), t(np.zeros(1))
    st = torch.full((B + tail,), -7, dtype=torch.int32, device=dev)
    nw = torch.full((B + tail,), -7, dtype=torch.int32, device=dev)
    ekf.step_batch_device(B, xd.data_ptr(), Pd.data_ptr(), yd.data_ptr(), ud.data_ptr(), none.data_ptr(), none.data_ptr(), Qd.data_ptr(),
                          Rd.data_ptr(), status=st.data_ptr(), shared_mask=2 | 4 | 8 | 16, stream=torch.cuda.current_stream().cuda_stream,
                          z=zd.data_ptr(), newton=nw.data_ptr())
    torch.cuda.synchronize()
    xo, Po, zo, so, no = xd.cpu().numpy(), Pd.cpu().numpy(), zd.cpu().numpy(), st.cpu().numpy(), nw.cpu().numpy()
    assert np.array_equal(xo[:B], host["x"]) and np.array_equal(Po[:B], host["P"]) and np.array_equal(zo[:B], host["Z"])
    assert np.array_equal(so[:B] & 0xFF, host["status"]) and np.array_equal(so[:B] >> 8, host["n_steps"]) and np.array_equal(no[:B], host["newton"])
    bits = lambda a: np.ascontiguousarray(a[B:]).view(np.uint64)      # noqa: E731
    assert np.all(bits(xo) == dc.NAN_BITS) and np.all(bits(Po) == dc.NAN_BITS) and np.all(bits(zo) == dc.NAN_BITS)
    assert np.all(so[B:] == -7) and np.all(no[B:] == -7)


@pytest.mark.parametrize("name", ["masses", "oscillating_masses_dae"])
def test_discrete_filters_use_no_scratch(name, tmp_path):
    """the code objects of the shipped discrete filters: no scratch memory, no spilled VGPR (amdhsa metadata, as tests/test_ekf.py; None
    without llvm-readelf).  The continuous filters and the n_x = n_z = n_y = 16 one are recorded in profiles/ekf_dae_resource_usage.txt."""
    import __graft_entry__ as ge
    from do_mpc_amd import build
    (_, hdr, h), = ge.lowered_ekf_dae([name])
    meta = lc.kernel_metadata(build.ekf_code_object(hdr, h), tmp_path, kernel="dompc_ekf_kernel")
    assert meta in (None, (0, 0)), (name, meta)


def test_device_resident_closed_loop_on_the_dae_model_equals_the_per_sample_loops():
    """BatchClosedLoopEKF on oscillating_masses_dae - the shipped controller, the plant and the filter of the model with its algebraic
    states, full-state measurement - against the per-sample loops mpc.make_step / simulator.make_step / ekf.make_step: 1e-9 for u0, y and
    the estimate, the bounds of tests/test_gpu_ekf.py::test_device_resident_closed_loop_with_the_filter_equals_the_per_sample_loops"""
    from do_mpc_amd.closed_loop import BatchClosedLoopEKF
    from do_mpc_amd.simulator import Simulator
    ex = dc.OM
    model = ex.build_model()
    B, steps = 5, 3
    rng = np.random.RandomState(77)
    X0 = np.array([ex.X0 * (0.5 + rng.rand()) for _ in range(B)])
    x_est0 = X0 + 0.05 * (rng.rand(B, 4) - 0.5)
    P0, Q, R = 0.1 * np.eye(4), 1e-3 * np.eye(4), 1e-2 * np.eye(4)

    def make_sim():
        sim = Simulator(model)
        sim.set_param(t_step=0.5)
        sim.setup()
        return sim

    def make_ekf():
        ekf = dc.make_filter("oscillating_masses_dae", hostemu=False)
        assert ekf.model.n_z == 4 and ekf.model.n_y == 4
        return ekf

    loop = BatchClosedLoopEKF(ex.build_mpc(model, max_batch=B), make_sim(), make_ekf(), X0, x_est0, P0, Q, R)
    out = [loop.step() for _ in range(steps)]
    assert all(o["mpc_stats"]["success"].all() and not o["plant_status"].any() and not o["ekf_status"].any() for o in out)
    assert out[-1]["z_est"].shape == (B, 4)
    for b in range(B):
        mpc, sim, ekf = ex.build_mpc(model), make_sim(), make_ekf()
        x_est = x_est0[b].copy()
        mpc.x0 = x_est
        ekf.x0 = x_est
        ekf.P0 = P0.copy()
        sim.x0 = X0[b]
        mpc.set_initial_guess()
        for k in range(steps):
            u0 = mpc.make_step(x_est)
            y = sim.make_step(u0)
            x_est = ekf.make_step(y, u0, Q, R).ravel()
            assert ec.relerr(out[k]["u0"][b], u0.ravel()) < 1e-9 and ec.relerr(out[k]["y"][b], y.ravel()) < 1e-9
            assert ec.relerr(out[k]["x_est"][b], x_est) < 1e-9 and ec.relerr(out[k]["z_est"][b], ekf.z0.master) < 1e-9
