"""Extended Kalman filter on the MI355X (HIP path through the C ABI dompc_ekf_*): the checks of tests/test_ekf.py on the device, large
batches, the in-place device entry and the device-resident closed loop controller -> plant -> filter."""
import json
import os

import numpy as np
import pytest

import ekf_common as ec
from do_mpc_amd.examples import CASES, triple_tank

pytestmark = pytest.mark.gpu


def test_triple_tank_example_reproduces_the_golden_estimator_records_with_the_pinned_code_object():
    ekf = triple_tank.build_ekf(triple_tank.build_model())
    ec.check_golden_triple_tank(ekf)
    # the code object that ran is the one the un-edited reference templates lower to (tests/test_ekf_reference_templates.py pins the
    # hash where the reference tree exists; the runtime compared it with the hash embedded in the code object at create)
    pinned = json.load(open(os.path.join(ec.GOLDEN, "ekf_template_hashes.json")))["triple_tank"]
    assert ekf.model_hash == pinned
    assert os.path.basename(os.path.dirname(ekf.code_object)) == "ekf_" + pinned and os.path.isfile(ekf.code_object)


def test_measurement_jacobian_is_evaluated_at_the_prior_estimate():
    ec.check_evaluation_point(hostemu=False)


@pytest.mark.parametrize("name", ["rotating_masses", "CSTR"])
def test_continuous_models_against_the_twin(name):
    """the bound established on the CPU (tests/test_ekf.py::test_continuous_models_against_the_twin)"""
    ec.check_continuous(name, hostemu=False)


@pytest.mark.parametrize("shared_qr", [True, False])
@pytest.mark.parametrize("B", [1, 3, 4, 9])
def test_a_filter_does_not_depend_on_its_slot_in_the_batch(B, shared_qr):
    ec.check_batch_semantics(ec.make_ekf("rotating_masses", hostemu=False), B, shared_qr)


@pytest.mark.parametrize("name", ["oscillating_masses", "rotating_masses"])
def test_large_batch_not_a_multiple_of_the_wavefront(name):
    """B = 16 387 random filters (not a multiple of 4 or 64): 64 members drawn at random against the twin, rows 0, B-2 and B-1 against
    single calls bit for bit.  Bounds: the discrete filter is a few hundred operations on numbers of size 1 with cond(S) < 100
    (P ~ 0.1, R >= 1e-2): 1e-10 leaves three digits over round-off; the continuous one the 1e-9 of the integration tests."""
    B = 16387
    ekf = ec.make_ekf(name, hostemu=False)
    m = ekf.model
    X, Pc, Y, U, Q, R = ec.random_filters(m, B, seed=5)
    r = ekf.step_batch(X, Pc, Y, U, Q, R)
    assert np.all(r["status"] == 0) and np.all(np.isfinite(r["x"])) and np.all(np.isfinite(r["P"]))
    p, tvp = ec.p_tvp(ekf)
    tw = ec.Twin(m, t_step=ekf.settings.t_step)
    bound = 1e-10 if m.model_type == "discrete" else 1e-9
    worst = 0.0
    for b in np.random.default_rng(17).choice(B, 64, replace=False):
        xt, Pt = tw.step(X[b], Pc[b], Y[b], U[b], Q[b], R[b], p=p, tvp=tvp)
        worst = max(worst, ec.relerr(r["x"][b], xt), ec.relerr(r["P"][b], Pt))
    print(f"{name}: 64 of {B} members, kernel - twin = {worst:.3e} (bound {bound:.0e})")
    assert worst < bound
    for b in (0, B - 2, B - 1):
        one = ekf.step_batch(X[b:b + 1], Pc[b:b + 1], Y[b:b + 1], U[b:b + 1], Q[b], R[b])
        assert np.array_equal(one["x"][0], r["x"][b]) and np.array_equal(one["P"][0], r["P"][b]), b


def test_device_entry_updates_in_place_and_equals_the_host_entry():
    import torch
    ekf = ec.make_ekf("rotating_masses", hostemu=False)
    m = ekf.model
    B, tail = 1023, 3
    X, Pc, Y, U, Q, R = ec.random_filters(m, B, seed=9)
    host = ekf.step_batch(X, Pc, Y, U, Q[0], R)
    dev = torch.device("cuda", 0)
    pad = lambda a: np.concatenate([a, np.full((tail,) + a.shape[1:], ec.NAN_PATTERN)])      # noqa: E731
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)         # noqa: E731
    p, tvp = ec.p_tvp(ekf)
    xd, Pd, yd, ud, Qd, Rd, pd, td = t(pad(X)), t(pad(Pc)), t(Y), t(U), t(Q[0]), t(R), t(p), t(tvp)
    st = torch.full((B + tail,), -7, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream()
    ekf.step_batch_device(B, xd.data_ptr(), Pd.data_ptr(), yd.data_ptr(), ud.data_ptr(), td.data_ptr(), pd.data_ptr(), Qd.data_ptr(),
                          Rd.data_ptr(), status=st.data_ptr(), shared_mask=2 | 4 | 8, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    xo, Po, so = xd.cpu().numpy(), Pd.cpu().numpy(), st.cpu().numpy()
    assert np.array_equal(xo[:B], host["x"]) and np.array_equal(Po[:B], host["P"]) and np.array_equal(so[:B] & 0xFF, host["status"])
    bits = lambda a: np.ascontiguousarray(a[B:]).view(np.uint64)      # noqa: E731
    assert np.all(bits(xo) == 0x7FF8DEADBEEF0123) and np.all(bits(Po) == 0x7FF8DEADBEEF0123) and np.all(so[B:] == -7)


def test_device_resident_closed_loop_with_the_filter_equals_the_per_sample_loops():
    """controller -> plant -> extended Kalman filter -> controller for a batch of loops resident in HBM (BatchClosedLoopEKF: three
    launches per control step) against the per-sample host loops mpc.make_step / simulator.make_step / ekf.make_step: 1e-9 for u0, y
    and the estimate, the bound of test_device_resident_closed_loop_with_the_estimator_equals_the_per_sample_loops"""
    from do_mpc_amd.closed_loop import BatchClosedLoopEKF
    from do_mpc_amd.simulator import Simulator
    ex = CASES["rotating_masses"]
    model = ex.build_model()
    B, steps = 4, 3
    rng = np.random.RandomState(99)
    X0 = np.array([rng.rand(8) - 0.5 for _ in range(B)])
    x_est0 = 0.1 * np.array([rng.rand(8) - 0.5 for _ in range(B)])
    P0, Q, R = 0.1 * np.eye(8), 1e-3 * np.eye(8), 1e-2 * np.eye(5)

    def make_sim():
        sim = Simulator(model)
        sim.set_param(t_step=0.1, abstol=1e-10, reltol=1e-10)
        pt = sim.get_p_template()
        for k in ("Theta_1", "Theta_2", "Theta_3"):
            pt[k] = 2.25e-4
        sim.set_p_fun(lambda t: pt)
        tv = sim.get_tvp_template()
        sim.set_tvp_fun(lambda t: tv)
        sim.setup()
        return sim

    loop = BatchClosedLoopEKF(ex.build_mpc(model, max_batch=B), make_sim(), ec.make_ekf("rotating_masses", hostemu=False, model=model),
                              X0, x_est0, P0, Q, R)
    out = [loop.step() for _ in range(steps)]
    assert all(o["mpc_stats"]["success"].all() and not o["plant_status"].any() and not o["ekf_status"].any() for o in out)
    for b in range(B):
        mpc, sim, ekf = ex.build_mpc(model), make_sim(), ec.make_ekf("rotating_masses", hostemu=False, model=model)
        x_est = x_est0[b].copy()
        mpc.x0 = x_est
        ekf.x0 = x_est
        ekf.P0 = P0.copy()
        sim.x0 = X0[b]
        mpc.set_initial_guess()
        ekf.set_initial_guess()
        for k in range(steps):
            u0 = mpc.make_step(x_est)
            y = sim.make_step(u0)
            x_est = ekf.make_step(y, u0, Q, R).ravel()
            assert ec.relerr(out[k]["u0"][b], u0.ravel()) < 1e-9 and ec.relerr(out[k]["y"][b], y.ravel()) < 1e-9
            assert ec.relerr(out[k]["x_est"][b], x_est) < 1e-9


# ---------------------------------------------------------------------------------------------- unequal problems in one wavefront
# On the device the integration loop runs to the slowest filter of the wavefront and a finished filter keeps its values by select
# (rule 1): rows of a batch with unequal work against their single calls, bit for bit.
@pytest.mark.parametrize("B", [8, 7, 5])
def test_neighbours_with_unequal_step_counts_equal_their_single_calls(B):
    ec.check_unequal_steps(ec.make_ekf("CSTR", hostemu=False), B)


@pytest.mark.parametrize("last", [None, 1, 2, 3], ids=lambda v: "B8" if v is None else f"B7-member{v}-last")
def test_failing_filters_leave_their_neighbours_alone(last):
    ec.check_failures_beside_neighbours(ec.make_ekf("CSTR", hostemu=False), last)


def test_step_limit_inside_a_wavefront():
    ec.check_step_limit_inside_a_wavefront(hostemu=False)


@pytest.mark.parametrize("slot", [2, 4])
def test_singular_s_beside_neighbours(slot):
    """twin of tests/test_ekf.py::test_singular_s_returns_the_a_priori_estimate_with_status_bit_1 with good filters around the bad one"""
    ec.check_status_bit_1_beside_neighbours(hostemu=False, slot=slot)


def test_step_limit_of_a_batch():
    """twin of tests/test_ekf.py::test_step_limit_sets_status_bit_0"""
    ec.check_step_limit(hostemu=False)


@pytest.mark.parametrize("name", ["rotating_masses", "CSTR", "oscillating_masses"])
def test_elimination_of_s_with_row_swaps(name):
    ec.check_row_swaps(name, hostemu=False)
