"""Batched plant integrator (csrc/dompc_plant.hip) on the MI355X with lanes of one wavefront that do unequal work: the checks of
tests/test_plant_family.py on the HIP path, and the device entry `step_batch_device` (masks, optional arguments, a stream of the
caller's, nothing written past row B - 1)."""
import numpy as np
import pytest

import plant_family_common as pf

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B", pf.SIZES)
@pytest.mark.parametrize("kind", ["ode", "dae"])
def test_values_status_and_step_counts(kind, B):
    pf.check_values(kind, hostemu=False, B=B)


def test_explicit_pair_alone_reports_the_step_limit():
    pf.check_explicit_only(hostemu=False)


@pytest.mark.parametrize("kind", ["ode", "dae"])
def test_implicit_method_alone(kind):
    pf.check_implicit_only(kind, hostemu=False)


def test_looser_tolerance_takes_fewer_steps():
    pf.check_looser_tolerance(hostemu=False)


def test_failures_stay_local():
    pf.check_failures_stay_local(hostemu=False)


@pytest.mark.parametrize("kind", ["ode", "dae"])
def test_rows_do_not_depend_on_their_position(kind):
    pf.check_position(kind, hostemu=False)


@pytest.mark.parametrize("kind", ["ode", "dae"])
def test_shared_rows_equal_tiled_rows(kind):
    pf.check_shared_rows(kind, hostemu=False)


def test_discrete_member_equals_numpy():
    pf.check_discrete(hostemu=False)


def test_dip_newton_starts_survive_a_growing_batch():
    pf.check_dip_growing_z_buffer(hostemu=False)


def test_dip_permutation_across_the_wavefront_boundary():
    pf.check_dip_permutation(hostemu=False)


# ---------------------------------------------------------------------------------------------------- the device entry
X_GUARD, ST_GUARD = -12345.678, -1234567                   # what the guard row past B holds before and after a launch


def _device_step(sim, inp, mask, lane, with_w=True, with_v=True, with_y=True, with_status=True):
    """step_batch_device on a stream of its own, outputs with one guard row -> (x_next, y, status) with the guard rows, on the host.
    A group whose mask bit is set passes row `lane` alone."""
    import torch
    B = inp["X"].shape[0]
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")      # noqa: E731
    rows = lambda name, bit: dev(inp[name][lane] if mask & bit else inp[name])                       # noqa: E731
    x, u, tvp, p, w, v = dev(inp["X"]), rows("U", 1), rows("TVP", 2), rows("P", 4), rows("W", 8), rows("V", 16)
    xn = torch.full((B + 1, 3), X_GUARD, dtype=torch.float64, device="cuda")
    y = torch.full((B + 1, 2), X_GUARD, dtype=torch.float64, device="cuda")
    st = torch.full((B + 1,), ST_GUARD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    sim.step_batch_device(B, x.data_ptr(), u.data_ptr(), tvp.data_ptr(), p.data_ptr(), xn.data_ptr(),
                          y=y.data_ptr() if with_y else 0, status=st.data_ptr() if with_status else 0,
                          w=w.data_ptr() if with_w else 0, v=v.data_ptr() if with_v else 0, shared_mask=mask, stream=stream.cuda_stream)
    stream.synchronize()
    return xn.cpu().numpy(), y.cpu().numpy(), st.cpu().numpy()


def _host_step(sim, inp, mask, lane):
    pick = lambda name, bit: inp[name][lane] if mask & bit else inp[name]             # noqa: E731
    r = sim.make_step_batch(inp["X"], pick("U", 1), P=pick("P", 4), TVP=pick("TVP", 2), W=pick("W", 8), V=pick("V", 16))
    return r["x"], r["y"], r["status"] | (r["n_steps"] << 8)


@pytest.mark.parametrize("mask", [0, 31, 2 | 4, 8 | 16])
def test_device_entry_equals_the_host_entry_for_every_mask(mask):
    ref = pf.reference()
    B = 65
    inp = pf.take(ref["inp"], slice(0, B))
    lane = int(np.nonzero(ref["explicit"][:B])[0][1])
    sim = pf.make_simulator("ode", hostemu=False)
    xn, y, st = _device_step(sim, inp, mask, lane)
    hx, hy, hst = _host_step(sim, inp, mask, lane)
    assert np.array_equal(xn[:B], hx) and np.array_equal(y[:B], hy) and np.array_equal(st[:B], hst)
    assert (xn[B] == X_GUARD).all() and (y[B] == X_GUARD).all() and st[B] == ST_GUARD


def test_device_entry_without_noise_measurement_or_status():
    ref = pf.reference()
    B = 65
    inp = pf.take(ref["inp"], slice(0, B))
    sim = pf.make_simulator("ode", hostemu=False)
    zero = dict(inp, W=np.zeros_like(inp["W"]), V=np.zeros_like(inp["V"]))
    hx, hy, hst = _host_step(sim, zero, 0, 0)
    xn, y, st = _device_step(sim, inp, 0, 0, with_w=False, with_v=False)             # w = v = 0: zero noise
    assert np.array_equal(xn[:B], hx) and np.array_equal(y[:B], hy) and np.array_equal(st[:B], hst)
    xn2, y2, st2 = _device_step(sim, inp, 0, 0, with_w=False, with_v=False, with_y=False, with_status=False)
    assert np.array_equal(xn2, xn)                         # y = 0 and status = 0 leave x_next unchanged ...
    assert (y2 == X_GUARD).all() and (st2 == ST_GUARD).all()      # ... and are not written


@pytest.mark.parametrize("B", [63, 64, 65])
def test_nothing_is_written_past_the_last_row(B):
    ref = pf.reference()
    inp = pf.take(ref["inp"], slice(0, B))
    sim = pf.make_simulator("ode", hostemu=False)
    xn, y, st = _device_step(sim, inp, 0, 0)
    assert (xn[B] == X_GUARD).all() and (y[B] == X_GUARD).all() and st[B] == ST_GUARD
    assert np.array_equal(st[:B] & 0xFF, pf.expected_status(ref, 0)[:B])
    assert (pf.relerr(xn[:B], ref["x"][:B]) < np.where(ref["explicit"][:B], 1e-9, 2e-9)).all()
