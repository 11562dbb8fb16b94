"""Extended Kalman filter (do_mpc_amd/ekf.py, csrc/dompc_ekf.hip) on the CPU: the kernel text that ships, compiled for the host
(tests/ekf_common.py: ekf_hostemu_library), against the reference's stored run of examples/triple_tank_ekf and against a numpy / scipy
twin of the reference's recursion."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import ekf_common as ec
from do_mpc_amd import build, sym
from do_mpc_amd.ekf import EKF
from do_mpc_amd.examples import CASES, triple_tank
from do_mpc_amd.model import Model


# ---------------------------------------------------------------------------------------------- 1, 2: the stored run of the reference
def test_twin_reproduces_the_golden_estimator_trajectory():
    """the numpy twin alone, fed the stored measurements, against `estimator._x` of results_triple_tank_ekf.pkl within the reference
    test's own 1e-8 (measured: 0.0): the twin is a sound yardstick where no fixture exists"""
    g = np.load(os.path.join(ec.GOLDEN, "triple_tank.npz"))
    tw = ec.Twin(triple_tank.build_model())
    x, P = triple_tank.X0_EST.copy(), np.eye(3)
    for k in range(200):
        x, P = tw.step(x, P, g["simulator._y"][k], triple_tank.U_CONST, ec.Q_TT, ec.R_TT, p=[2.0], tvp=[0.5 if k < 50 else 1.0])
        assert np.max(np.abs(x - g["estimator._x"][k])) < 1e-8, k


def test_triple_tank_example_reproduces_the_golden_estimator_records():
    ekf = triple_tank.build_ekf(triple_tank.build_model(), setup=False)
    ec.setup_on_hostemu(ekf)
    ec.check_golden_triple_tank(ekf)
    assert ekf.model_hash == json.load(open(os.path.join(ec.GOLDEN, "ekf_template_hashes.json")))["triple_tank"]


# ---------------------------------------------------------------------------------------------- 3: Model.get_linear_system_matrices
@pytest.mark.parametrize("name", ["triple_tank", "CSTR", "rotating_masses"])
def test_linear_system_matrices_equal_the_jacobians(name):
    m = CASES[name].build_model()
    rng = np.random.default_rng(2)
    x, u = 1.0 + rng.uniform(0, 1, m.n_x), rng.uniform(0, 1, m.n_u)
    tvp, p = 0.5 + rng.uniform(0, 1, m.n_tvp), 0.5 + rng.uniform(0, 1, m.n_p)
    A, B, C, D = m.get_linear_system_matrices(x, u, tvp=tvp, p=p)
    ins = [m._x.cat, m._u.cat, m._tvp.cat, m._p.cat, m._w.cat, m._v.cat]
    args = (x, u, tvp, p, np.zeros(m.n_w), np.zeros(m.n_v))
    for got, expr, wrt in ((A, m._rhs, m._x.cat), (B, m._rhs, m._u.cat), (C, m._y.cat, m._x.cat), (D, m._y.cat, m._u.cat)):
        J = sym.jacobian(expr, wrt)
        want = np.asarray(sym.Function("J", ins, [J]).eval(*args)[0], float).reshape(J.shape, order="F")
        assert isinstance(got, np.ndarray) and got.shape == J.shape
        assert np.array_equal(got, want)
    if name == "rotating_masses":
        assert np.any(D != 0.0)                    # the measured set-points: y depends on u directly
    As, Bs, Cs, Ds = m.get_linear_system_matrices()
    assert (As.shape, Bs.shape, Cs.shape, Ds.shape) == ((m.n_x, m.n_x), (m.n_x, m.n_u), (m.n_y, m.n_x), (m.n_y, m.n_u))
    assert isinstance(As, sym.SX) and not As.is_constant() or name == "rotating_masses"
    # partly numeric: still symbolic in what was not given
    A2 = m.get_linear_system_matrices(xss=x)[0]
    if m.n_p and name != "triple_tank":
        assert isinstance(A2, sym.SX)


# ---------------------------------------------------------------------------------------------- 4: evaluation point of C
def test_measurement_jacobian_is_evaluated_at_the_prior_estimate():
    ec.check_evaluation_point(hostemu=True)


# ---------------------------------------------------------------------------------------------- 5: batch semantics
@pytest.mark.parametrize("shared_qr", [True, False])
@pytest.mark.parametrize("B", [1, 3, 4, 9])
@pytest.mark.parametrize("name", ["triple_tank", "rotating_masses"])
def test_a_filter_does_not_depend_on_its_slot_in_the_batch(name, B, shared_qr):
    ekf = ec.make_ekf(name, hostemu=True)
    ec.check_batch_semantics(ekf, B, shared_qr, offset=2.0 if name == "triple_tank" else 0.0)


# ---------------------------------------------------------------------------------------------- 6: continuous models
@pytest.mark.parametrize("name", ["rotating_masses", "CSTR"])
def test_continuous_models_against_the_twin(name):
    """Five steps, abstol = reltol = 1e-10, x and P against scipy's DOP853 on the augmented system at rtol = atol = 1e-12.
    Bound: max(1e-9, 10 x (twin at 1e-12 - twin at 1e-13)); 1e-9 relative with floor 1 is what the plant integrator meets with the
    same pair and safety factor (simulator_common.check_against_scipy).  Measured on the host emulation:
      rotating_masses (nx 8, ny 5, D != 0): kernel - twin 1.3e-11, twin(1e-12) - twin(1e-13) 5.0e-12 -> bound 1e-9
      CSTR (nx 4, ny 4):                    kernel - twin 8.4e-13, twin(1e-12) - twin(1e-13) 7.9e-14 -> bound 1e-9"""
    ec.check_continuous(name, hostemu=True)


# ---------------------------------------------------------------------------------------------- 7: surface
def _tank_ekf():
    return triple_tank.build_ekf(triple_tank.build_model(), setup=False)


def test_p0_setter_validates_like_the_reference():
    ekf = _tank_ekf()
    assert np.array_equal(ekf.P0, np.eye(3))
    with pytest.raises(TypeError, match="numpy.ndarray"):
        ekf.P0 = [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]
    with pytest.raises(ValueError, match="2D"):
        ekf.P0 = np.ones(3)
    with pytest.raises(ValueError, match="square"):
        ekf.P0 = np.ones((3, 2))
    with pytest.raises(ValueError, match=r"shape \(3, 3\)"):
        ekf.P0 = np.eye(4)
    ekf.P0 = 2.0 * np.eye(3)
    assert np.array_equal(ekf.P0, 2.0 * np.eye(3))


def test_make_step_asserts_the_shapes_of_q_and_r_and_the_call_order():
    ekf = _tank_ekf()
    y, u = np.zeros((1, 1)), np.zeros((2, 1))
    with pytest.raises(AssertionError, match="not setup"):
        ekf.make_step(y, u, ec.Q_TT, ec.R_TT)
    ec.setup_on_hostemu(ekf)
    with pytest.raises(AssertionError, match="Initial guess"):
        ekf.make_step(y, u, ec.Q_TT, ec.R_TT)
    ekf.x0 = triple_tank.X0_EST
    ekf.set_initial_guess()
    with pytest.raises(AssertionError, match="Q_k must be a square matrix of shape"):
        ekf.make_step(y, u, np.eye(2), ec.R_TT)
    with pytest.raises(AssertionError, match="R_k must be a square matrix of shape"):
        ekf.make_step(y, u, ec.Q_TT, np.eye(3))


def test_missing_parameter_functions_raise_the_reference_exceptions():
    m = triple_tank.build_model()
    ekf = EKF(m)
    ekf.settings.t_step = 1
    with pytest.raises(Exception, match="time-varying parameters defined in model"):
        ec.setup_on_hostemu(ekf)
    tv = ekf.get_tvp_template()
    ekf.set_tvp_fun(lambda t: tv)
    with pytest.raises(Exception, match="obtain the parameters defined in model"):
        ec.setup_on_hostemu(ekf)
    ekf2 = EKF(m)
    with pytest.raises(ValueError, match="t_step"):
        ekf2.setup()


def test_models_outside_the_kernel_are_refused_by_name():
    dae = CASES["oscillating_masses_dae"].build_model()
    ekf = EKF(dae)
    ekf.settings.t_step = 0.5
    with pytest.raises(NotImplementedError, match="structured HIP backend: .*algebraic states"):
        ekf.setup()
    m = Model("discrete")
    x = m.set_variable("_x", "x", shape=(17, 1))
    m.set_rhs("x", 0.5 * x)
    m.setup()
    ekf = EKF(m)
    ekf.settings.t_step = 1.0
    with pytest.raises(NotImplementedError, match="structured HIP backend: .*more than 16 states"):
        ekf.setup()
    m = Model("discrete")
    x = m.set_variable("_x", "x")
    m.set_meas("y", x * x, meas_noise=False)
    m.set_rhs("x", x * x, process_noise=True)
    m.setup()
    # (additive noise leaves A and C free of it; a product with the noise does not)
    m2 = Model("discrete")
    x = m2.set_variable("_x", "x")
    w = m2.set_variable("_w", "w")
    m2.set_rhs("x", x * x * (1.0 + w))
    m2.setup()
    EKF(m)._lower()
    with pytest.raises(NotImplementedError, match="structured HIP backend: .*depends on _w, _v or _z"):
        EKF(m2)._lower()


def test_singular_s_returns_the_a_priori_estimate_with_status_bit_1():
    ekf = ec.make_ekf("triple_tank", hostemu=True)
    x = np.array([[2.0, 2.8, 2.7]])
    u = triple_tank.U_CONST
    r = ekf.step_batch(x, np.zeros((1, 3, 3)), np.array([[2.5]]), u, np.zeros((3, 3)), np.zeros((1, 1)))
    assert r["status"][0] == 2
    m = ekf.model
    p, tvp = ec.p_tvp(ekf)
    x_prior = np.asarray(m._rhs_fun.eval(x[0], u, np.zeros(0), tvp, p, np.zeros(0))[0], float).ravel()
    assert np.array_equal(r["x"][0], x_prior) and np.array_equal(r["P"][0], np.zeros((3, 3)))
    assert np.all(np.isfinite(r["x"])) and np.all(np.isfinite(r["P"]))
    # a measurement that is not finite does not reach the estimate either
    r = ekf.step_batch(x, np.eye(3)[None], np.array([[np.nan]]), u, ec.Q_TT, ec.R_TT)
    assert r["status"][0] == 2 and np.all(np.isfinite(r["x"])) and np.all(np.isfinite(r["P"]))


def test_step_limit_sets_status_bit_0():
    ekf = ec.make_ekf("rotating_masses", hostemu=True, max_steps=3)
    m, x, P, u, Q, R, ys = ec.continuous_case("rotating_masses")
    r = ekf.step_batch(x[None], P[None], ys[0][None], u, Q, R)
    assert r["status"][0] & 1 and np.all(np.isfinite(r["x"])) and np.all(np.isfinite(r["P"]))


def test_results_of_filter_and_simulator_are_saved_and_loaded(tmp_path):
    from do_mpc_amd import data
    from do_mpc_amd.estimator import EKF as FromEstimator
    assert FromEstimator is EKF
    model = triple_tank.build_model()
    ekf = triple_tank.build_ekf(model, setup=False)
    ec.setup_on_hostemu(ekf)
    sim = triple_tank.build_simulator(model, setup=False)
    ekf.x0 = triple_tank.X0_EST
    ekf.set_initial_guess()
    for k in range(3):
        ekf.make_step(np.array([[2.7]]), triple_tank.U_CONST.reshape(-1, 1), ec.Q_TT, ec.R_TT)
    data.save_results([ekf, sim], result_name="tt", result_path=str(tmp_path) + "/", overwrite=True)
    res = data.load_results(str(tmp_path / "tt.pkl"))
    assert set(res) == {"estimator", "simulator"}
    assert np.array_equal(res["estimator"]["_x"], ekf.data["_x"]) and res["estimator"]["_x"].shape == (3, 3)
    assert np.array_equal(res["estimator"]["_time"].ravel(), [1.0, 2.0, 3.0])


# ---------------------------------------------------------------------------------------------- unequal problems in one wavefront
# (the host emulation runs one group at a time: "equals the single call" is trivially true here and is the point of the GPU twins in
# tests/test_gpu_ekf.py; what the CPU side establishes are the preconditions, the status words and the figures against the twin)
@pytest.mark.parametrize("B", [8, 7, 5])
def test_neighbours_with_unequal_step_counts_equal_their_single_calls(B):
    """eight CSTR filters of 51, 52, 54, 55, 57, 59, 61 and 64 integration steps; B = 7 and 5 with the slowest one last.  Measured on
    the host emulation: member 3 against the twin 6.9e-14 (twin(1e-12) - twin(1e-13) = 6.1e-15, bound 1e-9)"""
    ec.check_unequal_steps(ec.make_ekf("CSTR", hostemu=True), B)


@pytest.mark.parametrize("last", [None, 1, 2, 3], ids=lambda v: "B8" if v is None else f"B7-member{v}-last")
def test_failing_filters_leave_their_neighbours_alone(last):
    """status [0 2 3 2 0 0 0 0] and steps [51 52 1 25 57 59 61 64] on the host emulation; the a-priori estimates handed out with bit 1
    against the twin's prediction: 6.4e-13 and 4.1e-13 (bound 1e-9)"""
    ec.check_failures_beside_neighbours(ec.make_ekf("CSTR", hostemu=True), last)


def test_step_limit_inside_a_wavefront():
    """max_steps = 57: status [0 0 0 0 0 1 1 1], steps [51 52 54 55 57 57 57 57] on the host emulation"""
    ec.check_step_limit_inside_a_wavefront(hostemu=True)


@pytest.mark.parametrize("slot", [2, 4])
def test_singular_s_beside_neighbours(slot):
    ec.check_status_bit_1_beside_neighbours(hostemu=True, slot=slot)


def test_step_limit_of_a_batch():
    ec.check_step_limit(hostemu=True)


@pytest.mark.parametrize("name", ["rotating_masses", "CSTR", "oscillating_masses"])
def test_elimination_of_s_with_row_swaps(name):
    """full, non-symmetric R per filter: partial pivoting on S' takes another row order in every filter.  Measured on the host
    emulation, kernel - twin: rotating_masses (n_y 5, six different orders, cond(S) <= 35.7) 1.3e-12, CSTR (n_y 4, three orders,
    cond(S) <= 21.7) 5.9e-12, both at the bound 1e-9 of the integration tests; oscillating_masses (discrete, n_y 2, swap and no swap
    alternate, cond(S) <= 4.4) 8.3e-17 at 1e-10"""
    ec.check_row_swaps(name, hostemu=True)


# ---------------------------------------------------------------------------------------------- compiler evidence
def _kernel_metadata(code_object, tmp_dir):
    """(private segment bytes, spilled VGPRs) of dompc_ekf_kernel from the code object's amdhsa metadata"""
    tool = None
    for cand in (shutil.which("llvm-readelf"), os.path.join(os.path.dirname(os.path.realpath(build._hipcc())), "..", "llvm", "bin", "llvm-readelf"),
                 "/opt/rocm/llvm/bin/llvm-readelf"):
        if cand and os.path.exists(cand):
            tool = cand
            break
    if tool is None:
        pytest.skip("llvm-readelf not found next to hipcc")
    raw = open(code_object, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    if raw.startswith(magic):                      # hipcc --genco wraps the ELF in an offload bundle: take the gfx950 entry out
        import struct
        pos, elf = len(magic) + 8, None
        for _ in range(struct.unpack_from("<Q", raw, len(magic))[0]):
            off, size, tlen = struct.unpack_from("<QQQ", raw, pos)
            triple = raw[pos + 24:pos + 24 + tlen].decode()
            pos += 24 + tlen
            if "gfx950" in triple:
                elf = raw[off:off + size]
        assert elf is not None, "no gfx950 entry in the code object"
        code_object = str(tmp_dir / "kernel.elf")
        with open(code_object, "wb") as f:
            f.write(elf)
    notes = subprocess.run([tool, "--notes", code_object], stdout=subprocess.PIPE, text=True, check=True).stdout
    blocks = notes.split("- .agpr_count")
    blk = next(b for b in blocks if ".name:           dompc_ekf_kernel" in b or ".name: dompc_ekf_kernel" in b.replace("  ", " "))
    field = lambda k: int(next(l for l in blk.splitlines() if l.strip().startswith(k)).split(":")[1])      # noqa: E731
    return field(".private_segment_fixed_size"), field(".vgpr_spill_count")


@pytest.mark.parametrize("name", ["triple_tank", "oscillating_masses"])
def test_discrete_filters_use_no_scratch(name, tmp_path):
    """every register array of the kernel is indexed at compile time: the discrete filters need no scratch memory and spill no VGPR"""
    try:
        build._hipcc()
    except build.BuildError:
        pytest.skip("hipcc not available")
    ekf = EKF(CASES[name].build_model(**ec.MODEL_KW.get(name, {})))
    hdr = ekf._lower()
    co = build.ekf_code_object(hdr, hdr.rsplit('EKF_MODEL_HASH "', 1)[1].split('"')[0])
    scratch, spills = _kernel_metadata(co, tmp_path)
    assert scratch == 0 and spills == 0
