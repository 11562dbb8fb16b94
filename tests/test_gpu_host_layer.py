"""The start of every create (csrc/dompc_host.h: load the code object, look its kernels up, ask the info kernel) on the MI355X: a
code object without the component's kernels is refused before anything is launched, and the refusal leaves the process able to set
the component up correctly."""
import os

import numpy as np
import pytest

from do_mpc_amd import build
from do_mpc_amd.examples import triple_tank as tt

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_filter_create_refuses_the_plants_code_object_and_a_correct_setup_steps_afterwards():
    model = tt.build_model()
    hdr = tt.build_simulator(model, setup=False)._lower()
    plant_object = build.plant_code_object(hdr, hdr.rsplit('PLANT_MODEL_HASH "', 1)[1].split('"')[0])
    with pytest.raises(RuntimeError, match="lacks the filter kernels"):
        tt.build_ekf(model, _lib_path=build.runtime_library(), _code_object=plant_object)
    # the first step of the reference's triple-tank run, to the bound of the smoke test
    g = np.load(os.path.join(GOLDEN, "triple_tank.npz"))
    ekf = tt.build_ekf(model)
    ekf.x0 = tt.X0_EST
    ekf.set_initial_guess()
    ekf.make_step(g["simulator._y"][0].reshape(-1, 1), tt.U_CONST.reshape(-1, 1), 1e-3 * np.eye(3), 1e-2 * np.eye(1))
    assert float(np.max(np.abs(ekf.data["_x"][0] - g["estimator._x"][0]))) < 1e-8
