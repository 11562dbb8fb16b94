"""The reference's examples/lqr_examples/{oscillating_masses_discrete_lqr, CSTR_lqr} templates (template_model.py, template_lqr.py,
template_simulator.py) run UN-EDITED through do_mpc_amd.casadi_compat: they give the gain of the in-repo examples, lower to the same
design headers (hashes pinned in tests/golden/lqr_template_hashes.json and checked again on the GPU) and close the loop of the stored
run.  Needs the reference tree: skipped where it is absent."""
import importlib.util
import json
import os
import warnings

import numpy as np
import pytest

import lqr_common as lc
from do_mpc_amd import casadi_compat
from do_mpc_amd.examples import CASES
from hostemu_build import OUT, plant_hostemu_library

REF = "/root/reference/examples/lqr_examples"
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not available")


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture()
def compat():
    """the stand-in modules, with LQR.setup and Simulator.setup on the host emulation"""
    names = casadi_compat.install()
    import do_mpc
    lqr_setup, sim_setup = do_mpc.controller.LQR.setup, do_mpc.simulator.Simulator.setup

    def sim_on_hostemu(self):
        hdr = self._lower()
        sim_setup(self, _lib_path=plant_hostemu_library(hdr, hdr.rsplit('PLANT_MODEL_HASH "', 1)[1].split('"')[0], OUT), _code_object="")
    do_mpc.controller.LQR.setup = lambda self, **kw: lqr_setup(self, _lib_path=lc.lqr_hostemu_library, _code_object="")
    do_mpc.simulator.Simulator.setup = sim_on_hostemu
    yield
    do_mpc.controller.LQR.setup, do_mpc.simulator.Simulator.setup = lqr_setup, sim_setup
    casadi_compat.uninstall(names)


@pytest.mark.parametrize("name, folder", [("oscillating_masses_lqr", "oscillating_masses_discrete_lqr"), ("cstr_lqr", "CSTR_lqr")])
def test_unedited_templates_give_the_gain_and_the_headers_of_the_example(compat, name, folder):
    d = os.path.join(REF, folder)
    tm, tl, ts = (_load(os.path.join(d, f"template_{w}.py"), f"ref_{name}_{w}") for w in ("model", "lqr", "simulator"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        if name == "cstr_lqr":
            plant, linear = tm.template_model()
        else:
            plant = linear = tm.template_model()
        lqr = tl.template_lqr(linear)
    sim = ts.template_simulator(plant)
    ex, plant_ours, ours = lc.example(name, hostemu=True)
    assert np.array_equal(lqr.K, ours.K) and lqr.mode == ours.mode and lqr.settings.n_horizon == ours.settings.n_horizon
    pinned = json.load(open(os.path.join(lc.GOLDEN, "lqr_template_hashes.json")))
    assert lqr.header() == ours.header() and next(iter(lqr._designs.values())).hash == pinned[name]
    # the object of gains_at: the template's plant model lowers to the text of the in-repo one
    hdr = lqr.header(plant)
    assert hdr == ours.header(plant_ours) and hdr.rsplit('LQR_MODEL_HASH "', 1)[1].split('"')[0] == pinned[name + "_gains_at"]
    # ... and the loop of main.py on the template's objects
    x0 = ex.X0.reshape(-1, 1)
    sim.x0 = x0
    if name == "cstr_lqr":
        lqr.set_setpoint(xss=ex.XSS, uss=ex.USS)
    for _ in range(ex.N_STEPS):
        x0 = sim.make_step(lqr.make_step(x0))
    g = np.load(os.path.join(lc.GOLDEN, name + ".npz"))
    ex_, eu_ = lc.relerr(sim.data["_x"], g["simulator._x"]), lc.relerr(sim.data["_u"], g["simulator._u"])
    print(f"{name} (templates): relerr _x = {ex_:.3e}, _u = {eu_:.3e}")
    assert ex_ < 1e-8 and eu_ < (1.2e-7 if name == "cstr_lqr" else 1e-8)      # (tests/test_lqr.py::test_cstr_loop_reproduces_the_stored_run)
    assert CASES[name] is ex
