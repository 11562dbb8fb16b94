"""The reference's examples/lqr_examples/batch_reactor_lqr_dae templates (template_model.py, template_lqr.py, template_simulator.py)
run UN-EDITED through do_mpc_amd.casadi_compat: dae2odeconversion and linearize of the template's model give the gain and the design
header of the in-repo example (hashes pinned in tests/golden/lqr_dae_template_hashes.json), the template's DAE model lowers to the
text of the in-repo one, and symvar_type='MX' raises ValueError as the reference's test expects
(testing/test_batch_reactor_lqr_dae.py).  Needs the reference tree: skipped where it is absent."""
import importlib.util
import json
import os
import warnings

import numpy as np
import pytest

import lqr_common as lc
import lqr_dae_common as dc
from do_mpc_amd import casadi_compat
from do_mpc_amd.examples import CASES
from hostemu_build import OUT, plant_hostemu_library

REF = "/root/reference/examples/lqr_examples/batch_reactor_lqr_dae"
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


def test_unedited_templates_give_the_gain_and_the_headers_of_the_example(compat):
    tm, tl, ts = (_load(os.path.join(REF, f"template_{w}.py"), f"ref_batch_reactor_lqr_dae_{w}") for w in ("model", "lqr", "simulator"))
    ex = CASES["batch_reactor_lqr_dae"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        model, daemodel, linearmodel = tm.template_model()
        lqr = tl.template_lqr(linearmodel.discretize(0.5))
        ours = lc.setup_lqr(ex.build_lqr(ex.build_model(), setup=False), hostemu=True)
    assert daemodel._x.names == ["Ca", "Cb", "Ad", "Cain", "Cc"] and daemodel._u.vars["q"].shape == (1, 1)
    assert np.array_equal(linearmodel.sys_A, ex.build_model().sys_A) and np.array_equal(linearmodel.sys_B, ex.build_model().sys_B)
    assert np.array_equal(lqr.K, ours.K) and lqr.mode == ours.mode == "standard" and lqr.settings.n_horizon == ours.settings.n_horizon == 10
    pinned = json.load(open(os.path.join(lc.GOLDEN, "lqr_dae_template_hashes.json")))
    assert lqr.header() == ours.header() and next(iter(lqr._designs.values())).hash == pinned["batch_reactor_lqr_dae"]
    # the object of gains_at on the model with its algebraic state: the template's DAE model lowers to the text of the in-repo one
    ours_dae, lq = dc.design("batch_reactor", hostemu=True)
    hdr = lq.header(model)
    assert hdr == lq.header(ours_dae) and hdr.rsplit('LQR_MODEL_HASH "', 1)[1].split('"')[0] == pinned["batch_reactor_lqr_dae_gains_at"]
    # ... and the loop of main.py on the template's objects, against the stored run
    sim = ts.template_simulator(linearmodel)
    x0 = ex.X0.reshape(-1, 1)
    sim.x0 = x0
    lqr.set_setpoint(xss=ex.XSS, uss=lqr.model.get_steady_state(xss=ex.XSS))
    for _ in range(ex.N_STEPS):
        x0 = sim.make_step(lqr.make_step(x0))
    g = np.load(os.path.join(lc.GOLDEN, "batch_reactor_lqr_dae.npz"))
    for k in ("_x", "_u", "_time"):
        assert np.max(np.abs(sim.data[k] - g["simulator." + k])) < 1e-8, k
    assert sim.data["_z"].shape == g["simulator._z"].shape
    with pytest.raises(ValueError):
        tm.template_model("MX")
