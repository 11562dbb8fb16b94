"""The reference's examples/CSTR_approximate_mpc templates (template_model.py, template_mpc.py, template_simulator.py) run UN-EDITED
through do_mpc_amd.casadi_compat, `from do_mpc.approximateMPC import AMPCSampler, ApproxMPC, Trainer` resolves, and the flow of the
reference's testing/test_CSTR_approx_MPC.py runs up to approx_mpc.setup() - and one step further, on the host emulation of the
network kernel.  Needs the reference tree: skipped where it is absent."""
import importlib.util
import os

import numpy as np
import pytest

import ampc_common as ac
import hostemu
from do_mpc_amd import casadi_compat
from hostemu_build import OUT, plant_hostemu_library

REF = "/root/reference/examples/CSTR_approximate_mpc"
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not available")


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture()
def compat():
    """the stand-in modules, with the solver, Simulator.setup and ApproxMPC.setup on the host emulations"""
    names = casadi_compat.install()
    import do_mpc
    sim_setup, ampc_setup = do_mpc.simulator.Simulator.setup, do_mpc.approximateMPC.ApproxMPC.setup

    def sim_on_hostemu(self):
        hdr = self._lower()
        sim_setup(self, _lib_path=plant_hostemu_library(hdr, hdr.rsplit('PLANT_MODEL_HASH "', 1)[1].split('"')[0], OUT), _code_object="")
    do_mpc.simulator.Simulator.setup = sim_on_hostemu
    do_mpc.approximateMPC.ApproxMPC.setup = lambda self: ac.setup_ampc_with(ampc_setup, self)
    with hostemu.patched():
        yield
    do_mpc.simulator.Simulator.setup, do_mpc.approximateMPC.ApproxMPC.setup = sim_setup, ampc_setup
    casadi_compat.uninstall(names)


def test_unedited_templates_and_the_flow_of_the_references_test(compat):
    from do_mpc.approximateMPC import AMPCSampler, ApproxMPC, Trainer      # noqa: F401
    import do_mpc
    tm, tc, ts = (_load(os.path.join(REF, f"template_{w}.py"), f"ref_cstr_ampc_{w}") for w in ("model", "mpc", "simulator"))
    model = tm.template_model()
    mpc = tc.template_mpc(model, silence_solver=True)
    simulator = ts.template_simulator(model)
    estimator = do_mpc.estimator.StateFeedback(model)
    x0 = np.array([0.8, 0.5, 134.14, 130.0]).reshape(-1, 1)
    u0 = np.array([5.0, 0.0]).reshape(-1, 1)
    mpc.u0 = u0
    mpc.x0 = x0
    simulator.x0 = x0
    mpc.set_initial_guess()
    approx_mpc = ApproxMPC(mpc)
    approx_mpc.settings.n_hidden_layers = 1
    approx_mpc.settings.n_neurons = 50
    approx_mpc.setup()
    assert approx_mpc.flags["setup"] and approx_mpc.net.n_in == 6 and approx_mpc.net.n_out == 2
    assert np.array_equal(approx_mpc.x_range.numpy().ravel(), [1.9, 1.9, 90.0, 90.0, 95.0, 8500.0])
    # the template's controller carries the box of the stored network: load it and close the loop of main.py for a few steps
    approx_mpc.load_from_state_dict(ac.STORED)
    for _ in range(3):
        u0 = approx_mpc.make_step(x0, clip_to_bounds=True)
        x0 = estimator.make_step(simulator.make_step(u0))
        assert u0.shape == (2, 1) and np.all(u0.ravel() >= [5.0, -8500.0]) and np.all(u0.ravel() <= [100.0, 0.0])
    sampler, trainer = AMPCSampler(mpc), Trainer(approx_mpc)
    assert sampler.settings.n_samples is None and trainer.settings.batch_size == 1000 and trainer.scheduler_settings.patience == 10
