"""The reference's examples/triple_tank_ekf templates (template_model.py, template_ekf.py) run UN-EDITED through
do_mpc_amd.casadi_compat: they lower to the same filter header as the in-repo example (the same gfx950 code object, whose hash is
pinned in tests/golden/ekf_template_hashes.json and checked again on the GPU) and reproduce the stored run of the reference.
Needs the reference tree: skipped where it is absent."""
import importlib.util
import json
import os

import pytest

import ekf_common as ec
from do_mpc_amd import casadi_compat
from do_mpc_amd.examples import triple_tank

REF = "/root/reference/examples/triple_tank_ekf"
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not available")


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture()
def compat():
    names = casadi_compat.install()
    yield
    casadi_compat.uninstall(names)


def test_unedited_triple_tank_templates_lower_to_the_example_and_reproduce_the_golden_estimator(compat):
    import do_mpc
    tm = _load(os.path.join(REF, "template_model.py"), "ref_tt_ekf_tm")
    te = _load(os.path.join(REF, "template_ekf.py"), "ref_tt_ekf_te")
    model = tm.template_model()
    orig_setup = do_mpc.estimator.EKF.setup

    def setup_on_hostemu(self):
        hdr = self._lower()
        h = hdr.rsplit('EKF_MODEL_HASH "', 1)[1].split('"')[0]
        orig_setup(self, _lib_path=ec.ekf_hostemu_library(hdr, h), _code_object="")
    do_mpc.estimator.EKF.setup = setup_on_hostemu
    try:
        ekf = te.template_ekf(model)
    finally:
        do_mpc.estimator.EKF.setup = orig_setup
    ours = triple_tank.build_ekf(triple_tank.build_model(), setup=False)
    assert ekf.generated_header == ours._lower()
    assert ekf.model_hash == json.load(open(os.path.join(ec.GOLDEN, "ekf_template_hashes.json")))["triple_tank"]
    ec.check_golden_triple_tank(ekf)
