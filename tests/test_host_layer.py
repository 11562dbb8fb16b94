"""The start of every create, which the runtimes share through csrc/dompc_host.h (open the code object, ask its info kernel, compare
with the description), on the host emulation of the plant, the filter, the network and the law: a code object of another model is
refused by name, and the refusal leaves nothing behind that keeps a correct create from working.  (tests/test_lqr.py has the design's.)"""
import pytest

import ampc_common
import asmpc_common
import ekf_common
import simulator_common
from do_mpc_amd import _native


def _network():
    ampc = ampc_common.network(4, 2, True, hostemu=True, n_hidden_layers=1, n_neurons=1)
    ampc._handle()
    return ampc


def _law():
    asmpc = asmpc_common.make_asmpc(asmpc_common.stub_mpc(1, 1), hostemu=True)
    asmpc._handle()
    return asmpc


# (component of the C ABI, a correct setup on the smallest model the suites lower, a size of the description the info kernel reports)
CASES = [("plant", lambda: simulator_common.make_simulator("oscillating_masses", hostemu=True), "nx"),
         ("ekf", lambda: ekf_common.make_ekf("triple_tank", hostemu=True), "nx"),
         ("ampc", _network, "n_neurons"),
         ("asmpc", _law, "nu")]


@pytest.mark.parametrize("component, make, size", CASES, ids=[c[0] for c in CASES])
def test_create_refuses_a_code_object_of_another_model(monkeypatch, component, make, size):
    seen = []
    create = _native.Native.create
    monkeypatch.setattr(_native.Native, "create", lambda self, desc: (seen.append((self, desc)), create(self, desc))[1])
    owner = make()                        # (keeps the library and the strings of the description alive)
    native, good = seen[-1]
    assert native.h is not None

    def attempt(**changed):
        desc = type(good).from_buffer_copy(good)
        for k, v in changed.items():
            setattr(desc, k, v)
        n = _native.Native(component, None, None)
        n.lib = native.lib
        n.create(desc)
        return n

    with pytest.raises(RuntimeError, match="different model dimensions"):
        attempt(**{size: getattr(good, size) + 1})
    with pytest.raises(RuntimeError, match="model hash mismatch"):
        attempt(model_hash=b"0123456789abcdef")
    again = attempt()
    assert again.h is not None
    again.close()
    owner.close()
