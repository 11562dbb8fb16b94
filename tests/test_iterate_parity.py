"""The two copies of the iterate inside a workspace slot (csrc: SLOT_PARITY, prob_flip): the line search writes every trial point into the
copy that is not live and accepting it flips which copy is live, so a solve may end with the live iterate in either copy.  Nothing of that
may leak from one solve into the next one that uses the slot.  Host emulation of the kernels (tests/hostemu.py): it has ONE slot
(dompc_runtime.cpp; DOMPC_SLOTS=1 asks the same of the device runtime), so a batch runs its members one after the other through it."""
import numpy as np
import pytest

import hostemu
from do_mpc_amd.examples import CASES


def make_mpc(name, **kw):
    ex = CASES[name]
    with hostemu.patched():
        return ex.build_mpc(ex.build_model(), **kw)


def _x0_batch(name, B):
    X0 = np.asarray(CASES[name].X0, dtype=float).ravel()
    rng = np.random.default_rng(11)
    return X0[None, :] * (1.0 + 0.01 * rng.uniform(-1, 1, size=(B, X0.size)))


# CSTR: nl_cons rows with slacks, unused variables with and without bounds; batch_reactor: regularised iterations, no nl_cons rows;
# oscillating masses: a discrete model
@pytest.mark.parametrize("defs", ["", "DOMPC_FINE_ITEMS=1"])
@pytest.mark.parametrize("name", ["CSTR", "batch_reactor", "oscillating_masses"])
def test_members_of_a_batch_through_one_slot_equal_the_problems_solved_alone(name, defs, monkeypatch):
    monkeypatch.setenv("DOMPC_SLOTS", "1")
    monkeypatch.setenv("DOMPC_DEFS", defs)
    B = 6
    X0 = _x0_batch(name, B)
    mpc = make_mpc(name, max_batch=B)
    assert mpc.S.num_slots == 1
    r = mpc.make_step_batch(X0)
    st = r["stats"]
    assert np.all(st["success"] == 1)
    # (an odd number of accepted steps ends a solve in the second copy: the case that can leak into the next member)
    assert np.any(st["iter_count"][:-1] % 2 == 1), st["iter_count"]
    for b in range(B):
        alone = make_mpc(name)          # a fresh handle: a workspace that no solve has used
        ra = alone.make_step_batch(X0[b:b + 1])
        for key in ("x", "g", "lam_x", "lam_g", "f", "u0"):
            assert np.array_equal(r[key][b], ra[key][0]), (name, defs, b, key)
        for key in st.dtype.names:
            if not key.startswith("t_"):
                assert st[key][b] == ra["stats"][key][0], (name, defs, b, key)
