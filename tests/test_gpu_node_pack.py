"""Packed per-node index records (KArgs::node_pack) and the stores the batch solve no longer makes, on the device: the default build
against the build that keeps the table look-ups (-DDOMPC_NODE_PACK=0) bit for bit, and every case once more on a workspace pre-filled
with an all-ones byte pattern (DOMPC_WS_FILL) - the matrix-core recursion stores rows < NX of a chain node's value function only, the
gradient entries of the edge unknowns are zeroed once per problem, and measure() no longer reads lam after a trial evaluation: a read of
an entry that is no longer written would come back as NaN.  The cases are those of tests/test_node_pack.py plus the shipped CSTR, each
as one problem alone (the wide launch shape) and as a batch of 4096 (one wavefront per problem, the batch-only code object)."""
import numpy as np
import pytest

import node_pack_common as npc
from do_mpc_amd.examples import CASES

pytestmark = pytest.mark.gpu


def make_mpc(name, **kw):
    ex = CASES[name]
    return ex.build_mpc(ex.build_model(), **kw)


@pytest.mark.parametrize("cid,name,kw", npc.CASES_GPU, ids=npc.IDS_GPU)
def test_one_problem_alone(cid, name, kw, monkeypatch):
    packed_mpc, packed = npc.cold_solve(make_mpc, name, kw, monkeypatch, "")
    tables_mpc, tables = npc.cold_solve(make_mpc, name, kw, monkeypatch, npc.COMPARISON_DEFS)
    assert packed_mpc.S.code_object_path != tables_mpc.S.code_object_path
    npc.assert_same_bits(packed, tables, cid)
    monkeypatch.setenv("DOMPC_WS_FILL", npc.WS_FILL)
    _, filled = npc.cold_solve(make_mpc, name, kw, monkeypatch, "")
    npc.assert_finite(filled, cid)
    npc.assert_same_bits(packed, filled, cid + " on a filled workspace")


@pytest.mark.parametrize("cid,name,kw", npc.CASES_GPU, ids=npc.IDS_GPU)
def test_batch_of_4096(cid, name, kw, monkeypatch):
    packed_mpc, packed = npc.batch_solve(make_mpc, name, kw, monkeypatch, "")
    tables_mpc, tables = npc.batch_solve(make_mpc, name, kw, monkeypatch, npc.COMPARISON_DEFS)
    for mpc in (packed_mpc, tables_mpc):
        assert mpc.S.batch_object_state == 1          # (the batch-only sibling of this build ran)
    assert packed_mpc.S.code_object_path != tables_mpc.S.code_object_path
    npc.assert_same_bits(packed, tables, cid)
    _, filled = npc.batch_solve(make_mpc, name, kw, monkeypatch, "", fill=True)
    npc.assert_finite(filled, cid)
    npc.assert_same_bits(packed, filled, cid + " on a filled workspace")


def test_batched_sensitivities_read_the_node_records():
    """make_step_batch(..., sensitivities=True) on shape-family member s3: mode 3 (dompc_sens_kernel) runs the sweep and both Riccati
    passes on the node records"""
    mp = pytest.MonkeyPatch()
    try:
        name = "shape_family:s3"
        _, packed = npc.batch_solve(make_mpc, name, {}, mp, "", B=8, sensitivities=True)
        _, tables = npc.batch_solve(make_mpc, name, {}, mp, npc.COMPARISON_DEFS, B=8, sensitivities=True)
    finally:
        mp.undo()
    npc.assert_same_bits(packed, tables, name)
    assert packed["ok"].all()
    for key in ("du0dx0", "du0du_prev", "dxdp", "residual_step", "ok"):
        assert np.array_equal(packed[key], tables[key], equal_nan=True), key
