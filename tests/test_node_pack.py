"""Packed per-node index records (KArgs::node_pack) on the test-only host emulation: the default build against the build that keeps the
table look-ups (-DDOMPC_NODE_PACK=0), bit for bit.  The host emulation runs the generic Riccati recursion and the generic chain walk of the
forward pass: they read the records through the same accessors (csrc/dompc_edge.h) as the matrix-core recursion and the four-chain walk
of the device, which tests/test_gpu_node_pack.py compares in the same way."""
import pytest

import hostemu
import node_pack_common as npc
from do_mpc_amd.examples import CASES


def make_mpc(name, **kw):
    ex = CASES[name]
    with hostemu.patched():
        return ex.build_mpc(ex.build_model(), **kw)


@pytest.mark.parametrize("cid,name,kw", npc.CASES_CPU, ids=npc.IDS_CPU)
def test_node_records_give_the_bits_of_the_table_lookups(cid, name, kw, monkeypatch):
    """x, g, lam_g, lam_x, f and every statistic of a cold solve"""
    packed_mpc, packed = npc.cold_solve(make_mpc, name, kw, monkeypatch, "")
    tables_mpc, tables = npc.cold_solve(make_mpc, name, kw, monkeypatch, npc.COMPARISON_DEFS)
    assert packed_mpc.S._lib._name != tables_mpc.S._lib._name        # (two libraries: the switch reached the compiler)
    assert packed["stats"]["iter_count"] >= 1
    npc.assert_same_bits(packed, tables, cid)
