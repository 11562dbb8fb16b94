"""The rows of Z_p of the condensing of the four-edge sweep (csrc/dompc_quad.h, eval_edge_quad step 8) as DPP operands against the
staged copy in LDS they replace - the cases and the switches of tests/test_gpu_quad_dpp.py.

The condensing takes entry [k][i] of Z_p from lane i of the row of 16 lanes as the DPP operand of its multiply-add; the build with
-DDOMPC_QUAD_LDS=1 writes the columns to LDS and reads the rows back behind wave barriers.  Both feed every multiply-add the same
operands in the same order, so every output of a solve has the same bits.  The forward pass (phase_forward_quads) is the same code in
both builds; the cases still cover its shapes (partial quads, the fallback branch), since it consumes what the sweep stored.  The quad
path has no host twin (it is compiled out under DOMPC_HOST_EMU): the comparison runs on the device only."""
import node_pack_common as npc

COMPARISON_DEFS = "DOMPC_QUAD_LDS=1"
# every quad through the pivoting fallback (no pivot passes the test): the condensing of the quad path is abandoned after its
# elimination, the forward pass takes its wave-uniform fallback branch and reads the stored inverse
FALLBACK_DEFS = "DOMPC_GJ_U=1e9"

# (id, example, build_mpc keywords, edges)
CASES = [
    # one partial quad and no next quad: rows of lanes beyond the last edge repeat it and take part in every cross-lane read
    ("CSTR_two_edges", "CSTR", dict(n_horizon=2, n_robust=0), 2),
    # one full quad, one quad with a single active row, and the model's nl_cons rows (they keep reading dy from LDS)
    ("CSTR_five_edges", "CSTR", dict(n_horizon=5, n_robust=0), 5),
    # three active rows in the last quad, branching at the root, no nl_cons rows
    ("industrial_poly_N3_robust1", "industrial_poly", dict(n_horizon=3, n_robust=1), 27),
]
IDS = [c[0] for c in CASES]
FALLBACK_CASE = CASES[2]


def joined(*defs):
    """DOMPC_DEFS of a build with several sets of switches (the order is part of the build's name)"""
    return " ".join(d for d in defs if d)


def edges_of(mpc):
    return int(mpc.structure.n_edges)


cold_solve = npc.cold_solve
batch_solve = npc.batch_solve
assert_same_bits = npc.assert_same_bits
assert_finite = npc.assert_finite
WS_FILL = npc.WS_FILL
