"""The reads of the compact model-output record in the two four-edge loops (csrc/dompc_quad.h: eval_edge_quad, phase_forward_quads)
executed by all lanes against the reads inside a lane branch each - the cases and the switches of tests/test_gpu_mo_reads.py.

Most variable entries of the record feed a select `(j == bb) ? t_ : v`.  The default build reads such an entry through a volatile
pointer: every lane of the wavefront reads it (the address is the same for the 16 lanes of an edge), the reads of a row are issued
back to back, the select throws the value away on the lanes that do not own it.  The build with -DDOMPC_MO_BRANCHED=1 has plain reads,
which the compiler sinks into an exec-mask branch of their own: the former instruction stream.  Same values from the same addresses and
the selects of the source in both, so every output of a solve has the same bits.  What is new in the default build: lanes read entries
they do not use, rows beyond the last edge of a partial quad among them (they take the last edge's record) - a NaN there must not
reach an output.  The quad path has no host twin (it is compiled out under DOMPC_HOST_EMU): the comparison runs on the device only."""
import forward_stage_common as fc
import node_pack_common as npc

COMPARISON_DEFS = "DOMPC_MO_BRANCHED=1"
# every quad through the pivoting fallback: the sweep returns behind the elimination, the forward pass takes its fallback branch
FALLBACK_DEFS = "DOMPC_GJ_U=1e9"

# (id, example, build_mpc keywords, edges)
CASES = [
    # one partial quad: the rows beyond the last edge now read the last edge's record on every lane
    ("CSTR_two_edges", "CSTR", dict(n_horizon=2, n_robust=0), 2),
    # nl_cons rows: the reads of mo_nl_val (row values in front of the lane branch, Jacobian rows, Hessian)
    ("CSTR_five_edges", "CSTR", dict(n_horizon=5, n_robust=0), 5),
    # seven quads, the branching level first, the last quad with three rows, the last-level reads of mo_mt_val
    ("industrial_poly_N3_robust1", "industrial_poly", dict(n_horizon=3, n_robust=1), 27),
]
IDS = [c[0] for c in CASES]
FALLBACK_CASE = CASES[2]
# DOMPC_LDS_FILL: the wavefronts' LDS regions start as this value
LDS_FILL = "nan"

joined = fc.joined
edges_of = fc.edges_of
cold_solve = npc.cold_solve
batch_solve = npc.batch_solve
assert_same_bits = npc.assert_same_bits
assert_finite = npc.assert_finite
WS_FILL = npc.WS_FILL
