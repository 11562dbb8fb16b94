"""The per-edge operands of the forward pass with four edges per wavefront (csrc/dompc_quad.h, phase_forward_quads) staged one quad
ahead by LDS-DMA against the loop that loads them at the top of the quad - the cases and the switches of
tests/test_gpu_forward_stage.py.

The default build requests dx_n, du, the residuals, Sigma_w | r_w and d nu of a wavefront's NEXT quad into a staging area of its LDS
region while the current quad is computed and takes the index records of a quad from a request one quad ahead; the build with
-DDOMPC_FWD_STAGE=0 loads the operands at the top of the quad that consumes them.  A model whose LDS region has no room for the
staging area (the CSTR) keeps that loop in both builds: its cases pin that the switch changes nothing else.  Both feed every multiply-add the same operands in the same order, so every output of a solve has
the same bits.  The quad path has no host twin (it is compiled out under DOMPC_HOST_EMU): the comparison runs on the device only."""
import ctypes as C

import node_pack_common as npc

COMPARISON_DEFS = "DOMPC_FWD_STAGE=0"
# every quad through the pivoting fallback: the forward pass reads the stored inverse with plain loads while a DMA is in flight
FALLBACK_DEFS = "DOMPC_GJ_U=1e9"

# (id, example, build_mpc keywords, edges)
CASES = [
    # one partial quad: the prologue's request is the only one, rows beyond the last edge take the last edge's operands
    ("CSTR_two_edges", "CSTR", dict(n_horizon=2, n_robust=0), 2),
    # two quads, so exactly one request inside the loop; the last quad has a single active row; the model has nl_cons rows, whose
    # plain loads are issued while the DMA is in flight
    ("CSTR_five_edges", "CSTR", dict(n_horizon=5, n_robust=0), 5),
    # seven quads: as a batch one wavefront walks all of them and uses the staging area seven times; the quads of the branching
    # level come first, the last quad has three active rows
    ("industrial_poly_N3_robust1", "industrial_poly", dict(n_horizon=3, n_robust=1), 27),
]
IDS = [c[0] for c in CASES]
FALLBACK_CASE = CASES[2]
POISON_CASES = CASES[1:]
# one problem alone on ONE workgroup of four wavefronts (DOMPC_WIDE=0): twelve quads, wavefront w takes the quads w, w + 4, w + 8
STRIDE_CASE = ("industrial_poly_N5_robust1", "industrial_poly", dict(n_horizon=5, n_robust=1), 45)
# DOMPC_LDS_FILL: the wavefronts' LDS regions start as this value - an operand read from the staging area before it has landed, or from
# a slot that was never staged, is a NaN
LDS_FILL = "nan"


def joined(*defs):
    """DOMPC_DEFS of a build with several sets of switches (the order is part of the build's name)"""
    return " ".join(d for d in defs if d)


def edges_of(mpc):
    return int(mpc.structure.n_edges)


class Facts(C.Structure):
    """dompc_shape_facts (include/dompc_ipm.h)"""
    _fields_ = [("n_edges", C.c_int32), ("n_leaves", C.c_int32), ("edges_per_wave", C.c_int32), ("el_size", C.c_int64),
                ("slots64", C.c_int32), ("slots256", C.c_int32), ("n_slots", C.c_int32), ("block", C.c_int32),
                ("block_auto", C.c_int32), ("sharded", C.c_int32)]


class Overrides(C.Structure):
    """dompc_shape_overrides"""
    _fields_ = [("wide", C.c_int32), ("wide_spread", C.c_int32), ("wide_block", C.c_int32)]


class Shape(C.Structure):
    """dompc_shape"""
    _fields_ = [("block", C.c_int32), ("grid", C.c_int32), ("wide", C.c_int32), ("wide_spread", C.c_int32)]


def quads_of_wavefront_zero(mpc, wide):
    """(quads wavefront 0 takes, their stride) when one problem is solved alone under DOMPC_WIDE=`wide`, from the launch-shape
    function of the runtime (csrc/dompc_shape.h).  el_size: the largest region with which four wavefronts share a workgroup - the
    four-edge models are far below it, and every smaller region gives the same shape."""
    n_edges = edges_of(mpc)
    f = Facts(n_edges=n_edges, n_leaves=9, edges_per_wave=mpc.S.edges_per_wavefront, el_size=4992, slots64=2048, slots256=512,
              n_slots=1, block=256, block_auto=1, sharded=0)
    s = Shape()
    assert mpc.S._lib.dompc_launch_shape(C.byref(f), C.byref(Overrides(wide, -1, 0)), 1, C.byref(s)) == 0
    ng = s.grid * s.block // 64
    nq = (n_edges + 3) // 4
    return len(range(0, nq, ng)), ng


cold_solve = npc.cold_solve
batch_solve = npc.batch_solve
assert_same_bits = npc.assert_same_bits
assert_finite = npc.assert_finite
WS_FILL = npc.WS_FILL
