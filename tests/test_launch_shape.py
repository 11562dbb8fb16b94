"""The launch shape of a solve (csrc/dompc_shape.h) through dompc_launch_shape of a host-emulation library: the shapes the defaults
choose today, the conditions every shape must meet - among them the co-residency of the wide mode, whose device-scope barrier hangs on
a grid that is not resident at once - and the agreement of the batch shape (sweep, sensitivities) with the solve's.  No GPU, no handle."""
import ctypes as C
import itertools
import random

import pytest

import hostemu
from do_mpc_amd.examples import CASES


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


@pytest.fixture(scope="module")
def lib():
    ex = CASES["CSTR"]
    with hostemu.patched():
        mpc = ex.build_mpc(ex.build_model())
    return mpc.S._lib


def facts(**kw):
    f = dict(n_edges=180, n_leaves=9, edges_per_wave=4, el_size=2000, slots64=2048, slots256=512, n_slots=512, block=256,
             block_auto=1, sharded=0)
    f.update(kw)
    return Facts(**f)


def shape(lib, f, B, wide=-1, wide_spread=-1, wide_block=0):
    s = Shape()
    assert lib.dompc_launch_shape(C.byref(f), C.byref(Overrides(wide, wide_spread, wide_block)), B, C.byref(s)) == 0
    return s.block, s.grid, s.wide, s.wide_spread


TREE = dict(n_edges=4008, n_leaves=243)
# (B, facts that differ from facts(), overrides, (block, grid, wide, wide_spread))
ANCHORS = [
    (1, {}, {}, (128, 24, 24, 1)),                                   # the shipped 9-scenario problem alone: 24 x 128 threads
    (1, dict(edges_per_wave=1), {}, (256, 12, 12, 1)),
    (1, dict(TREE), {}, (256, 64, 64, 1)),                           # the 243-leaf tree: 64 x 256
    (1, dict(n_edges=20, n_leaves=1), {}, (256, 16, 2, 0)),          # two workgroups, one XCD
    (4, dict(TREE), {}, (256, 256, 64, 1)),
    (5, dict(TREE), {}, (256, 128, 16, 0)),
    (16, {}, {}, (256, 128, 8, 0)),
    (64, {}, {}, (256, 256, 4, 0)),
    (65, {}, {}, (256, 65, 1, 0)),
    (1024, {}, {}, (256, 512, 1, 0)),
    (1024, dict(n_slots=2048), {}, (256, 512, 1, 0)),                # capped by slots256
    (4096, dict(n_slots=2048), {}, (64, 2048, 1, 0)),                # one wavefront per problem
    (1, dict(slots64=64, slots256=16, n_slots=1), {}, (128, 16, 16, 1)),         # co-residency shrinks K
    (16, dict(slots64=400, slots256=100, n_slots=16), {}, (256, 96, 6, 0)),
    (1, dict(edges_per_wave=1, el_size=5760, slots64=512, slots256=128, n_slots=1), {}, (128, 12, 12, 1)),     # LDS forces 128 threads
    (1, dict(TREE, edges_per_wave=1, sharded=1), {}, (256, 128, 16, 0)),
    (1, dict(TREE, edges_per_wave=1), dict(wide_block=512), (512, 64, 64, 1)),
    (1, dict(TREE, edges_per_wave=1), dict(wide=32, wide_spread=1), (256, 32, 32, 1)),
]


@pytest.mark.parametrize("B,fk,ok,want", ANCHORS)
def test_anchor_shapes(lib, B, fk, ok, want):
    assert shape(lib, facts(**fk), B, **ok) == want


def test_bad_arguments_are_refused(lib):
    f, o, s = facts(), Overrides(-1, -1, 0), Shape()
    assert lib.dompc_launch_shape(C.byref(f), C.byref(o), 0, C.byref(s)) == 1
    assert lib.dompc_launch_shape(None, C.byref(o), 1, C.byref(s)) == 1
    assert lib.dompc_launch_shape(C.byref(f), None, 1, C.byref(s)) == 1
    assert lib.dompc_launch_shape(C.byref(f), C.byref(o), 1, None) == 1


def _sweep(n=4000):
    """fixed-seed draws (facts, B); every el_size fits 256 threads"""
    rng = random.Random(20240607)
    Bs = [1, 2, 3, 4, 5, 8, 9, 16, 32, 33, 64, 65, 100, 1024, 4095, 4096, 20000]
    edges = [1, 7, 8, 20, 45, 56, 180, 720, 2047, 2048, 4008, 20000]
    leaves = [1, 9, 27, 243, 1000]
    s256s = [1, 2, 8, 16, 40, 100, 256, 512, 1024]
    for _ in range(n):
        s256 = rng.choice(s256s)
        s64 = s256 * rng.choice([1, 2, 4])
        max_batch = rng.choice([1, 16, 64, 4096, 32768])
        yield facts(n_edges=rng.choice(edges), n_leaves=rng.choice(leaves), edges_per_wave=rng.choice([1, 4]),
                    el_size=rng.choice([500, 2000, 4900]), slots64=s64, slots256=s256,
                    n_slots=min(max_batch, s64 if max_batch >= 4096 else s256)), rng.choice(Bs)


def test_invariants_of_the_default_shapes(lib):
    n_wide = n_spread = 0
    for f, B in _sweep():
        block, grid, wide, spread = shape(lib, f, B)
        ctx = ({k: getattr(f, k) for k, _ in Facts._fields_}, B, (block, grid, wide, spread))
        assert grid >= 1 and block in (64, 128, 256), ctx
        assert wide >= 1 and spread in (0, 1), ctx
        if wide > 1:
            assert B <= 64 and B <= f.n_slots, ctx
            assert grid <= f.slots256, ctx            # co-residency: every workgroup of the launch on the chip at once
            if spread:
                assert B * wide <= 2048, ctx
            else:
                assert wide <= 32, ctx
        else:
            assert spread == 0 and grid <= min(B, max(f.n_slots, 1)), ctx
        n_wide += wide > 1
        n_spread += spread
    assert n_wide > 100 and n_spread > 20       # (the sweep reaches both modes)


def _batch_shape(f, n):
    """the three lines of dompc_launch::batch_shape for an el_size that fits 256 threads"""
    block = (64 if n >= 4096 else 256) if f.block_auto else f.block
    cap = f.slots256 if (f.block_auto and block != 64 and f.slots256 < f.n_slots) else f.n_slots
    return block, min(n, cap)


def test_batch_shape_agrees_with_the_solve_shape(lib):
    """One workgroup per problem: a solve launches the shape of the sweep and of the sensitivities for as many items.  DOMPC_WIDE=0
    leaves the batch shape as it is for every B."""
    n = 0
    for f, B in itertools.chain(_sweep(), ((facts(block_auto=0, block=b), B) for b in (64, 128, 256) for B in (1, 100, 600, 5000))):
        block, grid, wide, spread = shape(lib, f, B)
        assert shape(lib, f, B, wide=0) == _batch_shape(f, B) + (1, 0)
        if wide == 1:
            assert (block, grid) == _batch_shape(f, B)
            n += 1
    assert n > 1000
