"""Per-edge operands of the four-edge forward pass staged one quad ahead by LDS-DMA (the default build) against the loop with the loads at the top of the quad (-DDOMPC_FWD_STAGE=0), bit for bit on x, g, lam_g, lam_x, f and every
statistic but the timers: one problem alone (the wide launch: the next quad of a wavefront is ng quads ahead), a batch of 4096 (one
wavefront per problem walks every quad, the batch-only code object), one problem on a single workgroup (three quads per wavefront at a
stride of four), every quad through the fallback, and workspace and LDS pre-filled with NaN patterns.  Cases:
tests/forward_stage_common.py."""
import pytest

import forward_stage_common as fc
from do_mpc_amd.examples import CASES

pytestmark = pytest.mark.gpu


def make_mpc(name, **kw):
    ex = CASES[name]
    return ex.build_mpc(ex.build_model(), **kw)


def check_quad(mpc, edges, batch):
    assert mpc.S.edges_per_wavefront == 4
    assert fc.edges_of(mpc) == edges
    if batch:
        assert mpc.S.batch_object_state == 1          # (the batch-only sibling of this build ran)


def compare_alone(cid, name, kw, edges, monkeypatch, extra=""):
    st_mpc, st = fc.cold_solve(make_mpc, name, kw, monkeypatch, extra)
    ld_mpc, ld = fc.cold_solve(make_mpc, name, kw, monkeypatch, fc.joined(extra, fc.COMPARISON_DEFS))
    for mpc in (st_mpc, ld_mpc):
        check_quad(mpc, edges, False)
    assert st_mpc.S.code_object_path != ld_mpc.S.code_object_path
    fc.assert_finite(st, cid)
    fc.assert_same_bits(st, ld, cid)
    return st_mpc, st


def compare_batch(cid, name, kw, edges, monkeypatch, extra=""):
    st_mpc, st = fc.batch_solve(make_mpc, name, kw, monkeypatch, extra)
    ld_mpc, ld = fc.batch_solve(make_mpc, name, kw, monkeypatch, fc.joined(extra, fc.COMPARISON_DEFS))
    for mpc in (st_mpc, ld_mpc):
        check_quad(mpc, edges, True)
    assert st_mpc.S.code_object_path != ld_mpc.S.code_object_path
    fc.assert_finite(st, cid)
    fc.assert_same_bits(st, ld, cid)
    return st_mpc, st


@pytest.mark.parametrize("cid,name,kw,edges", fc.CASES[:2], ids=fc.IDS[:2])
def test_one_problem_alone(cid, name, kw, edges, monkeypatch):
    compare_alone(cid, name, kw, edges, monkeypatch)


@pytest.mark.parametrize("cid,name,kw,edges", fc.CASES, ids=fc.IDS)
def test_batch_of_4096(cid, name, kw, edges, monkeypatch):
    compare_batch(cid, name, kw, edges, monkeypatch)


def test_three_quads_per_wavefront_at_a_stride_of_four(monkeypatch):
    """one problem alone on one workgroup: wavefront 0 takes the quads 0, 4 and 8 of twelve - its requests are for quads that are not
    its neighbours, and the staging area is written three times"""
    cid, name, kw, edges = fc.STRIDE_CASE
    monkeypatch.setenv("DOMPC_WIDE", "0")             # (read by the runtime at every solve; cold_solve takes it back)
    st_mpc, st = fc.cold_solve(make_mpc, name, kw, monkeypatch, "")
    monkeypatch.setenv("DOMPC_WIDE", "0")
    ld_mpc, ld = fc.cold_solve(make_mpc, name, kw, monkeypatch, fc.COMPARISON_DEFS)
    for mpc in (st_mpc, ld_mpc):
        check_quad(mpc, edges, False)
    assert st_mpc.S.code_object_path != ld_mpc.S.code_object_path
    n_quads, ng = fc.quads_of_wavefront_zero(st_mpc, 0)
    assert n_quads >= 3 and ng >= 2, (n_quads, ng)
    fc.assert_finite(st, cid)
    fc.assert_same_bits(st, ld, cid)


def test_every_quad_through_the_fallback_alone(monkeypatch):
    """DOMPC_GJ_U=1e9 in both builds: no pivot passes the test, and the fallback branch of the forward pass reads the stored inverse
    with plain loads while the request for the next quad is in flight"""
    cid, name, kw, edges = fc.FALLBACK_CASE
    compare_alone(cid + " fallback", name, kw, edges, monkeypatch, extra=fc.FALLBACK_DEFS)


def test_every_quad_through_the_fallback_batch(monkeypatch):
    cid, name, kw, edges = fc.FALLBACK_CASE
    compare_batch(cid + " fallback", name, kw, edges, monkeypatch, extra=fc.FALLBACK_DEFS)


@pytest.mark.parametrize("cid,name,kw,edges", fc.POISON_CASES, ids=[c[0] for c in fc.POISON_CASES])
def test_poisoned_workspace_and_lds(cid, name, kw, edges, monkeypatch):
    """the default build on a workspace of 0xff bytes and LDS regions that start as NaN, against the comparison build on clean memory"""
    _, ld = fc.batch_solve(make_mpc, name, kw, monkeypatch, fc.COMPARISON_DEFS)
    monkeypatch.setenv("DOMPC_LDS_FILL", fc.LDS_FILL)
    mpc, st = fc.batch_solve(make_mpc, name, kw, monkeypatch, "", fill=True)
    check_quad(mpc, edges, True)
    fc.assert_finite(st, cid)
    fc.assert_same_bits(st, ld, cid + " on poisoned memory")
    monkeypatch.setenv("DOMPC_LDS_FILL", fc.LDS_FILL)
    monkeypatch.setenv("DOMPC_WS_FILL", fc.WS_FILL)
    _, alone = fc.cold_solve(make_mpc, name, kw, monkeypatch, "")
    _, ld_alone = fc.cold_solve(make_mpc, name, kw, monkeypatch, fc.COMPARISON_DEFS)
    fc.assert_finite(alone, cid)
    fc.assert_same_bits(alone, ld_alone, cid + " alone on poisoned memory")


def test_same_bits_twice(monkeypatch):
    """the batch solve of the seven-quad case twice with the default build: a race between a request and a read of the staged
    loop would not repeat its bits"""
    cid, name, kw, edges = fc.CASES[2]
    _, a = fc.batch_solve(make_mpc, name, kw, monkeypatch, "")
    _, b = fc.batch_solve(make_mpc, name, kw, monkeypatch, "")
    fc.assert_finite(a, cid)
    fc.assert_same_bits(a, b, cid + " twice")
