"""Model-output entries of the four-edge loops read by all lanes (the default build) against the reads inside lane branches
(-DDOMPC_MO_BRANCHED=1), bit for bit on x, g, lam_g, lam_x, f and every statistic but the timers: one problem alone, a batch of 4096 (one
wavefront per problem, the batch-only code object), every quad through the fallback, workspace and LDS pre-filled with NaN patterns,
and the same batch twice.  Cases: tests/mo_reads_common.py."""
import pytest

import mo_reads_common as mc
from do_mpc_amd.examples import CASES

pytestmark = pytest.mark.gpu

# solves of the comparison build on clean memory, computed once: (case id, "alone" / "batch", extra switches) -> (code object, outputs)
_REFERENCE = {}


def make_mpc(name, **kw):
    ex = CASES[name]
    return ex.build_mpc(ex.build_model(), **kw)


def check_quad(mpc, edges, batch):
    assert mpc.S.edges_per_wavefront == 4
    assert mc.edges_of(mpc) == edges
    if batch:
        assert mpc.S.batch_object_state == 1          # (the batch-only sibling of this build ran)


def solve(cid, name, kw, edges, monkeypatch, defs, batch, fill=False):
    run = mc.batch_solve if batch else mc.cold_solve
    mpc, got = run(make_mpc, name, kw, monkeypatch, defs, fill=True) if fill else run(make_mpc, name, kw, monkeypatch, defs)
    check_quad(mpc, edges, batch)
    return mpc.S.code_object_path, got


def reference(cid, name, kw, edges, monkeypatch, batch, extra=""):
    key = (cid, batch, extra)
    if key not in _REFERENCE:
        path, got = solve(cid, name, kw, edges, monkeypatch, mc.joined(extra, mc.COMPARISON_DEFS), batch)
        for a in got.values():
            if hasattr(a, "setflags"):
                a.setflags(write=False)
        _REFERENCE[key] = (path, got)
    return _REFERENCE[key]


def compare(cid, name, kw, edges, monkeypatch, batch, extra=""):
    path, got = solve(cid, name, kw, edges, monkeypatch, extra, batch)
    ref_path, ref = reference(cid, name, kw, edges, monkeypatch, batch, extra)
    assert path != ref_path
    mc.assert_finite(got, cid)
    mc.assert_same_bits(got, ref, cid)


@pytest.mark.parametrize("cid,name,kw,edges", mc.CASES, ids=mc.IDS)
def test_one_problem_alone(cid, name, kw, edges, monkeypatch):
    compare(cid, name, kw, edges, monkeypatch, False)


@pytest.mark.parametrize("cid,name,kw,edges", mc.CASES, ids=mc.IDS)
def test_batch_of_4096(cid, name, kw, edges, monkeypatch):
    compare(cid, name, kw, edges, monkeypatch, True)


def test_every_quad_through_the_fallback_alone(monkeypatch):
    """DOMPC_GJ_U=1e9 in both builds: no pivot passes the test - the sweep leaves every quad behind its elimination, the forward pass
    forms its columns from the record and takes the stored inverse"""
    cid, name, kw, edges = mc.FALLBACK_CASE
    compare(cid + " fallback", name, kw, edges, monkeypatch, False, extra=mc.FALLBACK_DEFS)


def test_every_quad_through_the_fallback_batch(monkeypatch):
    cid, name, kw, edges = mc.FALLBACK_CASE
    compare(cid + " fallback", name, kw, edges, monkeypatch, True, extra=mc.FALLBACK_DEFS)


@pytest.mark.parametrize("cid,name,kw,edges", mc.CASES, ids=mc.IDS)
def test_poisoned_workspace_and_lds(cid, name, kw, edges, monkeypatch):
    """the default build on a workspace of 0xff bytes and LDS regions that start as NaN, against the comparison build on clean memory:
    every lane reads entries whose value its select throws away, and none of them may reach an output"""
    _, ref = reference(cid, name, kw, edges, monkeypatch, True)
    monkeypatch.setenv("DOMPC_LDS_FILL", mc.LDS_FILL)
    _, got = solve(cid, name, kw, edges, monkeypatch, "", True, fill=True)
    mc.assert_finite(got, cid)
    mc.assert_same_bits(got, ref, cid + " on poisoned memory")
    _, ref_alone = reference(cid, name, kw, edges, monkeypatch, False)
    monkeypatch.setenv("DOMPC_LDS_FILL", mc.LDS_FILL)
    monkeypatch.setenv("DOMPC_WS_FILL", mc.WS_FILL)
    _, alone = solve(cid, name, kw, edges, monkeypatch, "", False)
    mc.assert_finite(alone, cid)
    mc.assert_same_bits(alone, ref_alone, cid + " alone on poisoned memory")


def test_same_bits_twice(monkeypatch):
    """the batch solve of the seven-quad case twice with the default build"""
    cid, name, kw, edges = mc.CASES[2]
    _, a = solve(cid, name, kw, edges, monkeypatch, "", True)
    _, b = solve(cid, name, kw, edges, monkeypatch, "", True)
    mc.assert_finite(a, cid)
    mc.assert_same_bits(a, b, cid + " twice")
