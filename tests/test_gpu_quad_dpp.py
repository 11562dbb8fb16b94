"""Rows of Z_p of the four-edge sweep's condensing through DPP (the default build) against the build that keeps the staged copy in LDS
(-DDOMPC_QUAD_LDS=1), bit for bit on x, g, lam_g, lam_x, f and every statistic but the timers; each case as one problem alone (the
wide launch: several wavefronts share the quads, the next quad of a wavefront is ng quads ahead), as a batch of 4096 (one wavefront per
problem, the batch-only code object) and once more on a workspace pre-filled with an all-ones byte pattern (DOMPC_WS_FILL): the default
build no longer writes the Wb region of LDS - a read of it, or of anything else that is not written first, would come back as NaN or
as other bits.  Cases: tests/quad_dpp_common.py."""
import pytest

import quad_dpp_common as qc
from do_mpc_amd.examples import CASES

pytestmark = pytest.mark.gpu


def make_mpc(name, **kw):
    ex = CASES[name]
    return ex.build_mpc(ex.build_model(), **kw)


def check_quad(mpc, edges, batch):
    assert mpc.S.edges_per_wavefront == 4
    assert qc.edges_of(mpc) == edges
    if batch:
        assert mpc.S.batch_object_state == 1          # (the batch-only sibling of this build ran)


def compare_alone(cid, name, kw, edges, monkeypatch, extra=""):
    dpp_mpc, dpp = qc.cold_solve(make_mpc, name, kw, monkeypatch, extra)
    lds_mpc, lds = qc.cold_solve(make_mpc, name, kw, monkeypatch, qc.joined(extra, qc.COMPARISON_DEFS))
    for mpc in (dpp_mpc, lds_mpc):
        check_quad(mpc, edges, False)
    assert dpp_mpc.S.code_object_path != lds_mpc.S.code_object_path
    qc.assert_finite(dpp, cid)
    qc.assert_same_bits(dpp, lds, cid)
    monkeypatch.setenv("DOMPC_WS_FILL", qc.WS_FILL)
    _, filled = qc.cold_solve(make_mpc, name, kw, monkeypatch, extra)
    qc.assert_finite(filled, cid)
    qc.assert_same_bits(dpp, filled, cid + " on a filled workspace")
    return dpp


def compare_batch(cid, name, kw, edges, monkeypatch, extra=""):
    dpp_mpc, dpp = qc.batch_solve(make_mpc, name, kw, monkeypatch, extra)
    lds_mpc, lds = qc.batch_solve(make_mpc, name, kw, monkeypatch, qc.joined(extra, qc.COMPARISON_DEFS))
    for mpc in (dpp_mpc, lds_mpc):
        check_quad(mpc, edges, True)
    assert dpp_mpc.S.code_object_path != lds_mpc.S.code_object_path
    qc.assert_finite(dpp, cid)
    qc.assert_same_bits(dpp, lds, cid)
    _, filled = qc.batch_solve(make_mpc, name, kw, monkeypatch, extra, fill=True)
    qc.assert_finite(filled, cid)
    qc.assert_same_bits(dpp, filled, cid + " on a filled workspace")
    return dpp


@pytest.mark.parametrize("cid,name,kw,edges", qc.CASES, ids=qc.IDS)
def test_one_problem_alone(cid, name, kw, edges, monkeypatch):
    compare_alone(cid, name, kw, edges, monkeypatch)


@pytest.mark.parametrize("cid,name,kw,edges", qc.CASES, ids=qc.IDS)
def test_batch_of_4096(cid, name, kw, edges, monkeypatch):
    compare_batch(cid, name, kw, edges, monkeypatch)


def test_every_quad_through_the_fallback_alone(monkeypatch):
    """DOMPC_GJ_U=1e9 in both builds: no pivot passes the test, the sweep stores the inverses through the wavefront-per-edge path and
    the forward pass reads them on its fallback branch"""
    cid, name, kw, edges = qc.FALLBACK_CASE
    compare_alone(cid + " fallback", name, kw, edges, monkeypatch, extra=qc.FALLBACK_DEFS)


def test_every_quad_through_the_fallback_batch(monkeypatch):
    cid, name, kw, edges = qc.FALLBACK_CASE
    compare_batch(cid + " fallback", name, kw, edges, monkeypatch, extra=qc.FALLBACK_DEFS)
