"""`DoMPCDifferentiator.differentiate_batch` on the HIP path (twin of test_differentiator_batch.py)."""
import contextlib

import pytest

import differentiator_batch_common as bc
from test_gpu_parity import make_mpc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("reduction", [False, True])
@pytest.mark.parametrize("name", ["batch_reactor", "CSTR"])
def test_batch_equals_the_single_point_path(name, reduction):
    bc.check_batch_equals_single_point(make_mpc, name, reduction)


def test_two_members_with_different_active_sets_match_the_oracles_sparse_kkt_solve():
    bc.check_against_oracle(make_mpc)


def test_du0dx0_matches_central_differences_of_complete_resolves():
    bc.check_against_resolves(make_mpc)


def test_permuted_batch_single_member_more_items_than_slots_and_mixed_columns():
    bc.check_indexing(make_mpc)


def test_failed_members_stay_local():
    bc.check_failed_members_stay_local(make_mpc)


def test_singular_reduced_systems_are_reported_per_member():
    bc.check_singular_reduced_systems_are_reported(make_mpc)


def test_make_step_batch_with_sensitivities_and_the_refused_checks():
    bc.check_make_step_batch_flag(make_mpc)


def test_refusals_of_the_differentiator_reach_the_batched_call():
    bc.check_refusals(make_mpc, contextlib.nullcontext)


def test_batched_asmpc_example_equals_the_formula_from_single_point_sensitivities():
    bc.check_asmpc(make_mpc)


def test_sampler_stores_sensitivities_only_when_asked(tmp_path):
    bc.check_sampler_files(make_mpc, tmp_path)


def test_device_resident_call_equals_the_host_array_call():
    """differentiate_batch_device on tensors of the solver's device: no host copies, same numbers as differentiate_batch"""
    import numpy as np
    import torch
    from do_mpc_amd.differentiator import DoMPCDifferentiator
    mpc, r = bc.solved_batch(make_mpc, "batch_reactor")
    nd = DoMPCDifferentiator(mpc, active_set_reduction=True)
    ref = nd.differentiate_batch(r)
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.array(r[k], dtype=np.float64)).to(dev) for k in ("x", "lam_g", "p")}
    stats = torch.from_numpy(np.frombuffer(r["stats"].tobytes(), dtype=np.uint8).copy()).to(dev)
    out = nd.differentiate_batch_device(t["x"], t["lam_g"], stats, t["p"])
    torch.cuda.synchronize()
    assert out["dxdp"].is_cuda and np.array_equal(out["dxdp"].cpu().numpy(), ref["dxdp"])
    assert np.array_equal(out["ok"].cpu().numpy(), ref["ok"]) and np.array_equal(out["residual_step"].cpu().numpy(), ref["residual_step"])
