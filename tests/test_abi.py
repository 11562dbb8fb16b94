"""The C-ABI shared library: loads, exports every symbol include/dompc_ipm.h declares, and fails
loudly (no CPU fallback) when there is no GPU.  No compute calls here."""
import ctypes
import os
import re

import pytest

from do_mpc_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "dompc_ipm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dompc_[a-z_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(build.runtime_library())
    names = _declared_functions()
    assert len(names) >= 12 and "dompc_riccati_kind" in names and "dompc_edges_per_wavefront" in names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/dompc_ipm.h but not exported"


def test_product_simulator_refuses_to_run_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from do_mpc_amd.examples import oscillating_masses as ex
    from do_mpc_amd.simulator import Simulator
    sim = Simulator(ex.build_model())
    sim.set_param(t_step=0.5)
    with pytest.raises(RuntimeError, match="HIP|GPU|hip"):
        sim.setup()


def test_stats_struct_layout_matches_header():
    from do_mpc_amd.solver import STATS_DTYPE, Stats
    assert ctypes.sizeof(Stats) == STATS_DTYPE.itemsize == 10 * 4 + 7 * 8      # (8 counters + n_watchdog + one reserved word, then 7 doubles)


def test_product_solver_refuses_to_run_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from do_mpc_amd.examples import oscillating_masses as ex
    with pytest.raises(RuntimeError, match="HIP|GPU|hip"):
        ex.build_mpc(ex.build_model())
