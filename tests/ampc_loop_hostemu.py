"""TEST-ONLY builder of the host emulation of the fused approximate-MPC loop: csrc/dompc_ampc_loop.hip (which includes dompc_plant.hip
and dompc_ampc.hip, the texts that ship) + dompc_plant_runtime.cpp compiled by g++ with -DDOMPC_HOST_EMU into tests/_hostemu/ - one
library per (plant, network shape) pair, a superset of the plant's own host library.  Never loaded by the product."""
import os

from do_mpc_amd.build import _write_atomic
from hostemu_build import OUT, _hostemu


def ampc_loop_hostemu_library(plant_header: str, network_header: str, pair_hash: str, out_dir: str = OUT, force: bool = False) -> str:
    """the pair's host library; the plant's header goes the way of every _hostemu header, the network's is written next to it and
    named by a second -D"""
    os.makedirs(out_dir, exist_ok=True)
    net = os.path.join(out_dir, f"ampc_loop_net_{pair_hash}.h")
    if not (os.path.exists(net) and open(net).read() == network_header):
        _write_atomic(net, network_header)
    return _hostemu("dompc_ampc_loop_hostemu", "dompc_plant_runtime.cpp", "dompc_ampc_loop.hip", "DOMPC_PLANT_HEADER", "ampc_loop_plant_gen",
                    [f"-DDOMPC_AMPC_HEADER=\"{net}\""], "approximate-MPC loop ", plant_header, pair_hash, out_dir, force)


def on_pairs(sim, hostemu):
    """`sim` builds its pair objects on the host emulation (hostemu) or on the GPU"""
    sim._ampc_loop_lib = ampc_loop_hostemu_library if hostemu else None
    return sim
