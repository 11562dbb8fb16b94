"""TEST-ONLY builder of the host emulation of the approximate-MPC step: csrc/dompc_ampc.hip + dompc_ampc_runtime.cpp compiled by g++
with -DDOMPC_HOST_EMU (the matrix step of dompc_ampc_wave.h as 64 lane slots and std::fmaf in k order) into tests/_hostemu/.  Never
loaded by the product."""
from hostemu_build import OUT, _hostemu


def ampc_hostemu_library(header_text: str, model_hash: str, out_dir: str = OUT, force: bool = False) -> str:
    return _hostemu("dompc_ampc_hostemu", "dompc_ampc_runtime.cpp", "dompc_ampc.hip", "DOMPC_AMPC_HEADER", "ampc_gen", [], "network ",
                    header_text, model_hash, out_dir, force)
