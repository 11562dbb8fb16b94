"""TEST-ONLY builder of the host emulation of the sensitivity-based MPC law: csrc/dompc_asmpc.hip + dompc_asmpc_runtime.cpp compiled by
g++ with -DDOMPC_HOST_EMU (the lane values of dompc_lanes.h as 16 slots, the law step as a loop over the batch) into tests/_hostemu/.
Never loaded by the product."""
from hostemu_build import OUT, _hostemu


def asmpc_hostemu_library(header_text: str, model_hash: str, out_dir: str = OUT, force: bool = False) -> str:
    return _hostemu("dompc_asmpc_hostemu", "dompc_asmpc_runtime.cpp", "dompc_asmpc.hip", "DOMPC_ASMPC_HEADER", "asmpc_gen", [], "law ",
                    header_text, model_hash, out_dir, force)
