"""What HipIpmSolver, Simulator and EKF share on their way to libdompc_ipm.so."""
import os

from . import build


def runtime_library() -> str:
    """Path of the built libdompc_ipm.so.  torch ships its own HIP runtime: it has to be the first one in the process, so torch is
    imported (when it is installed, and unless DOMPC_NO_TORCH_FIRST is set) before the library is."""
    if not os.environ.get("DOMPC_NO_TORCH_FIRST"):
        try:
            import torch          # noqa: F401
            torch.cuda.is_available()
        except ImportError:
            pass
    return build.runtime_library()


def check(rc, prefix: str, last_error, handle=None) -> None:
    """RuntimeError(prefix + the library's message) for a non-zero return code; `last_error`: the component's dompc_*_last_error,
    `handle` None after a failed create."""
    if rc != 0:
        raise RuntimeError(prefix + (last_error(handle) or b"?").decode())
