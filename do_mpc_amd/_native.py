"""What HipIpmSolver, Simulator, EKF, LQR, ApproxMPC and ASMPC share on their way to libdompc_ipm.so."""
import ctypes as C
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


class Native:
    """One native handle of a component: the library it comes from, dompc_<component>_create / _destroy / _last_error and the
    messages of a failed call.  `component`: "plant", "ekf", ... or "" for the solver (dompc_create); `bind`: library path -> CDLL
    with the component's argtypes; `code_object`: (header, model hash) -> path of the built gfx950 code object.
    TEST-ONLY: `lib_path` names the library instead of libdompc_ipm.so - a path, or a callable (header, model hash) -> path - and
    `given_code_object` the code object to load with it: "" selects the host emulation of the kernels."""

    def __init__(self, component: str, bind, code_object, lib_path=None, given_code_object=None):
        self._name = "dompc_" + component if component else "dompc"
        self._bind, self._code_object = bind, code_object
        self._lib_path, self._given = lib_path, given_code_object
        self.lib = None
        self.h = None

    def load(self, header: str, model_hash: str) -> str:
        """binds the library (once) and returns the path of the code object: built now, or the one given with the library"""
        given = self._lib_path is not None
        if self.lib is None:
            path = self._lib_path(header, model_hash) if callable(self._lib_path) else self._lib_path
            self.lib = self._bind(path if given else runtime_library())
        return (self._given or "") if given else self._code_object(header, model_hash)

    def create(self, desc) -> None:
        """a new handle from the component's description; one that exists is destroyed first"""
        self.close()
        h = C.c_void_p()
        last_error = getattr(self.lib, self._name + "_last_error")
        check(getattr(self.lib, self._name + "_create")(C.byref(desc), C.byref(h)), self._name + "_create failed: ", last_error)
        self.h = h

    def check(self, rc) -> None:
        if rc != 0:
            check(rc, self._name + ": ", getattr(self.lib, self._name + "_last_error"), self.h)

    def close(self) -> None:
        if self.h is not None:
            getattr(self.lib, self._name + "_destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
