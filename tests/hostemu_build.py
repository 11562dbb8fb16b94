"""TEST-ONLY builders of the host emulation: the kernel sources compiled by g++ with -DDOMPC_HOST_EMU (one "workgroup" = one host
thread) into tests/_hostemu/.  They lived in do_mpc_amd/build.py until round 4 although only tests call them: the product
package now holds nothing that can run the solver without a GPU."""
import hashlib
import os
import shutil

from do_mpc_amd.build import CSRC, _compile_to, _fresh, _locked, _sources_digest, _write_atomic

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_hostemu")


def _hostemu(name, runtime, kernel, header_macro, header_name, extra, what, header_text, model_hash, out_dir, force):
    """`out_dir`/lib<name>_<hash>[_<tag of DOMPC_DEFS>].so from csrc/`runtime` and csrc/`kernel` (compiled as C++), the generated header
    next to it.  DOMPC_DEFS: extra -D switches (e.g. DOMPC_KAPPA_D=1e-5) or, starting with '-', compiler flags (tools/asan_hostemu.sh:
    -fsanitize=address) - an own library per set."""
    os.makedirs(out_dir, exist_ok=True)
    hdr = os.path.join(out_dir, f"{header_name}_{model_hash}.h")
    defs = os.environ.get("DOMPC_DEFS", "").split()
    tag = ("_" + hashlib.sha256(" ".join(defs).encode()).hexdigest()[:8]) if defs else ""
    out = os.path.join(out_dir, f"lib{name}_{model_hash}{tag}.so")
    stamp = out + ".stamp"
    dig = _sources_digest() + hashlib.sha256(header_text.encode()).hexdigest()[:12] + " ".join(defs)
    if not force and _fresh(out, stamp, dig):
        return out
    with _locked(out_dir):                                # (world_size-2 gloo tests build from two processes)
        if not force and _fresh(out, stamp, dig):
            return out
        if not (os.path.exists(hdr) and open(hdr).read() == header_text):
            _write_atomic(hdr, header_text)
        cxx = shutil.which("g++") or "g++"
        cmd = [cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-DDOMPC_HOST_EMU", *extra,
               *[(d if d.startswith("-") else f"-D{d}") for d in defs],
               f"-D{header_macro}=\"{hdr}\"", "-I", CSRC,
               os.path.join(CSRC, runtime), "-x", "c++", os.path.join(CSRC, kernel), "-lm"]
        _compile_to(cmd, out, f"building {what}host emulation")
        _write_atomic(stamp, dig)
    return out


def hostemu_library(header_text: str, model_hash: str, out_dir: str, force: bool = False) -> str:
    """TEST-ONLY: runtime + kernels compiled for the host (g++), one workgroup = one thread.
    Lives outside the package build dir (tests/_hostemu) and is never loaded by the product."""
    return _hostemu("dompc_hostemu", "dompc_runtime.cpp", "dompc_device.hip", "DOMPC_MODEL_HEADER", "model_gen", ["-DDOMPC_SHARD=1"], "",
                    header_text, model_hash, out_dir, force)


def plant_hostemu_library(header_text: str, model_hash: str, out_dir: str, force: bool = False) -> str:
    """TEST-ONLY: plant integrator compiled for the host (g++); lives in tests/_hostemu, never loaded by the product."""
    return _hostemu("dompc_plant_hostemu", "dompc_plant_runtime.cpp", "dompc_plant.hip", "DOMPC_PLANT_HEADER", "plant_gen", [], "plant ",
                    header_text, model_hash, out_dir, force)


def ekf_hostemu_library(header_text: str, model_hash: str, out_dir: str = OUT, force: bool = False) -> str:
    """TEST-ONLY: filter kernel + runtime compiled for the host (g++); lives in tests/_hostemu, never loaded by the product."""
    return _hostemu("dompc_ekf_hostemu", "dompc_ekf_runtime.cpp", "dompc_ekf.hip", "DOMPC_EKF_HEADER", "ekf_gen", [], "filter ",
                    header_text, model_hash, out_dir, force)


def lqr_hostemu_library(header_text: str, model_hash: str, out_dir: str = OUT, force: bool = False) -> str:
    """TEST-ONLY: design kernel + runtime compiled for the host (g++); lives in tests/_hostemu, never loaded by the product."""
    return _hostemu("dompc_lqr_hostemu", "dompc_lqr_runtime.cpp", "dompc_lqr.hip", "DOMPC_LQR_HEADER", "lqr_gen", [], "LQR design ",
                    header_text, model_hash, out_dir, force)
