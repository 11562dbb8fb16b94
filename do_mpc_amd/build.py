"""Compile the native pieces: the generic runtime (C ABI) and per-model gfx950 code objects.

Everything is built in-tree under do_mpc_amd/_build/ (git-ignored; travels to the GPU box with
the gpurun snapshot).  hipcc cross-compiles for gfx950 without a GPU.
"""
from __future__ import annotations

import contextlib
import fcntl
import hashlib
import os
import shutil
import subprocess
import tempfile
from typing import Optional

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
BUILD = os.path.join(HERE, "_build")
ARCH = "gfx950"


class BuildError(RuntimeError):
    pass


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise BuildError("hipcc not found: the dompc IPM backend needs the ROCm toolchain to lower models to gfx950")


def _run(cmd, what):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise BuildError(f"{what} failed:\n{' '.join(cmd)}\n{r.stdout}")
    return r.stdout


@contextlib.contextmanager
def _locked(directory: str, name: str = ".lock"):
    """Exclusive lock on a build directory: several rank processes lower the same MPC at the same time
    (MPC.shard_tree, torchrun) and must not compile into the same paths concurrently.  `name`: a lock of one output file of the
    directory instead - the code objects of one model (its variants and sets of switches) are compiled side by side."""
    os.makedirs(directory, exist_ok=True)
    fd = os.open(os.path.join(directory, name), os.O_CREAT | os.O_RDWR, 0o644)
    try:
        fcntl.flock(fd, fcntl.LOCK_EX)
        yield
    finally:
        fcntl.flock(fd, fcntl.LOCK_UN)
        os.close(fd)


def _write_atomic(path: str, text: str) -> None:
    """temp file in the same directory + rename: a reader never sees a truncated file"""
    fd, tmp = tempfile.mkstemp(dir=os.path.dirname(path), prefix=os.path.basename(path) + ".", suffix=".tmp")
    with os.fdopen(fd, "w") as f:
        f.write(text)
    os.replace(tmp, path)


def _fresh(out: str, stamp: str, dig: str) -> bool:
    try:
        return os.path.exists(out) and open(stamp).read() == dig
    except OSError:
        return False


def _compile_to(cmd_without_out, out: str, what: str) -> None:
    """run the compiler into a temporary name next to `out`, then rename into place"""
    tmp = f"{out}.{os.getpid()}.tmp"
    try:
        _run(cmd_without_out + ["-o", tmp], what)
        os.replace(tmp, out)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def _sources_digest() -> str:
    h = hashlib.sha256()
    for fn in sorted(os.listdir(CSRC)):                       # (every source of the kernels and of the runtime)
        if not fn.endswith((".h", ".hip", ".cpp")):
            continue
        h.update(fn.encode())
        with open(os.path.join(CSRC, fn), "rb") as f:
            h.update(f.read())
    with open(os.path.join(INCLUDE, "dompc_ipm.h"), "rb") as f:
        h.update(f.read())
    return h.hexdigest()[:12]


def runtime_library(force: bool = False) -> str:
    """libdompc_ipm.so - the C-ABI host runtime (HIP only; no CPU fallback inside)."""
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "libdompc_ipm.so")
    stamp = out + ".stamp"
    dig = _sources_digest()
    if not force and _fresh(out, stamp, dig):
        return out
    with _locked(BUILD):
        if not force and _fresh(out, stamp, dig):       # another process built it while we waited
            return out
        cmd = [_hipcc(), "-O2", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__",
               os.path.join(CSRC, "dompc_runtime.cpp"), os.path.join(CSRC, "dompc_plant_runtime.cpp"),
               os.path.join(CSRC, "dompc_ekf_runtime.cpp"), os.path.join(CSRC, "dompc_lqr_runtime.cpp"),
               os.path.join(CSRC, "dompc_ampc_runtime.cpp"), os.path.join(CSRC, "dompc_asmpc_runtime.cpp"), "-ldl"]
        _compile_to(cmd, out, "building libdompc_ipm.so")
        _write_atomic(stamp, dig)
    return out


def model_dir(model_hash: str) -> str:
    d = os.path.join(BUILD, "models", model_hash)
    os.makedirs(d, exist_ok=True)
    return d


def model_code_object(header_text: str, model_hash: str, force: bool = False, opt: str = "-O3", shard: bool = False, batch_only: bool = False,
                      defs: Optional[str] = None) -> str:
    """Per-model gfx950 code object (hsaco) from the generated header + the kernel sources.
    shard=True: the variant with tree-sharding support (ownership masks, cross-rank exchanges).
    batch_only=True: the sibling `..._batch.hsaco` compiled with -DDOMPC_NO_WIDE=1 -DDOMPC_BLOCK_CONST=64 - "one workgroup of ONE wavefront
    per problem" (the launch shape of batches >= 4096) is a compile-time fact there: no device-scope barrier / atomic flag code in the phases
    (+1.6 % on the headline batch in a same-box A/B), thread counts and strides constants, workgroup barriers folded (+1.0 % more); the
    runtime loads it next to the general object when it exists and launches it whenever the workgroups have 64 threads.
    defs: the extra switches of the build, in place of the environment's DOMPC_DEFS (build() compiles the objects of several sets of
    switches side by side: the environment is one per process)."""
    forced = os.environ.get("DOMPC_CODE_OBJECT")     # measurement aid: use this code object as it is (A/B against an older kernel)
    if forced and not shard:
        return forced
    assert not (shard and batch_only)
    d = model_dir(model_hash)
    hdr = os.path.join(d, "model_gen.h")
    out = os.path.join(d, f"dompc_{ARCH}{'_shard' if shard else ''}.hsaco")
    stamp = out + ".stamp"
    lb = os.environ.get("DOMPC_LB", "2")          # tuning aid: wavefronts per SIMD the kernel is compiled for
    prof = os.environ.get("DOMPC_PROFILE", "0")    # measurement aid: sub-phase cycle counters compiled in (tools/gpu_profile.py)
    defs = (os.environ.get("DOMPC_DEFS", "") if defs is None else defs).split()  # measurement aid: extra -D switches / compiler flags (entries starting with '-') for A/B builds (own file per set)
    if defs or prof != "0" or lb != "2":          # (measurement builds live next to the product build, under their own names)
        tag = ("prof" if prof != "0" else "") + (("lb" + lb) if lb != "2" else "") + (hashlib.sha256(" ".join(defs).encode()).hexdigest()[:8] if defs else "")
        out = out[:-len(".hsaco")] + "_" + tag + ".hsaco"
    if batch_only:
        out = out[:-len(".hsaco")] + "_batch.hsaco"      # (the name the runtime derives from the general object's path)
        defs = defs + ["DOMPC_NO_WIDE=1", "DOMPC_BLOCK_CONST=64"]
    stamp = out + ".stamp"
    # machine scheduler / register allocation of the solver kernels (round 5, same-box A/B on the headline batch, profiles/r05_flags.txt):
    # the iterative ILP strategy of the AMDGPU backend +3.0 % against the default strategy, region priorities in the greedy allocator
    # another +0.6 % (default 7 604 -> 7 828 / 7 853 -> 7 889 MPC steps/s; iterative-minreg -9 %, iterative-maxocc +2.5 %, post-RA scheduler
    # off -1.8 %; bitwise the same results: the flags reorder instructions, they do not change the arithmetic).  DOMPC_SCHED=default
    # builds without them; a DOMPC_DEFS set that names a strategy itself wins.
    sched = []
    if os.environ.get("DOMPC_SCHED", "iterative-ilp") != "default" and not any("amdgpu-sched-strategy" in d_ for d_ in defs):
        sched = ["-mllvm", "-amdgpu-sched-strategy=iterative-ilp"]
        if not any("greedy-regclass-priority" in d_ for d_ in defs):
            sched += ["-mllvm", "-greedy-regclass-priority-trumps-globalness=1"]
    dig = _sources_digest() + hashlib.sha256(header_text.encode()).hexdigest()[:12] + opt + ("S" if shard else "") + "lb" + lb + "p" + prof + " ".join(defs) + " ".join(sched)
    if not force and _fresh(out, stamp, dig):
        return out
    with _locked(d, os.path.basename(out) + ".lock"):
        if not force and _fresh(out, stamp, dig):       # another rank built it while we waited for the lock
            return out
        if not (os.path.exists(hdr) and open(hdr).read() == header_text):
            _write_atomic(hdr, header_text)
        # (the iterative scheduler of this ROCm's clang crashes - segmentation fault in the greedy register allocator - on some models, e.g. the
        #  discrete oscillating-masses class: such a model is compiled with the default strategy instead; `<out>.sched` says which one it got)
        last = None
        for fl in ([sched, []] if sched else [[]]):
            cmd = [_hipcc(), f"--offload-arch={ARCH}", opt, "-std=c++17", "--genco", f"-DDOMPC_SHARD={1 if shard else 0}", f"-DDOMPC_SRC_DIGEST=0x{_sources_digest()}ULL", *fl, f"-DDOMPC_LB={lb}", f"-DDOMPC_PROFILE={prof}", *[(d if d.startswith("-") else f"-D{d}") for d in defs],
                   f"-DDOMPC_MODEL_HEADER=\"{hdr}\"", "-I", CSRC, os.path.join(CSRC, "dompc_device.hip")]
            try:
                _compile_to(cmd, out, f"lowering model {model_hash} to {ARCH}")
                _write_atomic(out + ".sched", " ".join(fl) or "default")
                last = None
                break
            except BuildError as e:
                last = e
                if "Segmentation fault" not in str(e) and "frontend command failed" not in str(e):
                    raise
        if last is not None:
            raise last
        _write_atomic(stamp, dig)
    return out


def _kernel_code_object(prefix: str, source: str, header_macro: str, header_name: str, what: str, header_text: str, model_hash: str,
                        force: bool, remarks: bool = False):
    """gfx950 code object of csrc/`source` for one lowered model: `_build/models/<prefix>_<hash>/dompc_<prefix>_gfx950.hsaco`, the
    generated header next to it and named to the kernel by -D`header_macro`."""
    d = model_dir(prefix + "_" + model_hash)
    hdr = os.path.join(d, header_name)
    out = os.path.join(d, f"dompc_{prefix}_{ARCH}.hsaco")
    stamp = out + ".stamp"
    dig = _sources_digest() + hashlib.sha256(header_text.encode()).hexdigest()[:12]
    cmd = [_hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "--genco", f"-D{header_macro}=\"{hdr}\"", "-I", CSRC,
           os.path.join(CSRC, source)]
    if not force and not remarks and _fresh(out, stamp, dig):
        return out
    with _locked(d):
        if not force and not remarks and _fresh(out, stamp, dig):
            return out
        if not (os.path.exists(hdr) and open(hdr).read() == header_text):
            _write_atomic(hdr, header_text)
        if remarks:
            tmp = f"{out}.{os.getpid()}.remarks.tmp"
            try:
                text = _run(cmd + ["-Rpass-analysis=kernel-resource-usage", "-o", tmp], f"resource usage of {what} {model_hash}")
            finally:
                if os.path.exists(tmp):
                    os.remove(tmp)
            return out, text
        _compile_to(cmd, out, f"lowering {what} {model_hash} to {ARCH}")
        _write_atomic(stamp, dig)
    return out


def plant_code_object(header_text: str, model_hash: str, force: bool = False) -> str:
    """gfx950 code object of the batched plant integrator (csrc/dompc_plant.hip) for one lowered plant model."""
    return _kernel_code_object("plant", "dompc_plant.hip", "DOMPC_PLANT_HEADER", "plant_gen.h", "plant", header_text, model_hash, force)


def ekf_code_object(header_text: str, model_hash: str, force: bool = False, remarks: bool = False):
    """gfx950 code object of the batched extended Kalman filter (csrc/dompc_ekf.hip) for one lowered model.
    remarks=True: compile again with -Rpass-analysis=kernel-resource-usage and return (path, compiler output) - registers, scratch and
    LDS of the kernels (profiles/ekf_resource_usage.txt)."""
    return _kernel_code_object("ekf", "dompc_ekf.hip", "DOMPC_EKF_HEADER", "ekf_gen.h", "filter", header_text, model_hash, force, remarks)


def lqr_code_object(header_text: str, model_hash: str, force: bool = False, remarks: bool = False):
    """gfx950 code object of the batched LQR design (csrc/dompc_lqr.hip) for one lowered design (sizes, mode and - for gains_at - the
    model's Jacobians).  remarks=True: as ekf_code_object (profiles/lqr_resource_usage.txt)."""
    return _kernel_code_object("lqr", "dompc_lqr.hip", "DOMPC_LQR_HEADER", "lqr_gen.h", "LQR design", header_text, model_hash, force, remarks)


def ampc_code_object(header_text: str, model_hash: str, force: bool = False, remarks: bool = False):
    """gfx950 code object of the batched approximate-MPC step (csrc/dompc_ampc.hip) for one lowered network shape (sizes, activations,
    scaling; the weights are runtime data).  remarks=True: as ekf_code_object (profiles/ampc_resource_usage.txt)."""
    return _kernel_code_object("ampc", "dompc_ampc.hip", "DOMPC_AMPC_HEADER", "ampc_gen.h", "network", header_text, model_hash, force, remarks)


def ampc_loop_pair_hash(plant_hash: str, network_hash: str) -> str:
    """the hash of a (plant, network shape) pair: made of the two model hashes"""
    return f"{plant_hash}_{network_hash}"


def ampc_loop_code_object(plant_header: str, network_header: str, pair_hash: str, force: bool = False, remarks: bool = False):
    """gfx950 code object of the fused approximate-MPC loop (csrc/dompc_ampc_loop.hip) for one PAIR of a lowered plant model and a
    lowered network shape: the plant's kernels plus dompc_ampc_loop_kernel, two generated headers behind -DDOMPC_PLANT_HEADER and
    -DDOMPC_AMPC_HEADER (the weights are runtime data).  `pair_hash`: ampc_loop_pair_hash of the two model hashes.  Digest cache and
    lock as in _kernel_code_object.  remarks=True: as ekf_code_object (profiles/ampc_loop_resource_usage.txt)."""
    d = model_dir("ampc_loop_" + pair_hash)
    hdrs = [(os.path.join(d, "plant_gen.h"), plant_header), (os.path.join(d, "ampc_gen.h"), network_header)]
    out = os.path.join(d, f"dompc_ampc_loop_{ARCH}.hsaco")
    stamp = out + ".stamp"
    dig = _sources_digest() + hashlib.sha256((plant_header + "\0" + network_header).encode()).hexdigest()[:12]
    cmd = [_hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "--genco", f"-DDOMPC_PLANT_HEADER=\"{hdrs[0][0]}\"",
           f"-DDOMPC_AMPC_HEADER=\"{hdrs[1][0]}\"", "-I", CSRC, os.path.join(CSRC, "dompc_ampc_loop.hip")]
    if not force and not remarks and _fresh(out, stamp, dig):
        return out
    with _locked(d):
        if not force and not remarks and _fresh(out, stamp, dig):
            return out
        for hdr, text in hdrs:
            if not (os.path.exists(hdr) and open(hdr).read() == text):
                _write_atomic(hdr, text)
        if remarks:
            tmp = f"{out}.{os.getpid()}.remarks.tmp"
            try:
                text = _run(cmd + ["-Rpass-analysis=kernel-resource-usage", "-o", tmp], f"resource usage of the loop pair {pair_hash}")
            finally:
                if os.path.exists(tmp):
                    os.remove(tmp)
            return out, text
        _compile_to(cmd, out, f"lowering the loop pair {pair_hash} to {ARCH}")
        _write_atomic(stamp, dig)
    return out


def asmpc_code_object(header_text: str, model_hash: str, force: bool = False, remarks: bool = False):
    """gfx950 code object of the sensitivity-based MPC law (csrc/dompc_asmpc.hip: law preparation and law step) for one pair of sizes
    (n_x, n_u); no model in it, the law is runtime data.  remarks=True: as ekf_code_object (profiles/asmpc_resource_usage.txt)."""
    return _kernel_code_object("asmpc", "dompc_asmpc.hip", "DOMPC_ASMPC_HEADER", "asmpc_gen.h", "law", header_text, model_hash, force, remarks)
