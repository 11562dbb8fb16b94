"""Registers, scratch and occupancy of the fused approximate-MPC loop kernel (csrc/dompc_ampc_loop.hip: dompc_ampc_loop_kernel) of the
prebuilt pairs, next to the plant step (dompc_plant_kernel, from the same pair object) and the network step (dompc_ampc_kernel, from the
network's own object) it is made of, as the compiler reports them (-Rpass-analysis=kernel-resource-usage) - and a disassembly diff of
every prebuilt plant and network object against the sources of a parent commit: their kernels must keep their instruction text.
No GPU needed.
usage: python tools/ampc_loop_resource_usage.py [--parent HEAD~1] > profiles/ampc_loop_resource_usage.txt"""
import argparse
import contextlib
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge
from do_mpc_amd import build
from do_mpc_amd.examples import CASES
from do_mpc_amd.simulator import Simulator

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default="HEAD~1", help="the commit whose csrc/ the plant and network kernels are compared with")
args = ap.parse_args()

FIELDS = ["SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]


def usage(text, kernel):
    blk = text.split(f"Function Name: {kernel}", 1)[1].split("Function Name:", 1)[0]
    return [re.search(re.escape(f) + r": (\d+)", blk).group(1) for f in FIELDS]


print("# hipcc --offload-arch=gfx950 -O3 --genco -Rpass-analysis=kernel-resource-usage: csrc/dompc_ampc_loop.hip per (plant, network shape) pair,")
print("# dompc_plant_kernel of the same object and dompc_ampc_kernel of the network's own object beside it")
print("| pair | kernel | " + " | ".join(FIELDS) + " |")
print("|" + "---|" * (2 + len(FIELDS)))
worse = []
for label, ph, nh, p_hash, n_hash in ge.lowered_ampc_loop():
    _, text = build.ampc_loop_code_object(ph, nh, build.ampc_loop_pair_hash(p_hash, n_hash), remarks=True)
    _, net = build.ampc_code_object(nh, n_hash, remarks=True)
    loop, plant, netw = usage(text, "dompc_ampc_loop_kernel"), usage(text, "dompc_plant_kernel"), usage(net, "dompc_ampc_kernel")
    for kernel, vals in (("dompc_ampc_loop_kernel", loop), ("dompc_plant_kernel", plant), ("dompc_ampc_kernel", netw)):
        print(f"| {label} | {kernel} | " + " | ".join(vals) + " |")
    i = FIELDS.index("ScratchSize [bytes/lane]")
    if int(loop[i]) > max(int(plant[i]), int(netw[i])):
        worse.append(label)
print("\nScratch of the loop kernel beyond that of the plant step and the network step of its pair: " + (", ".join(worse) if worse else "in no pair") + ".")
print("The loop kernel's scratch is the integrator's (its per-thread arrays are indexed at run time); the network step adds none: the weight")
print("and bound loads are kept inside the loop over the two groups of 32 samples (dompc_ampck::reloaded), hoisted out of it and out of the")
print("loop over the control steps they sat in registers beside the integrator's and spilled (widest pair: 256 VGPRs + 256 AGPRs, 464 bytes).")

# ---------------------------------------------------------------------------------------------- the parent's instruction text
tmp = tempfile.mkdtemp(prefix="dompc_parent_")
tar = subprocess.run(["git", "-C", ROOT, "archive", args.parent, "do_mpc_amd/csrc"], stdout=subprocess.PIPE, check=True).stdout
tarfile.open(fileobj=io.BytesIO(tar)).extractall(tmp)
parent_csrc = os.path.join(tmp, "do_mpc_amd", "csrc")


def text_of(csrc, source, macro, header_text):
    """the instruction text of a kernel file: its assembly without comments, file names, the compiler's identification and the
    compilation unit's id (__hip_cuid_<hash of the source's path>)"""
    hdr = os.path.join(tmp, "gen.h")
    with open(hdr, "w") as f:
        f.write(header_text)
    asm = build._run([build._hipcc(), f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "--cuda-device-only", "-S", f"-D{macro}=\"{hdr}\"", "-I", csrc,
                      os.path.join(csrc, source), "-o", "-"], f"assembly of {source}")
    keep = []
    for line in re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", asm).splitlines():
        line = line.split(";", 1)[0].rstrip()
        if line and not line.lstrip().startswith((".file", ".ident", ".amdgcn_target", ".loc")):
            keep.append(line)
    return "\n".join(keep)


objects = []
with contextlib.redirect_stdout(sys.stderr):               # (an example's model builder may print)
    for name in ge.PREBUILT_PLANTS:
        case, _, builder = name.partition(":")
        objects.append((f"plant {name}", "dompc_plant.hip", "DOMPC_PLANT_HEADER", Simulator(getattr(CASES[case], builder or "build_model")())._lower()))
    objects += [(f"plant of the probe family '{kind}'", "dompc_plant.hip", "DOMPC_PLANT_HEADER", hdr) for kind, hdr, _ in ge.lowered_plant_family()]
    objects += [(f"network {label}", "dompc_ampc.hip", "DOMPC_AMPC_HEADER", hdr) for label, hdr, _ in ge.lowered_ampc()]
rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", args.parent], stdout=subprocess.PIPE, text=True, check=True).stdout.strip()
print(f"\n# the kernels of the prebuilt plant and network objects against the sources of the parent commit {rev}: assembly (-S) of the same")
print("# generated header with either csrc/; comments, file names, the compiler's identification and the compilation unit's id dropped")
print("| object | lines of instruction text | differs from the parent |")
print("|---|---|---|")
changed = []
for label, source, macro, hdr in objects:
    new, old = text_of(build.CSRC, source, macro, hdr), text_of(parent_csrc, source, macro, hdr)
    if new != old:
        changed.append(label)
    print(f"| {label} | {len(new.splitlines())} | {'YES' if new != old else 'no'} |")
print("\nInstruction text that differs from the parent's: " + (", ".join(changed) if changed else "none - every kernel of every prebuilt plant and network object is the parent's, instruction for instruction") + ".")
