"""Registers, scratch and LDS of the prebuilt LQR design kernels, as the compiler reports them
(-Rpass-analysis=kernel-resource-usage; no GPU needed).  usage: python tools/lqr_resource_usage.py > profiles/lqr_resource_usage.txt"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge
from do_mpc_amd import build

FIELDS = ["SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]
print("# hipcc --offload-arch=gfx950 -O3 --genco -Rpass-analysis=kernel-resource-usage csrc/dompc_lqr.hip, kernel dompc_lqr_kernel")
print("| design | nx | nu | N | model | " + " | ".join(FIELDS) + " |")
print("|" + "---|" * (5 + len(FIELDS)))
for label, hdr, h in ge.lowered_lqr():
    _, text = build.lqr_code_object(hdr, h, remarks=True)
    blk = text.split("Function Name: dompc_lqr_kernel", 1)[1].split("Function Name:", 1)[0]
    vals = [re.search(re.escape(f) + r": (\d+)", blk).group(1) for f in FIELDS]
    dims = {k: re.search(rf"#define LQR_{k} (\d+)", hdr).group(1) for k in ("NX", "NU", "N", "HAS_MODEL", "DISCRETE")}
    model = "none" if dims["HAS_MODEL"] == "0" else ("discrete" if dims["DISCRETE"] == "1" else "continuous (zero-order hold)")
    print(f"| {label} | {dims['NX']} | {dims['NU']} | {dims['N']} | {model} | " + " | ".join(vals) + " |")
print("\nScratch: none in any of them (every register array is indexed at compile time).  At N = 16 the doubling step holds A_k, G_k, H_k,")
print("I + G H and its two right-hand sides, 32 registers each: the architectural VGPRs are full and the allocator keeps further live")
print("values in AGPRs (one wavefront per SIMD either way: __launch_bounds__(64)) - register copies, no memory traffic, no spill counted.")
