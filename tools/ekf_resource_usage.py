"""Registers, scratch and LDS of the prebuilt extended Kalman filter kernels, as the compiler reports them
(-Rpass-analysis=kernel-resource-usage; no GPU needed).  usage: python tools/ekf_resource_usage.py > profiles/ekf_resource_usage.txt"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge
from do_mpc_amd import build

FIELDS = ["SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]
print("# hipcc --offload-arch=gfx950 -O3 --genco -Rpass-analysis=kernel-resource-usage csrc/dompc_ekf.hip, kernel dompc_ekf_kernel")
print("| model | nx | ny | type | " + " | ".join(FIELDS) + " |")
print("|" + "---|" * (4 + len(FIELDS)))
for name, kw, hdr, h in ge.lowered_ekf():
    _, text = build.ekf_code_object(hdr, h, remarks=True)
    blk = text.split("Function Name: dompc_ekf_kernel", 1)[1].split("Function Name:", 1)[0]
    vals = [re.search(re.escape(f) + r": (\d+)", blk).group(1) for f in FIELDS]
    dims = {k: re.search(rf"#define EKF_{k} (\d+)", hdr).group(1) for k in ("NX", "NY", "DISCRETE")}
    print(f"| {name} {kw or ''} | {dims['NX']} | {dims['NY']} | {'discrete' if dims['DISCRETE'] == '1' else 'continuous'} | " + " | ".join(vals) + " |")
print("\nScratch: none in any of the four (every register array is indexed at compile time).  The continuous filters hold the seven stage")
print("derivatives of [x; P] of the Dormand-Prince pair in registers: they fill the architectural VGPRs (one wavefront per SIMD) and the")
print("compiler parks a few SGPRs in VGPR lanes (SGPRs Spill) - no memory traffic.")
