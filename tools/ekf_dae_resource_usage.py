"""Registers, scratch and LDS of the prebuilt extended Kalman filter kernels for models with algebraic states
(__graft_entry__.PREBUILT_EKF_DAE), as the compiler reports them (-Rpass-analysis=kernel-resource-usage; no GPU needed).
usage: python tools/ekf_dae_resource_usage.py > profiles/ekf_dae_resource_usage.txt"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge
from do_mpc_amd import build

FIELDS = ["SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]
print("# hipcc --offload-arch=gfx950 -O3 --genco -Rpass-analysis=kernel-resource-usage csrc/dompc_ekf.hip, kernel dompc_ekf_kernel,")
print("# headers of lowering.lower_ekf(..., dae_reduction=True) for the models of tests/ekf_dae_common.py")
print("| model | nx | nz | ny | type | " + " | ".join(FIELDS) + " |")
print("|" + "---|" * (5 + len(FIELDS)))
for name, hdr, h in ge.lowered_ekf_dae():
    _, text = build.ekf_code_object(hdr, h, remarks=True)
    blk = text.split("Function Name: dompc_ekf_kernel", 1)[1].split("Function Name:", 1)[0]
    vals = [re.search(re.escape(f) + r": (\d+)", blk).group(1) for f in FIELDS]
    dims = {k: (re.search(rf"#define EKF_{k} (\d+)", hdr) or [None, "0"])[1] for k in ("NX", "NZ", "NY", "DISCRETE")}
    print(f"| {name} | {dims['NX']} | {dims['NZ']} | {dims['NY']} | {'discrete' if dims['DISCRETE'] == '1' else 'continuous'} | " + " | ".join(vals) + " |")
print("\nThe discrete filters of the shipped sizes (masses, oscillating_masses_dae) are asserted free of scratch and spills by")
print("tests/test_gpu_ekf_dae.py; the continuous filters and the n_x = n_z = n_y = 16 one are recorded here only.  nz = 0: models 1 and 5")
print("with z eliminated by hand, ODE filters the others are compared with.")
