"""Registers, scratch and LDS of the prebuilt approximate-MPC network kernels - the step (dompc_ampc_kernel) and the Jacobian
(dompc_ampc_jac_kernel) of the same code object -, as the compiler reports them (-Rpass-analysis=kernel-resource-usage; no GPU needed).
usage: python tools/ampc_resource_usage.py > profiles/ampc_resource_usage.txt"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge
from do_mpc_amd import build

KERNELS = ["dompc_ampc_kernel", "dompc_ampc_jac_kernel"]
FIELDS = ["SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]
print("# hipcc --offload-arch=gfx950 -O3 --genco -Rpass-analysis=kernel-resource-usage csrc/dompc_ampc.hip, kernels " + " and ".join(KERNELS))
print("| network (n_in -> hidden layers x neurons, activation -> n_out, output activation) | kernel | v_mfma_f32_32x32x2_f32 in the text | " + " | ".join(FIELDS) + " |")
print("|" + "---|" * (3 + len(FIELDS)))
clean = True
for label, hdr, h in ge.lowered_ampc():
    out, text = build.ampc_code_object(hdr, h, remarks=True)
    asm = build._run([build._hipcc(), f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "--cuda-device-only", "-S", f"-DDOMPC_AMPC_HEADER=\"{os.path.join(os.path.dirname(out), 'ampc_gen.h')}\"",
                      "-I", build.CSRC, os.path.join(build.CSRC, "dompc_ampc.hip"), "-o", "-"], "assembly of the network kernels")
    for kernel in KERNELS:
        blk = text.split(f"Function Name: {kernel}", 1)[1].split("Function Name:", 1)[0]
        vals = [re.search(re.escape(f) + r": (\d+)", blk).group(1) for f in FIELDS]
        body = asm.split(f"\n{kernel}:", 1)[1].split("s_endpgm", 1)[0]
        n_mfma = sum(1 for line in body.splitlines() if line.strip().startswith("v_mfma_f32_32x32x2_f32"))
        clean = clean and all(vals[FIELDS.index(f)] == "0" for f in ("ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"))
        print(f"| {label} | {kernel} | {n_mfma} | " + " | ".join(vals) + " |")
print("\nScratch, spills and LDS: " + ("none in any of them" if clean else "NOT ZERO in at least one row above") + " (every tile register is indexed at compile time; the")
print("activations of one layer are the operand of the next in place).  The step's widest shape holds two activations of four 32-row")
print("tiles, 2 x 64 registers, plus the operand and the addresses, and still runs two wavefronts per SIMD (the accumulator tiles live in")
print("AGPRs).  The Jacobian kernel carries a primal and one tangent per input direction; a layer's primal pass runs first and its tangent")
print("pass behind it, so three sets of tiles are live at most (3 x 64 registers at the widest shape, one wavefront per SIMD there), and")
print("the loads that are the same in every direction are kept inside the direction loop.  The matrix instruction count is the unrolled")
print("text of one kernel (first layer, ONE hidden-to-hidden layer as a rolled loop, output layer; the Jacobian's loop over the input")
print("directions is rolled too), steps over padding skipped.")
