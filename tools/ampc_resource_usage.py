"""Registers, scratch and LDS of the prebuilt approximate-MPC network kernels, as the compiler reports them
(-Rpass-analysis=kernel-resource-usage; no GPU needed).  usage: python tools/ampc_resource_usage.py > profiles/ampc_resource_usage.txt"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge
from do_mpc_amd import build

FIELDS = ["SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]
print("# hipcc --offload-arch=gfx950 -O3 --genco -Rpass-analysis=kernel-resource-usage csrc/dompc_ampc.hip, kernel dompc_ampc_kernel")
print("| network (n_in -> hidden layers x neurons, activation -> n_out, output activation) | v_mfma_f32_32x32x2_f32 in the text | " + " | ".join(FIELDS) + " |")
print("|" + "---|" * (2 + len(FIELDS)))
for label, hdr, h in ge.lowered_ampc():
    out, text = build.ampc_code_object(hdr, h, remarks=True)
    blk = text.split("Function Name: dompc_ampc_kernel", 1)[1].split("Function Name:", 1)[0]
    vals = [re.search(re.escape(f) + r": (\d+)", blk).group(1) for f in FIELDS]
    asm = build._run([build._hipcc(), f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "--cuda-device-only", "-S", f"-DDOMPC_AMPC_HEADER=\"{os.path.join(os.path.dirname(out), 'ampc_gen.h')}\"",
                      "-I", build.CSRC, os.path.join(build.CSRC, "dompc_ampc.hip"), "-o", "-"], "assembly of the network kernel")
    n_mfma = sum(1 for line in asm.splitlines() if line.strip().startswith("v_mfma_f32_32x32x2_f32"))
    print(f"| {label} | {n_mfma} | " + " | ".join(vals) + " |")
print("\nScratch and LDS: none in any of them (every tile register is indexed at compile time; the activations of one layer are the operand")
print("of the next in place).  The widest shape holds two activations of four 32-row tiles, 2 x 64 registers, plus the operand and the")
print("addresses, and still runs two wavefronts per SIMD (the accumulator tiles live in AGPRs).  The matrix instruction count is the")
print("unrolled text (first layer, ONE hidden-to-hidden layer as a rolled loop, output layer), steps over padding skipped.")
