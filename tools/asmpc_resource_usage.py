"""Registers, scratch and LDS of the entries of the sensitivity-based MPC loop, as the compiler reports them
(-Rpass-analysis=kernel-resource-usage; no GPU needed): the law preparation and the law step of csrc/dompc_asmpc.hip for every prebuilt
shape - the last one, n_x = 64 and n_u = 16, is the limit -, the two launches of the selection (they read no size: listed once) and the
plant rollout of csrc/dompc_plant.hip next to the plant step it
contains, for the plants the loop is tested and measured on.  usage: python tools/asmpc_resource_usage.py > profiles/asmpc_resource_usage.txt"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge
from do_mpc_amd import build
from do_mpc_amd.examples import CASES
from do_mpc_amd.simulator import Simulator

FIELDS = ["SGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]


def row(text, kernel):
    blk = text.split("Function Name: " + kernel + " ", 1)[1].split("Function Name:", 1)[0]
    return [re.search(re.escape(f) + r": (\d+)", blk).group(1) for f in FIELDS]


print("# hipcc --offload-arch=gfx950 -O3 --genco -Rpass-analysis=kernel-resource-usage csrc/dompc_asmpc.hip and csrc/dompc_plant.hip")
print("| object | kernel | " + " | ".join(FIELDS) + " |")
print("|" + "---|" * (2 + len(FIELDS)))
for label, hdr, h in ge.lowered_asmpc():
    _, text = build.asmpc_code_object(hdr, h, remarks=True)
    for kernel in ("dompc_asmpc_prepare_kernel", "dompc_asmpc_step_kernel"):
        print(f"| law, {label} | {kernel} | " + " | ".join(row(text, kernel)) + " |")
for kernel in ("dompc_asmpc_select_count_kernel", "dompc_asmpc_select_write_kernel"):
    print(f"| law, any shape | {kernel} | " + " | ".join(row(text, kernel)) + " |")
for name in ("batch_reactor", "CSTR", "industrial_poly"):
    hdr = Simulator(CASES[name].build_model())._lower()
    h = hdr.rsplit('PLANT_MODEL_HASH "', 1)[1].split('"')[0]
    _, text = build._kernel_code_object("plant", "dompc_plant.hip", "DOMPC_PLANT_HEADER", "plant_gen.h", "plant", hdr, h, False, remarks=True)
    for kernel in ("dompc_plant_kernel", "dompc_plant_rollout_kernel"):
        print(f"| plant {name} | {kernel} | " + " | ".join(row(text, kernel)) + " |")
