"""Where two builds of one code object differ, symbol by symbol, with the pc-relative literals masked.

    python tools/kernel_text_diff.py A.hsaco B.hsaco [--regions SYMBOL]

tools/code_object_text.py answers "same instruction text or not".  Adding a kernel to a code object moves the constant tables, and every
`s_add_u32 / s_addc_u32 sN, sN, <literal>` that forms a pc-relative address changes its literal although no instruction changed: this
tool masks those literals, prints the instruction count of every symbol of A in both objects with the number of lines that still
differ, the register / scratch / LDS figures of the kernels from the code-object notes, and for --regions SYMBOL the line ranges of
that symbol that differ.  Needs no GPU (clang-offload-bundler, llvm-objdump, llvm-readelf of ROCm)."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def unbundle(hsaco, tmp, tag):
    elf = os.path.join(tmp, tag + ".elf")
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", f"--targets={TARGET}", "--unbundle", f"--input={hsaco}",
                    f"--output={elf}"], check=True)
    return elf


def symbols(elf):
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", elf], check=True, stdout=subprocess.PIPE, text=True).stdout
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name and line.strip():
            out[name].append(re.sub(r"^(s_addc?_u32 s\d+, s\d+, )0x[0-9a-f]+$", r"\1<pcrel>", " ".join(line.split("//")[0].split())))
    return out


def resources(elf):
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", elf], check=True, stdout=subprocess.PIPE, text=True).stdout
    out, cur = {}, {}
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(agpr_count|vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size|name):\s+(\S+)", line)
        if m:
            if m.group(1) == "agpr_count" and cur:
                out[cur.get("name")] = cur
                cur = {}
            cur[m.group(1)] = m.group(2)
    if cur:
        out[cur.get("name")] = cur
    return out


def main(argv):
    a_path, b_path = argv[0], argv[1]
    region = argv[argv.index("--regions") + 1] if "--regions" in argv else None
    with tempfile.TemporaryDirectory() as tmp:
        ea, eb = unbundle(a_path, tmp, "a"), unbundle(b_path, tmp, "b")
        sa, sb, ra, rb = symbols(ea), symbols(eb), resources(ea), resources(eb)
    for s in sorted(set(sa) | set(sb)):
        a, b = sa.get(s), sb.get(s)
        if a is None or b is None:
            print(f"{s}: only in {'B' if a is None else 'A'} ({len(b if a is None else a)} instructions)")
            continue
        nd = 0 if a == b else sum(1 for x in difflib.ndiff(a, b) if x[0] in "+-")
        print(f"{s}: {len(a)} -> {len(b)} instructions, {'same' if nd == 0 else str(nd) + ' lines differ'} after masking pc-relative literals")
    for k in sorted(set(ra) | set(rb)):
        f = lambda r: "-" if r is None else "vgpr %s agpr %s sgpr %s scratch %s lds %s" % tuple(r.get(x, "?") for x in (      # noqa: E731
            "vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size"))
        print(f"resources {k}: A {f(ra.get(k))} | B {f(rb.get(k))}")
    if region:
        sm = difflib.SequenceMatcher(None, sa[region], sb[region], autojunk=False)
        for tag, i1, i2, j1, j2 in sm.get_opcodes():
            if tag != "equal":
                print(f"{region}: {tag} A lines {i1}-{i2} ({i2 - i1}), B lines {j1}-{j2} ({j2 - j1})")


if __name__ == "__main__":
    main(sys.argv[1:])
