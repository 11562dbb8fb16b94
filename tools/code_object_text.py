"""Instruction text of the gfx950 code objects of two builds, symbol by symbol - the check that a refactor of the kernel sources left
every instruction stream as it was.  Needs no GPU.

    python tools/code_object_text.py compare DIR_A DIR_B [--allow SYMBOL ...]

DIR_A, DIR_B: two do_mpc_amd/_build/models trees (the directory names are model hashes from the Python lowering, so two builds of the
same classes have the same names).  Every .hsaco present at the same relative path in both is unbundled (clang-offload-bundler),
disassembled (llvm-objdump -d) and split by function symbol; the instruction text of each symbol - mnemonics and operands, without
addresses and encodings - is compared.  Whole files are not: the ELF differs outside .text from build to build.  The symbols that
differ are printed with the number of objects compared; the exit status is non-zero on any difference in a symbol not named with
--allow (the solver's info kernel carries the digest of the sources as a literal)."""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _tool(name):
    for cand in (shutil.which(name), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", name)):
        if cand and os.path.exists(cand):
            return cand
    sys.exit(f"{name} not found (ROCm's llvm/bin)")


def symbols(hsaco, tmp):
    """{function symbol: sha256 of its instruction text} of the gfx950 part of `hsaco`"""
    elf = os.path.join(tmp, "part.elf")
    subprocess.run([_tool("clang-offload-bundler"), "--type=o", f"--targets={TARGET}", "--unbundle", f"--input={hsaco}", f"--output={elf}"],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = subprocess.run([_tool("llvm-objdump"), "-d", elf], check=True, stdout=subprocess.PIPE, text=True).stdout
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = hashlib.sha256()
        elif name is not None and line.strip():
            out[name].update((" ".join(line.split("//")[0].split()) + "\n").encode())
    return {k: h.hexdigest() for k, h in out.items()}


def code_objects(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs if f.endswith(".hsaco"))


def compare(dir_a, dir_b, allow):
    a, b = code_objects(dir_a), code_objects(dir_b)
    common = [p for p in a if p in set(b)]
    for p in sorted(set(a) ^ set(b)):
        print(f"only in {'A' if p in a else 'B'}: {p}")
    n_sym, differing, allowed = 0, 0, 0
    with tempfile.TemporaryDirectory() as tmp:
        for p in common:
            sa, sb = symbols(os.path.join(dir_a, p), tmp), symbols(os.path.join(dir_b, p), tmp)
            n_sym += len(set(sa) | set(sb))
            for s in sorted(set(sa) | set(sb)):
                if sa.get(s) != sb.get(s):
                    what = "differs" if s in sa and s in sb else ("only in A" if s in sa else "only in B")
                    ok = s in allow
                    allowed += ok
                    differing += not ok
                    print(f"{'allowed  ' if ok else 'DIFFERENT'} {p}: {s} ({what})")
    print(f"{len(common)} code objects at the same path in both trees compared ({len(a)} in A, {len(b)} in B), {n_sym} symbols; "
          f"{differing} differing symbols, {allowed} more allowed by name ({', '.join(sorted(allow)) or 'none'})")
    return 1 if differing or not common else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    allow = set()
    while "--allow" in args:
        i = args.index("--allow")
        if i + 1 >= len(args):
            sys.exit(__doc__)
        allow.add(args[i + 1])
        del args[i:i + 2]
    if len(args) == 3 and args[0] == "compare":
        sys.exit(compare(args[1], args[2], allow))
    sys.exit(__doc__)
