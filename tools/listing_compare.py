#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 device code of two builds (no GPU needed):

    python tools/listing_compare.py OLD/csrc/build NEW/csrc/build [regular expression of the kernel names for the resource table]

For sart_kernels.o and sart_api.o of both build directories: the code object is taken out of the host object, disassembled, and cut
into kernels; an instruction is its mnemonic and operands (addresses, encodings and the numbers of branch labels left out).  Prints
which kernels are the same instruction for instruction, which differ (in how many lines, and by which mnemonics: new count minus
old count) and which exist on one side only, then the resource table (tools/kernel_resources.py) of the kernels the expression
selects, in the old build and in the new."""
import collections
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import LLVM, code_object_notes, demangle, kernels  # noqa: E402


def listing(obj_path: str) -> dict:
    """{kernel symbol: [instruction text]} of the code object inside a host object."""
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, os.path.basename(obj_path))
        shutil.copy(obj_path, obj)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", obj], check=True, capture_output=True, cwd=tmp)
        dev = [f for f in os.listdir(tmp) if "amdgcn" in f]
        if not dev:
            return {}
        text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", os.path.join(tmp, dev[0])],
                              capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = None if re.match(r"L\d+|\$", m.group(1)) else out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith("\t") and not line.startswith(" "):
            continue
        ins = line.split("//")[0].strip()
        ins = re.sub(r"^[0-9a-f]+:\s*", "", ins)
        ins = re.sub(r"<[^>]*>", "<label>", ins)                       # branch targets by name ...
        ins = re.sub(r"(s_c?branch\S*|s_call\S*)\s+\S+", r"\1 <label>", ins)   # ... or by offset
        if ins and ins != "...":   # ("...": the zero padding in front of the next kernel)
            cur.append(ins)
    return out


def main():
    old_dir, new_dir = sys.argv[1], sys.argv[2]
    pat = sys.argv[3] if len(sys.argv) > 3 else "_histogram_kernel"
    for o in ("sart_kernels.o", "sart_api.o"):
        old, new = listing(os.path.join(old_dir, o)), listing(os.path.join(new_dir, o))
        if not old and not new:
            print("%s: no device code in either build" % o)
            continue
        names = sorted(set(old) | set(new))
        nice = dict(zip(names, demangle(names)))
        same = [n for n in names if n in old and n in new and old[n] == new[n]]
        print("%s: %d kernels in the old build, %d in the new; %d the same instruction for instruction" % (o, len(old), len(new), len(same)))
        for n in names:
            if n in old and n in new and old[n] != new[n]:
                d = [l for l in difflib.unified_diff(old[n], new[n], lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
                print("  DIFFERS (%d lines of %d / %d): %s" % (len(d), len(old[n]), len(new[n]), nice[n]))
                h = collections.Counter(i.split()[0] for i in new[n])
                h.subtract(collections.Counter(i.split()[0] for i in old[n]))
                print("    mnemonics, new - old: %s" % (", ".join("%s %+d" % (m, k) for m, k in sorted(h.items()) if k) or "none"))
            elif n not in new:
                print("  ONLY OLD (%d instructions): %s" % (len(old[n]), nice[n]))
            elif n not in old:
                print("  ONLY NEW (%d instructions): %s" % (len(new[n]), nice[n]))
    for side, build_dir in (("old", old_dir), ("new", new_dir)):
        print()
        print("resources of the %s build's kernels matching %r:" % (side, pat))
        ks = kernels(code_object_notes(os.path.join(build_dir, "sart_kernels.o")))
        for k, nm in zip(ks, demangle([k["name"] for k in ks])):
            if re.search(pat, nm) and "trace_histogram_kernel" not in nm:
                print("  %-62s vgpr %3d sgpr %3d scratch %d lds %6d spills v%d s%d kernarg %d" % (
                    re.sub(r"\(.*", "", nm).replace("void sart::", ""), k["vgpr"], k["sgpr"], k["scratch"], k["lds"], k["vgpr_spill"],
                    k["sgpr_spill"], k["kernarg"]))


if __name__ == "__main__":
    main()
