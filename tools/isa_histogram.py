#!/usr/bin/env python3
"""Instruction histogram of a trace kernel from the compiler's own listing (no GPU needed):

  python tools/isa_histogram.py [--variant 5] [--fixed] [--salu] [--json profiles/r03_isa_histogram.json] [--pmc profiles/<..>_pmc_summary.json]

Compiles csrc/sart_kernels.hip with -save-temps into csrc/build/asm/ (same flags as the Makefile), cuts the chosen
instantiation of trace_histogram_kernel out of the gfx950 assembly and counts its instructions per pipeline stage and class.

Stages: the kernel source carries assembly comments `; SART_STAGE <name>` at the head of every stage region (prologue, A0,
A1 = phase A, B = phase B, ACC = accumulation, epilogue); a basic block belongs to the stage of the last marker before it in
program order.  Blocks that carry a `; rare:` comment are the divergent alternatives that a wave skips with s_cbranch_execz
when no lane needs them (bore-wall entry, normal facing the ray, wide energy bucket ...): they are listed separately and not
counted as executed.

Classes of vector instructions (the question of VERDICT r02 #6: what are the "other" 137 per 64 rays?):
  f64      v_fma/fmac/mul/add/rcp/rsq/sqrt/rndne/trunc/floor/ldexp/frexp/div_*_f64, v_cvt involving f64 is `cvt`
  int      v_mad_u64_u32, v_mul_*, v_add/sub_(co_)u32, v_addc/subb, v_lshl/lshr/ashr*, v_and/or/xor/not/bfe/bfi/alignbit/perm, v_min/max_[iu]32,
           v_mbcnt, v_lshl_add, v_add3, v_mad_u32_u24 ...
  cmp      v_cmp_* / v_cmpx_*       (predicates -> lane masks)
  select   v_cndmask_b32            (predication residue: two per f64 value selected)
  mov      v_mov_b32 / v_mov_b64 / v_accvgpr_* (copies, literal materialisation)
  cvt      v_cvt_*
  lane     v_readlane / v_readfirstlane / v_writelane / v_permlane / dpp moves (cross-lane, SGPR spills)
  other    anything else that starts with v_
Phase A is inlined at two call sites (behind stage A0, or on its own when the setup has no zones): the listing shows A1 twice,
a launch executes one copy, and the model below divides A1 by the number of copies.
Per 64 launched rays a stage executes `passes` times (A0: 1; A1: the share of rays that survive stage A0, + the drain
passes; B: N_SHELL_SELECTED / N_RAYS).  With --pmc the model  sum_stage static(stage) x passes(stage)  is compared with
the measured SQ_INSTS_VALU x 64 / rays; passes(A1) is solved from the measured total when it is not given."""
import argparse
import collections
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "solaraxionraytracing_amd", "csrc")
VARIANTS = {0: "Lb1ELb0ELi0ELb0E", 1: "Lb0ELb0ELin1ELb0E", 2: "Lb0ELb1ELin1ELb0E", 3: "Lb1ELb0ELi1ELb0E", 4: "Lb1ELb1ELi0ELb0E",
            5: "Lb1ELb0ELi0ELb1E", 6: "Lb1ELb0ELi1ELb1E"}
FOLDED = {7: "Li0E", 8: "Li1E"}   # folded_histogram_kernel<1024, GAS, FIXED>: variants 5 / 6 with their wave-uniform switches folded

F64 = re.compile(r"v_(fma|fmac|mul|add|rcp|rsq|sqrt|rndne|trunc|floor|ceil|fract|ldexp|frexp_mant|frexp_exp_i32|div_scale|div_fmas|div_fixup|min|max)_f64")
CMP = re.compile(r"v_cmpx?_")
LANE = re.compile(r"v_(readlane|readfirstlane|writelane|permlane|mov_b32_dpp|bpermute)|_dpp\b|ds_(b)?permute")
INT = re.compile(r"v_(mad_u64_u32|mad_i64_i32|mul_lo_u32|mul_hi_u32|mul_u32_u24|mul_i32_i24|mad_u32_u24|mad_i32_i24|add_co_u32|addc_co_u32|sub_co_u32|subb_co_u32|"
                 r"subrev_co_u32|subbrev_co_u32|add_u32|sub_u32|subrev_u32|add_nc_u32|lshlrev_b32|lshrrev_b32|ashrrev_i32|lshlrev_b64|lshrrev_b64|"
                 r"ashrrev_i64|and_b32|or_b32|xor_b32|not_b32|bfe_u32|bfe_i32|bfi_b32|alignbit_b32|perm_b32|min_u32|max_u32|min_i32|max_i32|"
                 r"mbcnt_lo_u32_b32|mbcnt_hi_u32_b32|lshl_add_u32|add_lshl_u32|lshl_or_b32|and_or_b32|or3_b32|add3_u32|xad_u32|bcnt_u32_b32|"
                 r"lshl_add_u64|add_i32|sub_i32|med3_i32|med3_u32|xnor_b32|ffbh_u32|ffbl_b32|bitop3_b32|bitop3_b16)")


def classify(mn: str) -> str:
    if not mn.startswith("v_"):
        if mn.startswith("s_waitcnt"):
            return "s_waitcnt"
        if mn.startswith("s_"):
            return "salu"
        if mn.startswith(("global_atomic", "flat_atomic", "buffer_atomic")):
            return "vmem_atomic"
        if mn.startswith(("global_", "flat_", "buffer_", "scratch_")):
            return "vmem"
        if mn.startswith("ds_"):
            return "lds"
        return "misc"
    if LANE.search(mn):
        return "lane"
    if mn.startswith("v_cndmask"):
        return "select"
    if CMP.match(mn):
        return "cmp"
    if mn.startswith(("v_mov_b", "v_accvgpr", "v_swap")):
        return "mov"
    if mn.startswith("v_cvt_"):
        return "cvt"
    if F64.match(mn):
        return "f64"
    if INT.match(mn):
        return "int"
    return "other"


def build_asm() -> str:
    out_dir = os.path.join(CSRC, "build", "asm")
    os.makedirs(out_dir, exist_ok=True)
    flags = subprocess.run(["make", "-s", "-C", CSRC, "print-kernel-flags"], capture_output=True, text=True, check=True).stdout.split()
    subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-save-temps", "-c", "-o", "sart_kernels.o", os.path.join(CSRC, "sart_kernels.hip")],
                   check=True, cwd=out_dir, capture_output=True)
    return os.path.join(out_dir, "sart_kernels-hip-amdgcn-amd-amdhsa-gfx950.s")


def kernel_lines(asm_path: str, variant: int, fixed: bool, scan: bool = False, ascan: str | None = None):
    if variant in FOLDED:
        tag = "_ZN4sart23folded_histogram_kernelILi1024E" + FOLDED[variant] + ("Lb1E" if fixed else "Lb0E")
    else:
        tag = "_ZN4sart22trace_histogram_kernelILi1024E" + VARIANTS[variant] + ("Lb1E" if fixed else "Lb0E") + ("Lb1E" if scan else "Lb0E")
    if ascan:   # the fused angular scan: trace_angular_scan_kernel<1024, FAST, GAS, FIXED> (fast: <true, 0>, generic: <false, -1>)
        tag = "_ZN4sart25trace_angular_scan_kernelILi1024E" + ("Lb1ELi0E" if ascan == "fast" else "Lb0ELin1E") + ("Lb1E" if fixed else "Lb0E")
    lines = open(asm_path).read().splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith(tag) and l.rstrip().split(":")[0].startswith(tag) and ":" in l)
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    return lines[start:end + 1]


def histogram(lines):
    """-> {stage: {"hot": Counter(class), "rare": Counter(class), "mnemonics": Counter}}

    Hot / rare: the kernel is written in predicated form, so its hot path is straight-line code; what the compiler guards
    with `s_and_saveexec` + `s_cbranch_execz LABEL` (the region up to LABEL is skipped when no lane needs it) is a divergent
    alternative.  Such a region counts as RARE unless it carries a `; hot` or `; SART_STAGE` comment (ring writes, the
    accumulation of the passed rays); a `; rare` comment marks a region as rare whatever guards it; the body of a loop that is
    closed by `s_cbranch_execnz` (the data-dependent search loops) is rare as well.  Regions nest."""
    # pass 1: instructions with their guard stack
    insts = []            # (mnemonic, stage, region ids)
    regions = {}          # id -> {"end": label, "hot": bool, "rare": bool}
    stack = []
    stage = "PROLOGUE"
    next_id = 0
    loop_labels = {}      # label -> index of the first instruction after it (for execnz back edges)
    back_edge = None      # region of the s_cbranch_execnz just read
    copies = collections.Counter()   # a stage whose marker appears k times was inlined at k call sites: one of them runs per launch
    for raw in lines[1:]:
        l = raw.strip()
        if not l:
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            lab = m.group(1)
            # a label closes every open region that ends there
            stack[:] = [r for r in stack if regions[r]["end"] != lab]
            loop_labels[lab] = len(insts)
            continue
        if l.startswith(";"):
            ms = re.search(r"SART_STAGE (\w+)", l)
            if ms:
                stage = ms.group(1)
                copies[stage] += 1
                for r in stack:
                    regions[r]["hot"] = True
            if "; hot" in l:
                mw = re.search(r"; hot x([0-9.]+)", l)
                for r in stack:
                    regions[r]["hot"] = True
                if mw and stack:
                    regions[stack[-1]]["weight"] = float(mw.group(1))
            if "; rare" in l and stack:
                regions[stack[-1]]["rare"] = True
            continue
        if l.startswith(".") or l.endswith(":"):
            continue
        parts = l.split()
        mn = parts[0]
        # `s_cbranch_execnz EARLIER` followed by `s_branch`: the tail of a block the compiler placed out of line, which enters a
        # guarded region above it if a lane needs it and jumps behind that region otherwise - a guard, not the back edge of a loop
        if mn == "s_branch" and back_edge is not None:
            regions[back_edge].update(hot=True, rare=False)
        back_edge = None
        insts.append([mn, stage, tuple(stack), l])
        if mn == "s_cbranch_execz" and len(parts) > 1 and parts[1] not in loop_labels:   # (a label already seen: the guard of a loop, whose region no later label would close)
            regions[next_id] = {"end": parts[1], "hot": False, "rare": False, "weight": 1.0}
            stack.append(next_id)
            next_id += 1
        elif mn == "s_cbranch_execnz" and len(parts) > 1 and parts[1] in loop_labels:
            # back edge of a divergent loop: its body is a rare region of its own
            regions[next_id] = {"end": None, "hot": False, "rare": True, "weight": 1.0}
            for k in range(loop_labels[parts[1]], len(insts)):
                insts[k][2] = insts[k][2] + (next_id,)
            back_edge = next_id
            next_id += 1
    out = collections.OrderedDict()
    dump = []
    for mn, st, regs, text in insts:
        rare = any(regions[r]["rare"] or not regions[r]["hot"] for r in regs)
        w = 1.0
        for r in regs:
            w *= regions[r]["weight"]          # "; hot x0.25": executed in a quarter of the passes
        d = out.setdefault(st, {"hot": collections.Counter(), "rare": collections.Counter(), "mnemonics": collections.Counter()})
        d["rare" if rare else "hot"][classify(mn)] += 1 if rare else w
        if not rare and mn.startswith("v_"):
            d["mnemonics"][mn] += w
        if not rare:
            dump.append((st, classify(mn), text))
    histogram.hot_lines = dump
    histogram.copies = dict(copies)
    return out


VALU_CLASSES = ("f64", "int", "cmp", "select", "mov", "cvt", "lane", "other")

# Classes of the scalar instructions of the hot path (--salu): a wave issues one instruction of any kind per four cycles, so
# with four waves per SIMD each of these takes an issue slot that a vector instruction could have had.
SALU_CLASSES = ("literal_mov", "s_nop", "mask", "branch", "s_load", "s_setprio", "s_waitcnt", "other")
MASK = re.compile(r"s_(and|or|xor|andn2|orn2|nand|nor|xnor|not|mov|cselect|bcnt1_i32|ff1_i32|wqm)_b64|s_(and|or|xor|andn2|orn2)_saveexec_b64|s_cmp_(eq|lg)_u64")
SREG = re.compile(r"\bs(\d+)\b|\bs\[(\d+):(\d+)\]")


def salu_class(mn: str, text: str) -> str:
    if mn == "s_nop":
        return "s_nop"
    if mn.startswith("s_waitcnt"):
        return "s_waitcnt"
    if mn == "s_setprio":
        return "s_setprio"
    if mn.startswith(("s_load_", "s_buffer_load_")):
        return "s_load"
    if mn.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if mn == "s_mov_b32" and re.search(r",\s*(0x[0-9a-fA-F]+|-?\d+(\.\d+)?)\s*(;.*)?$", text):
        return "literal_mov"
    if MASK.match(mn) or "exec" in text or "vcc" in text:
        return "mask"
    return "other"


def sregs(operands: str) -> set:
    out = set()
    for m in SREG.finditer(operands):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def salu_breakdown(hot_lines):
    """hot_lines: (stage, class, text) of the hot path in program order -> {stage: {class: n, "s_nop_by_neighbours": {"prev -> next": n},
    "nop_between_literal_mov_and_reader": n}}.  An s_nop counts as `between a literal move and its reader` when the instruction in
    front of it is an s_mov_b32 of a literal and the instruction behind it names the register that move wrote."""
    out = collections.OrderedDict()
    scalar = lambda c: c in ("salu", "s_waitcnt")
    for i, (st, cls, text) in enumerate(hot_lines):
        if not scalar(cls):
            continue
        mn = text.split()[0]
        d = out.setdefault(st, {**{c: 0 for c in SALU_CLASSES}, "s_nop_by_neighbours": collections.Counter(), "nop_between_literal_mov_and_reader": 0})
        c = salu_class(mn, text)
        d[c] += 1
        if c == "s_nop":
            prev = hot_lines[i - 1][2] if i > 0 else ""
            nxt = hot_lines[i + 1][2] if i + 1 < len(hot_lines) else ""
            pm, nm = (prev.split() or ["-"])[0], (nxt.split() or ["-"])[0]
            if salu_class(pm, prev) == "literal_mov":
                pm = "s_mov_b32(literal)"
                dst = sregs(prev.split(",")[0])
                if dst & sregs(nxt.split(None, 1)[1] if " " in nxt else ""):
                    d["nop_between_literal_mov_and_reader"] += 1
            d["s_nop_by_neighbours"]["%s -> %s" % (pm, nm)] += 1
    for d in out.values():
        d["s_nop_by_neighbours"] = dict(d["s_nop_by_neighbours"].most_common())
    return out


# Kinds of the hot path's LDS reads (--lds), told apart by their addressing: the rings are read with the 64-element stride
# forms or beyond the tables (offset >= 32 KiB); the tables behind the parameter block (shell table, sine / cosine table, CDF
# guides) with a per-lane base register and an offset of 4 KiB or more; a read at a small immediate offset is a field of the
# DevBlob / TraceArgs copies at the head of LDS (one address for the whole wave: a broadcast) when its base register is one that
# serves several such fields in the stage, and a per-lane table access (base register = entry address) otherwise.
LDS_KINDS = ("ring", "table", "parameter", "per_lane_small_offset", "write_or_atomic")


def lds_breakdown(hot_lines):
    """-> {stage: {kind: n, "parameter_reads": [text, ...]}} of the hot path's ds_* instructions."""
    per_stage = collections.OrderedDict()
    for st, cls, text in hot_lines:
        if cls == "lds":
            per_stage.setdefault(st, []).append(text)
    out = collections.OrderedDict()
    for st, texts in per_stage.items():
        parsed = []
        for t in texts:
            mn = t.split()[0]
            ops = [o.strip() for o in t.split(None, 1)[1].split(",")] if " " in t else []
            unit = 8 if "b64" in mn else 4
            unit *= 64 if "st64" in mn else 1
            offs = [int(m.group(2)) * (unit if m.group(1) != "offset" else 1) for m in re.finditer(r"(offset[01]?):(\d+)", t)] or [0]
            is_read = mn.startswith("ds_read") or mn.startswith("ds_load")
            base = ops[1] if is_read and len(ops) > 1 else (ops[0] if ops else "")
            parsed.append((mn, base.split()[0] if base else "", max(offs), is_read, t))
        small = collections.Counter(b for mn, b, off, rd, t in parsed if rd and "st64" not in mn and off < 4096)
        d = {k: 0 for k in LDS_KINDS}
        d["parameter_reads"] = []
        for mn, base, off, rd, t in parsed:
            if not rd:
                kind = "write_or_atomic"
            elif "st64" in mn or off >= 32768:
                kind = "ring"
            elif off >= 4096:
                kind = "table"
            elif small[base] >= 3:
                kind = "parameter"
                d["parameter_reads"].append(t)
            else:
                kind = "per_lane_small_offset"
            d[kind] += 1
        out[st] = d
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", type=int, default=5, help="0 vacuum, 1 generic, 2 generic rotated, 3 gas, 4 rotated, 5 vacuum + constant path, 6 gas + constant path, 7 / 8 the folded forms of 5 / 6 (7: headline)")
    ap.add_argument("--fixed", action="store_true", help="the SART_ACCUM_FIXED64 instantiation")
    ap.add_argument("--scan", action="store_true", help="the fused mass-scan instantiation (variants 1, 2, 3, 6)")
    ap.add_argument("--ascan", default=None, choices=["fast", "generic"], help="the fused angular-scan kernel instead (stages A0, A1a, A1b, B, ACC)")
    ap.add_argument("--asm", default=None, help="existing listing (default: compile now)")
    ap.add_argument("--pmc", default=None, help="profiles/<tag>_<workload>_pmc_summary.json of the same build: measured totals beside the model")
    ap.add_argument("--passes-b", type=float, default=None, help="phase-B passes per 64 launched rays (default: from --pmc results or 0.3295)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--salu", action="store_true", help="per-stage breakdown of the hot path's scalar instructions (also part of --json)")
    ap.add_argument("--lds", action="store_true", help="per-stage breakdown of the hot path's LDS instructions: ring, table, parameter broadcast (also part of --json)")
    ap.add_argument("--dump", default=None, help="comma-separated classes: print the hot-path instructions of these classes (e.g. mov,select,cvt,lane)")
    args = ap.parse_args()
    asm = args.asm or build_asm()
    h = histogram(kernel_lines(asm, args.variant, args.fixed, args.scan, args.ascan))
    report = {"variant": args.variant, "fixed64": args.fixed, "stages": {}, "how": "tools/isa_histogram.py: static counts of the hot path "
              "(blocks without a `; rare` marker) per stage of the gfx950 listing; rare = the divergent alternatives"}
    print("%-9s %5s | " % ("stage", "VALU") + " ".join("%6s" % c for c in VALU_CLASSES) + " | salu  lds vmem atom wait | rare VALU")
    for st, d in h.items():
        valu = sum(d["hot"][c] for c in VALU_CLASSES)
        rare = sum(d["rare"][c] for c in VALU_CLASSES)
        print("%-9s %5.0f | " % (st, valu) + " ".join("%6.0f" % d["hot"][c] for c in VALU_CLASSES) +
              " | %4d %4d %4d %4d %4d | %5d" % (d["hot"]["salu"], d["hot"]["lds"], d["hot"]["vmem"], d["hot"]["vmem_atomic"], d["hot"]["s_waitcnt"], rare))
        report["stages"][st] = {"copies_in_listing": histogram.copies.get(st, 1), "valu": valu, **{c: d["hot"][c] for c in VALU_CLASSES}, "salu": d["hot"]["salu"], "lds": d["hot"]["lds"],
                                "vmem": d["hot"]["vmem"], "vmem_atomic": d["hot"]["vmem_atomic"], "s_waitcnt": d["hot"]["s_waitcnt"],
                                "rare_valu": rare,
                                "top_non_arithmetic": [[k, v] for k, v in d["mnemonics"].most_common() if classify(k) in ("cmp", "select", "mov", "cvt", "lane", "other")][:14]}
    salu = salu_breakdown(histogram.hot_lines)
    for st, d in salu.items():
        report["stages"][st]["salu_by_kind"] = d
    if args.salu:
        print("%-9s " % "stage" + " ".join("%11s" % c for c in SALU_CLASSES) + " | nop between literal s_mov and its reader")
        for st, d in salu.items():
            print("%-9s " % st + " ".join("%11d" % d[c] for c in SALU_CLASSES) + " | %d" % d["nop_between_literal_mov_and_reader"])
        for st, d in salu.items():
            for k, v in d["s_nop_by_neighbours"].items():
                print("  s_nop %-8s %3d  %s" % (st, v, k))
    lds = lds_breakdown(histogram.hot_lines)
    for st, d in lds.items():
        report["stages"][st]["lds_by_kind"] = d
    if args.lds:
        print("%-9s " % "stage" + " ".join("%22s" % c for c in LDS_KINDS))
        for st, d in lds.items():
            print("%-9s " % st + " ".join("%22d" % d[c] for c in LDS_KINDS))
        for t in lds.get("B", {}).get("parameter_reads", []):
            print("  B parameter read  %s" % t)
    if args.dump:
        want = set(args.dump.split(","))
        for st, cls, text in histogram.hot_lines:
            if cls in want:
                print("%-8s %-6s %s" % (st, cls, text))
    if args.pmc:
        pmc = json.load(open(args.pmc))
        meas = pmc["derived"]["valu_insts_per_64_rays"]
        pb = args.passes_b if args.passes_b is not None else 0.3295
        s = report["stages"]
        # phase A is inlined at two call sites (with / without stage A0 in front of it); a launch runs one of them
        g = lambda k: s.get(k, {"valu": 0})["valu"] / (histogram.copies.get(k, 1) if k == "A1" else 1)
        fixed_part = g("A0") * 1.0 + (g("B") + g("ACC")) * pb
        pa = (meas - fixed_part) / max(1, g("A1"))
        report["model"] = {"measured_valu_per_64_rays": meas, "passes": {"A0": 1.0, "A1": pa, "B": pb},
                           "note": "passes(A1) solved from measured = A0 + A1 x passes(A1) + (B + ACC) x passes(B); the expected value is the "
                                   "share of rays that survive stage A0 (~0.48 for BabyIAXO) plus drain passes",
                           "per_class_per_64_rays": {c: s.get("A0", {}).get(c, 0) + s.get("A1", {}).get(c, 0) / histogram.copies.get("A1", 1) * pa +
                                                     (s.get("B", {}).get(c, 0) + s.get("ACC", {}).get(c, 0)) * pb for c in VALU_CLASSES}}
        print("measured VALU / 64 rays %.1f -> passes(A1) = %.3f with passes(B) = %.4f" % (meas, pa, pb))
        print("per class per 64 launched rays:", {k: round(v, 1) for k, v in report["model"]["per_class_per_64_rays"].items()})
    if args.json:
        json.dump(report, open(args.json, "w"), indent=1)
        print("wrote", args.json)


if __name__ == "__main__":
    main()
