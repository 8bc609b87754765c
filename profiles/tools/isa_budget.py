#!/usr/bin/env python3
"""Static VALU budget of the main march loop of the benchmarked sweeps, by section of the source.

Cross-compiles csrc/qk_hydro_fused.hip for gfx950 with the Makefile's flags plus line tables (-gline-tables-only: same code, and the listing then
carries, behind every .loc, the chain of inlined call sites), finds the main loop of each requested kernel — the widest backward branch — and
books every VALU instruction in it to a section according to the functions on its inline chain.  Loops are counted once: the figures are static,
the batch pass of the fused XY march executes one step in sixteen, rare branches count in full.

usage: isa_budget.py [--root TREE] [--asm FILE.s] [--keep FILE.s]      (TREE: a checkout of this repository, default the one this file is in)"""
import argparse
import collections
import os
import re
import subprocess
import sys

KERNELS = [("XY stage 1  k_sweep_march<1,3,1,false,0,true,false,false,FUSEX,GFS>", "13k_sweep_marchILi1ELi3ELi1ELb0ELi0ELb1ELb0ELb0ELb1ELb1EE"),
           ("XY stage 2  k_sweep_march<1,3,2,false,0,true,false,false,FUSEX,GFS>", "13k_sweep_marchILi1ELi3ELi2ELb0ELi0ELb1ELb0ELb0ELb1ELb1EE"),
           ("Z  stage 1  k_sweep_march<2,3,1,LAST,0,true,false,false,false,GFS>", "13k_sweep_marchILi2ELi3ELi1ELb1ELi0ELb1ELb0ELb0ELb0ELb1EE"),
           ("Z  stage 2  k_sweep_march<2,3,2,LAST,0,true,false,false,false,GFS>", "13k_sweep_marchILi2ELi3ELi2ELb1ELi0ELb1ELb0ELb0ELb0ELb1EE")]
# section <- any of these functions on the inline chain; the first rule that matches wins (outermost concerns first)
RULES = [("batch pass", {"fusexEdgeBatch", "stageEdgeRow"}),
         ("epilogue", {"updateCellFrom", "reduceSignal", "epiConst", "epiTgas", "epiEint", "enforceLimits", "syncDualEnergy", "signalSpeed", "atomicMaxNonNeg", "cellCentredDivV"}),
         ("conversion", {"consToPrim", "primsOf", "loadPrims", "marchBase", "xorSign"}),
         ("PPM", {"ppmEdges", "plmEdges", "MC", "minmod", "halfSgnSum", "halfSign", "cellEdges", "sgn"}),
         ("flatten blend", {"flattenEdges", "reconstructVar", "reconstructCell"}),
         ("HLLC", {"faceFluxAll", "faceFlux", "hllc", "makeState", "scalarFlux", "llf"}),
         ("face settle", {"settleFace", "maskedFaceFlux", "maskByte", "loadF1"}),
         ("row exchange", {"putColumn", "getColumn", "waveFence"})]
ORDER = ["conversion", "PPM", "flatten blend", "HLLC", "divergence", "batch pass", "row exchange", "face settle", "addressing", "epilogue", "no line"]
DEF = re.compile(r"^(?:template\s*<[^;{]*>\s*)?(?:QK_DEV|__global__|inline|static|auto|__host__|__device__)[^;=]*?\b([A-Za-z_]\w*)\s*\(")


def function_ranges(path):
    """line -> name of the function whose definition starts last at or before it (definitions start in column 0 in this code base)"""
    names, cur = {}, None
    pending_template = False
    for no, line in enumerate(open(path, errors="replace"), 1):
        if line[:1] not in " \t/#}\n" or pending_template:
            m = DEF.match(line)
            if m and m.group(1) not in ("if", "for", "while", "switch", "return", "__launch_bounds__"):
                cur = m.group(1)
            elif line.startswith("__global__") or pending_template:
                m2 = re.search(r"\b(k_\w+)\s*\(", line)
                if m2:
                    cur = m2.group(1)
            pending_template = line.startswith("template") and "(" not in line
        names[no] = cur
    return names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    ap.add_argument("--asm", default=None, help="a listing made earlier with --keep")
    ap.add_argument("--keep", default=None)
    args = ap.parse_args()
    csrc = os.path.join(os.path.abspath(args.root), "quokka_amd", "csrc")
    asm = args.asm
    if asm is None:
        asm = args.keep or "/tmp/isa_budget.s"
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-I../../include", "-I.",
                               "-gline-tables-only", "--cuda-device-only", "-S", "qk_hydro_fused.hip", "-o", asm], cwd=csrc, stderr=subprocess.DEVNULL)
    ranges = {}

    def func_at(fname, line):
        base = os.path.basename(fname)
        if base not in ranges:
            p = os.path.join(csrc, base)
            ranges[base] = function_ranges(p) if os.path.exists(p) else {}
        return ranges[base].get(line)

    txt = open(asm).read().split("\n")
    starts = [(i, l.split(":")[0]) for i, l in enumerate(txt) if re.match(r"^_Z\S+:", l)]
    starts.append((len(txt), None))
    print("static VALU instructions of the main march loop by section (isa_budget.py; loops counted once, rare branches in full)")
    for label, key in KERNELS:
        for (i0, name), (i1, _) in zip(starts, starts[1:]):
            if key in name:
                break
        else:
            print(f"{label}: not found")
            continue
        body = txt[i0:i1]
        for k, l in enumerate(body):
            if l.strip().startswith("s_endpgm"):
                body = body[:k + 1]
                break
        lab = {m.group(1): k for k, l in enumerate(body) for m in [re.match(r"^(\.LBB\w+):", l)] if m}
        best = (0, 0, 0)
        for k, l in enumerate(body):
            m = re.match(r"^\s+s_c?branch\w*\s+(\.LBB\w+)", l)
            if m and m.group(1) in lab and lab[m.group(1)] < k and k - lab[m.group(1)] > best[0]:
                best = (k - lab[m.group(1)], lab[m.group(1)], k)
        _, l0, l1 = best
        sect, mix = collections.Counter(), collections.defaultdict(collections.Counter)
        chain = []
        for k, l in enumerate(body):
            m = re.match(r"^\s+\.loc\s+\d+\s+(\d+)\s+\d+[^;]*;\s*(.*)$", l)
            if m:
                chain = [(f, int(n)) for f, n in re.findall(r"([^\s\[\]@]+):(\d+):\d+", m.group(2))]
                continue
            if k < l0 or k > l1 or not l.startswith("\t"):
                continue
            t = l.strip()
            if not t.startswith("v_"):
                continue
            funcs = [func_at(f, n) for f, n in chain]
            s = None
            for sec, fs in RULES:
                if any(f in fs for f in funcs):
                    s = sec
                    break
            if s is None:
                if not chain or all(n == 0 for _, n in chain):  # (line 0: code the compiler merged from several places)
                    s = "no line"
                else:  # the kernel's own text: the flux differences and quotients of the divergence are f64 arithmetic, everything else is index work
                    s = "divergence" if "f64" in t.split()[0] else "addressing"
            sect[s] += 1
            mix[s][t.split()[0]] += 1
        total = sum(sect.values())
        allv = collections.Counter(l.strip().split()[0] for l in body[l0:l1 + 1] if l.startswith("\tv_"))
        print(f"\n{label}\n  main loop: {l1 - l0 + 1} lines of listing, VALU {total}")
        for s in ORDER:
            if sect[s]:
                extra = f"   ({sect[s] / 6:.0f} per variable and edge pair)" if s == "PPM" else ""
                top = ", ".join(f"{op} {c}" for op, c in mix[s].most_common(4))
                print(f"  {s:<14} {sect[s]:>5}  {100.0 * sect[s] / total:5.1f} %{extra}   [{top}]")
        pick = lambda *p: sum(c for op, c in allv.items() if any(op.startswith(q) for q in p))
        print(f"  of these: v_cmp*_f64 {pick('v_cmp') - pick('v_cmp_class') - sum(c for op, c in allv.items() if op.startswith('v_cmp') and 'f64' not in op)}, "
              f"v_cndmask {pick('v_cndmask')}, v_subbrev/v_addc {pick('v_subbrev', 'v_addc')}, v_cvt_f64_i32 {pick('v_cvt_f64_i32')}, v_cvt_f64_f32 {pick('v_cvt_f64_f32')}, "
              f"v_bfi {pick('v_bfi')}, v_div_scale {pick('v_div_scale')}, v_rcp_f64 {pick('v_rcp_f64')}, global_load "
              f"{sum(1 for l in body[l0:l1 + 1] if l.startswith(chr(9) + 'global_load'))}")


if __name__ == "__main__":
    sys.exit(main())
