#!/usr/bin/env python3
"""Per-kernel resources of csrc/norm.hip (VGPRs, AGPRs, SGPRs, scratch, LDS, occupancy), both operand builds, with the Makefile's flags:
the table a change of norm.hip is judged by.  Needs hipcc only, no GPU.

  python scripts/norm_resources.py                   this tree, one line per kernel instantiation
  python scripts/norm_resources.py --against DIR     ... beside the same table of another checkout's prediff_amd/csrc (e.g. a worktree of
                                                     the parent commit); exit status 1 if a kernel gained scratch or lost occupancy
"""
import argparse
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC"]          # csrc/Makefile CXXFLAGS (warnings aside)
FIELDS = (("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"), ("VGPRs Spill", "vspill"), ("SGPRs Spill", "sspill"),
          ("LDS Size [bytes/block]", "lds"), ("Occupancy [waves/SIMD]", "occ"))


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool:
        return list(names)
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return out.split("\n")[:len(names)]


def resources(csrc, f16):
    cmd = [HIPCC] + FLAGS + (["-DPD_BUILD_F16"] if f16 else []) + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "norm.hip",
                                                                    "-o", os.devnull]
    err = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, check=True).stderr
    table, cur = {}, None
    for line in err.split("\n"):
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = table.setdefault(m.group(1), {})
            continue
        for label, key in FIELDS:
            m = re.search(r"remark: .*\s" + re.escape(label) + r": (\d+)", line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    names = sorted(table)
    # name and template arguments only: the namespace and the parameter list would fill the line
    short = []
    for d in demangle(names):
        d = re.sub(r"^void ", "", d).replace("pdk_bf16::", "").replace("pdk_f16::", "")
        d = d[:d.rindex(">(") + 1] if ">(" in d else d.split("(")[0]
        for i, kind in enumerate(("Op16", "E4M3", "MX")):
            d = d.replace("(Out)%d" % i, kind)
        short.append(d)
    return {("f16 " if f16 else "bf16 ") + s: table[n] for n, s in zip(names, short)}


def fmt(r):
    return "%3d v %2d a %3d scratch %d/%d spill %5d lds occ %d" % (r["vgpr"], r["agpr"], r["scratch"], r["vspill"], r["sspill"], r["lds"], r["occ"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--against", help="another checkout's prediff_amd/csrc")
    a = ap.parse_args()
    here = os.path.join(ROOT, "prediff_amd", "csrc")
    this = {**resources(here, False), **resources(here, True)}
    if not a.against:
        for k in sorted(this):
            print("%-60s %s" % (k, fmt(this[k])))
        return 0
    other = {**resources(a.against, False), **resources(a.against, True)}
    bad = 0
    for k in sorted(set(this) | set(other)):
        t, o = this.get(k), other.get(k)
        if t is None or o is None:
            print("%-60s %s   only in %s" % (k, fmt(t or o), "this tree" if t else "the other"))
            continue
        worse = t["scratch"] > o["scratch"] or t["occ"] < o["occ"]
        bad += worse
        print("%-60s %s   %s" % (k, fmt(t), "same" if t == o else ("WORSE, was " if worse else "differs, was ") + fmt(o)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
