#!/usr/bin/env python3
"""Static instruction mix of a marching kernel per PHASE of its plane loop: the kernel's text between two s_barrier.

  python tools/isa_phases.py cracks_amd/csrc/pfm_cart_uu3.hip --kernel 'k_cart_uu3ILi3ELb0ELb0ELb1E' [--asm file.s] [--json out.json]

The segments follow the barriers in program order (tools/isa_mix.py compiles and classifies).  For k_cart_uu3 they are:
prologue (in front of the loop) | top of a plane: residual rows of the last plane, landing and row requests of waves 5-7, w*g |
moment tables, node requests of waves 6, 7 | pressure part, table reads, row component 0 | copy-out 0, component 1 |
copy-out 1, component 2 | copy-out 2 (up to the loop's back edge) and the epilogue.  A segment holds EVERY arm of its
branches -- the eight slot sets, masked and unmasked, the regular and both face copy-outs -- so the numbers compare two
builds of one kernel; what one wave executes per plane is in the blocks of tools/isa_mix.py --blocks."""
from __future__ import annotations

import argparse
import collections
import json
import re

import isa_mix

NAMES_UU3 = ["prologue", "top: residual rows, landing/requests, w*g", "moments, node requests", "tables, component 0",
             "copy-out 0, component 1", "copy-out 1, component 2", "copy-out 2, epilogue"]
COLS = ["valu", "valu_fp64", "valu_int_other", "valu_mov", "valu_cmp_select", "valu_lane_permute", "lds", "vmem", "salu", "s_waitcnt"]


def phases(asm_path: str, pattern: str):
    txt = open(asm_path).read()
    out = {}
    for m in re.finditer(r"\n(_Z\S+):[^\n]*\n(.*?)\n\s*s_endpgm", txt, re.S):
        name, body = m.group(1), m.group(2)
        if pattern and not re.search(pattern, name):
            continue
        segs = []
        for seg in re.split(r"\n\ts_barrier[^\n]*", body):
            c = collections.Counter(isa_mix.classify(op) for op in isa_mix.instructions(seg))
            c["valu"] = sum(v for k, v in c.items() if k.startswith("valu"))
            c["salu"] += c["smem"]
            segs.append({k: c[k] for k in COLS})
        out[name] = segs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("source")
    ap.add_argument("--kernel", default="")
    ap.add_argument("--asm", default="")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    res = phases(a.asm or isa_mix.compile_to_asm(a.source), a.kernel)
    for name, segs in res.items():
        print(name)
        print("| phase | " + " | ".join(c.replace("valu_", "").replace("_other", "") for c in COLS) + " |")
        print("|---|" + "---:|" * len(COLS))
        for i, s in enumerate(segs):
            # (with the residual rows a last barrier follows the loop: the epilogue is a segment of its own)
            known = "k_cart_uu3" in name and len(segs) in (len(NAMES_UU3), len(NAMES_UU3) + 1)
            label = (NAMES_UU3 + ["epilogue: residual rows of the last plane"])[i] if known else f"segment {i}"
            print(f"| {label} | " + " | ".join(str(s[c]) for c in COLS) + " |")
        tot = {c: sum(s[c] for s in segs) for c in COLS}
        print("| all | " + " | ".join(str(tot[c]) for c in COLS) + " |")
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
