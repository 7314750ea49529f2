#!/usr/bin/env python3
"""Compare the compiler's kernel resource lines of two builds of one source file.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics --cuda-device-only -c cracks_amd/csrc/pfm_kernels.hip \
          -o /dev/null -Rpass-analysis=kernel-resource-usage 2> child.txt        (the same in a checkout of the parent: parent.txt)
    tools/resource_lines.py parent.txt child.txt [filter]

Prints a markdown table: per kernel (demangled, `filter` a substring of the name) VGPRs, AGPRs, scratch bytes per lane and LDS
bytes of both builds, and whether they are equal; kernels only one build has are listed with the other side empty.
Exit status 1 when a kernel that both builds have differs in one of these."""
import re
import subprocess
import sys

KEYS = [("VGPRs", r"\bVGPRs: (\d+)"), ("AGPRs", r"\bAGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("LDS", r"LDS Size \[bytes/block\]: (\d+)")]


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for k, pat in KEYS:
            m = re.search(pat, line)
            if m:
                cur[k] = int(m.group(1))
    return out


def demangle(names):
    try:
        txt = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, txt))
    except Exception:
        return {n: n for n in names}


def short(name):
    name = name.replace("pfm::(anonymous namespace)::", "").replace("void ", "")
    return re.sub(r"\(.*$", "", name)


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    flt = sys.argv[3] if len(sys.argv) > 3 else ""
    names = sorted(set(a) | set(b))
    dm = demangle(names)
    bad = 0
    print("| kernel | parent VGPR/AGPR/scratch/LDS | this build | |")
    print("|---|---|---|---|")
    for n in names:
        if flt not in dm[n]:
            continue
        fa, fb = a.get(n), b.get(n)
        cell = lambda f: "" if f is None else "/".join(str(f.get(k, "?")) for k, _ in KEYS)
        same = "new" if fa is None else "gone" if fb is None else "same" if cell(fa) == cell(fb) else "DIFFERS"
        bad += same == "DIFFERS"
        print(f"| `{short(dm[n])}` | {cell(fa)} | {cell(fb)} | {same} |")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
