#!/usr/bin/env python3
"""Extract the post-processing numbers of the reference's Sneddon goldens that make_kat.py does not parse into
tests/golden/postproc.json: the TCV line (cracks.cc:3604-3607), the COD lines compute_functional_values prints
(``<x>  <value>`` after ``writing cod-..``, cracks.cc:3545) and the phi L2 error (cracks.cc:4520).

Data only.  Usage, from the repository root:
    python tests/golden/make_postproc.py <the reference's tests/ directory>
Re-running it reproduces the file byte for byte.
"""
import json
import os
import re
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "postproc.json")
CASES = ["sneddon_2d_1", "sneddon_3d_1.mpirun=4"]
NUM = r"(-?[0-9.]+(?:e[-+]?[0-9]+)?)"


def parse(path):
    rec = {"source": "tests/" + os.path.basename(path), "cod": []}
    in_cod = False
    with open(path) as f:
        for line in f:
            line = line.rstrip("\n")
            m = re.match(r"Timestep difference linfty: " + NUM, line)
            if m:
                rec["timestep_difference"] = m.group(1)
            m = re.match(r"TCV: value= " + NUM + " exact= " + NUM + " error= " + NUM, line)
            if m:
                rec["tcv"], rec["tcv_exact"], rec["tcv_error"] = m.group(1), m.group(2), m.group(3)
                continue
            if line.startswith("writing cod-"):
                in_cod = True
                continue
            m = re.match(NUM + "  " + NUM + "$", line)
            if in_cod and m:
                rec["cod"].append([m.group(1), m.group(2)])
                continue
            m = re.match(r"phi_L2_error: " + NUM + " h: " + NUM, line)
            if m:
                rec["phi_L2_error"], rec["h"] = m.group(1), m.group(2)
                in_cod = False
    # numbers are kept as the printed strings: the printed digits are the precision of the golden
    return rec


def main(ref_tests):
    out = {c: parse(os.path.join(ref_tests, c + ".output")) for c in CASES}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(OUT)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
