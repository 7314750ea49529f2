#!/usr/bin/env python3
"""Extract the ``PStress:`` column compute_point_stress prints every time step (cracks.cc:3319) from the reference's
three-point bending golden into tests/golden/point_stress.json.

Data only.  Usage, from the repository root:
    python tests/golden/make_point_stress.py <the reference's tests/ directory>
Re-running it reproduces the file byte for byte.
"""
import json
import os
import re
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "point_stress.json")
CASES = ["threepoint_1.mpirun=2"]
NUM = r"(-?[0-9.]+(?:e[-+]?[0-9]+)?)"


def parse(path):
    rec = {"source": "tests/" + os.path.basename(path), "point": ["0.0", "2.0"], "pstress": []}
    with open(path) as f:
        for line in f:
            m = re.match(r"No ([0-9]+) time " + NUM + r" .* PStress: " + NUM + r"\s*$", line)
            if m:
                assert int(m.group(1)) == len(rec["pstress"])
                # numbers are kept as the printed strings: the printed digits are the precision of the golden
                rec["pstress"].append(m.group(3))
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
