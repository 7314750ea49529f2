#!/usr/bin/env python3
"""Extract the predictor-corrector refinement run of the reference's tests/miehe_shear_1.output into
tests/golden/amr_miehe_shear_1.json.

    python tests/golden/make_amr_kat.py <path to the reference checkout>

Data only.  One record per "Timestep" block of the output, the blocks that are redone after a "MESH CHANGED!" included,
in the order in which they are printed: cells and DoFs of the header line, the line-0 residual, the Newton rows, whether
the block ends in a mesh change, and the numbers of the "No ..." line (energies, load) where the block has one -- a
block that ends in a mesh change has none (cracks.cc:4419-4431 jumps back before the statistics).  Only the JSON is read
by the tests."""
import json
import os
import re
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "amr_miehe_shear_1.json")


def parse(path):
    blocks = []
    cur = None
    with open(path) as f:
        for lineno, line in enumerate(f, 1):
            line = line.rstrip("\n")
            m = re.match(r"Timestep (\d+): (\S+) \((\S+)\)\s+Cells: (\d+)\s+DoFs: (\d+)", line)
            if m:
                cur = {"timestep": int(m.group(1)), "time_before": float(m.group(2)), "dt": float(m.group(3)),
                       "cells": int(m.group(4)), "dofs": int(m.group(5)), "line": lineno, "newton": [],
                       "mesh_changed": False}
                blocks.append(cur)
                continue
            if cur is None:
                continue
            m = re.match(r"0\t\t\t(\S+)$", line)
            if m:
                cur["residual0"] = float(m.group(1))
            m = re.match(r"(\d+)\t(\d+)\t(\d+)\t(\S+)\t(\S+)\t(\d+)\t(\d+)$", line)
            if m:
                cur["newton"].append({"it": int(m.group(1)), "active_set": int(m.group(2)), "cycling": int(m.group(3)),
                                      "residual": float(m.group(4)), "reduction": float(m.group(5)),
                                      "line_search": int(m.group(6)), "lin_its": int(m.group(7))})
            if line.startswith("MESH CHANGED!"):
                cur["mesh_changed"] = True
            m = re.match(r"No (\d+) time (\S+) bulk energy: (\S+) crack energy: (\S+)\s+Load x: (\S+)", line)
            if m:
                assert int(m.group(1)) == cur["timestep"]
                cur["time"] = float(m.group(2))
                cur["bulk_energy"] = float(m.group(3))
                cur["crack_energy"] = float(m.group(4))
                cur["load_x"] = float(m.group(5))
    return blocks


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    src = os.path.join(sys.argv[1], "tests", "miehe_shear_1.output")
    blocks = parse(src)
    with open(OUT, "w") as f:
        json.dump({"source": "tests/miehe_shear_1.output", "blocks": blocks}, f, indent=1, sort_keys=True)
    print("wrote", OUT, "with", len(blocks), "blocks,", sum(b["mesh_changed"] for b in blocks), "mesh changes")


if __name__ == "__main__":
    main()
