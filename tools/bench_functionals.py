#!/usr/bin/env python3
"""Time the post-processing entries of include/pfm_newton.h on the 3-D Sneddon box (216^3 cells by default):

  pfm_cod_lines          the reference's 769 lines (compute_functional_values), cold (geometry pass + value pass; a
                         different eps every call forces the rebuild) and cached (value pass only)
  pfm_face_load          the x = +10 face of the box (216^2 faces)
  pfm_sneddon_phi_error  every cell

HIP events around each (synchronous) call, median of --reps calls.  For context, the numpy restatement
(tests/postproc_ref.py) of ONE compute_cod line on a small box.  Prints one JSON line.

    python tools/bench_functionals.py [--n 216] [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=216)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--np-n", type=int, default=24, help="cells per axis of the numpy comparison box")
    args = ap.parse_args()

    import torch

    import bench
    import postproc_ref as R
    from cracks_amd import mesh as M
    from cracks_amd import partition as P
    from cracks_amd import statistics as S
    from cracks_amd.assembler import Context

    dim, n = 3, args.n
    lp = P.build_local_problem(dim, (n,) * dim, (1, 1, 1), 0)
    mesh = lp.mesh
    h = (20.0 / n) * np.sqrt(dim)
    u, phi, po, poo, _ = bench.synthetic_state(mesh, lp.global_ids, h, dim)
    lay = M.DofLayout(mesh.n_nodes, dim, blocked=True)
    sol = lay.pack(u, phi)
    ctx = Context(mesh, True)
    ctx.set_params(bench.sneddon_params(h, dim))
    ctx.state_set_host(sol, lay.pack(0 * u, po), lay.pack(0 * u, poo))
    cells = np.nonzero(mesh.coords[mesh.cells[:, 1], 0] == 10.0)[0].astype(np.int32)  # vertex 1 lies on the x-hi side
    faces = np.ones(cells.size, np.uint8)
    lines = S.cod_lines()

    def timed(fn):
        ts = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts)), float(np.min(ts))

    eps_cycle = [1e-8 * (1.0 + 1e-6 * k) for k in range(2)]
    calls = {"k": 0}

    def cold():
        calls["k"] += 1
        ctx.cod_lines(lines, None, eps_cycle[calls["k"] % 2])

    ctx.cod_lines(lines)  # warm-up (module load)
    cod_cold = timed(cold)
    cod, nf = ctx.cod_lines(lines)
    cod_cached = timed(lambda: ctx.cod_lines(lines))
    ctx.face_load(cells, faces)
    load = timed(lambda: ctx.face_load(cells, faces))
    ctx.sneddon_phi_error_sq()
    phi_err = timed(lambda: ctx.sneddon_phi_error_sq())

    small = M.box_mesh(3, args.np_n, lo=-1.5, hi=1.5)
    slay = M.DofLayout(small.n_nodes, 3, blocked=True)
    ssol = slay.pack(np.zeros((small.n_nodes, 3)), np.ones(small.n_nodes))
    t0 = time.perf_counter()
    R.cod_lines(small, slay, ssol, np.array([0.0]))
    t_np = time.perf_counter() - t0

    print(json.dumps({
        "metric": "postproc_functionals", "n_cells": int(mesh.n_cells), "n_lines": int(lines.size),
        "lines_with_faces": int((nf > 0).sum()), "matched_faces": int(nf.sum()), "load_faces": int(cells.size),
        "cod_cold_ms": cod_cold[0], "cod_cold_min_ms": cod_cold[1], "cod_cached_ms": cod_cached[0],
        "cod_cached_min_ms": cod_cached[1], "face_load_ms": load[0], "face_load_min_ms": load[1],
        "phi_error_ms": phi_err[0], "phi_error_min_ms": phi_err[1], "reps": args.reps,
        "numpy_one_line_s": t_np, "numpy_one_line_cells": int(small.n_cells),
    }))


if __name__ == "__main__":
    main()
