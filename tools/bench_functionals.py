#!/usr/bin/env python3
"""Time the post-processing entries of include/pfm_newton.h on the 3-D Sneddon box (216^3 cells by default):

  pfm_cod_lines          the reference's 769 lines (compute_functional_values), cold (geometry pass + value pass; a
                         different eps every call forces the rebuild) and cached (value pass only)
  pfm_face_load          the x = +10 face of the box (216^2 faces)
  pfm_sneddon_phi_error  every cell
  pfm_point_eval         1 point and 4096 points (the cell search is a sweep over every cell)
  pfm_cod_buckets        the reference's call (75, -1.5, 1.5, 100) on a 2-D box of --buckets-2d-n^2 cells and on a 3-D box of
                         --buckets-3d-n^3 cells over [-1.5, 1.5]^dim (1e4 / 1e6 sample points per cell), --buckets-reps calls

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
    ap.add_argument("--buckets-2d-n", type=int, default=1000)
    ap.add_argument("--buckets-3d-n", type=int, default=32)
    ap.add_argument("--buckets-reps", type=int, default=3)
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

    def timed(fn, reps=None):
        ts = []
        for _ in range(reps or args.reps):
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

    rng = np.random.default_rng(0)
    pts = rng.uniform(-9.9, 9.9, (4096, dim))
    found = int((ctx.point_eval(pts)[0] >= 0).sum())
    pe1 = timed(lambda: ctx.point_eval(pts[:1]))
    pe4096 = timed(lambda: ctx.point_eval(pts))
    del ctx

    buckets = {}
    for bdim, bn in ((2, args.buckets_2d_n), (3, args.buckets_3d_n)):
        bmesh = M.box_mesh(bdim, bn, lo=-1.5, hi=1.5)
        x = bmesh.coords
        bu = np.stack([1e-3 * np.sin(x[:, c]) * x[:, (c + 1) % bdim] for c in range(bdim)], axis=1)
        bphi = 0.5 + 0.5 * np.tanh(4.0 * np.abs(x[:, 1]) - 0.3)
        blay = M.DofLayout(bmesh.n_nodes, bdim, blocked=True)
        bsol = blay.pack(bu, bphi)
        bctx = Context(bmesh, True)
        bctx.set_params(bench.sneddon_params(bmesh.min_cell_diameter(), bdim))
        bctx.state_set_host(bsol, bsol, bsol)
        bctx.cod_buckets(75, -1.5, 1.5, 2)  # warm-up (module load)
        t = timed(lambda: bctx.cod_buckets(), args.buckets_reps)
        n_points = bmesh.n_cells * 100 ** bdim
        buckets["%dd" % bdim] = {"n_cells": int(bmesh.n_cells), "n_sub": 100, "points": int(n_points), "cod_buckets_ms": t[0],
                                 "cod_buckets_min_ms": t[1], "ns_per_1e3_points": 1e9 * t[0] / n_points,
                                 "volume": float(bctx.cod_buckets()[1].sum())}
        del bctx

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
        "point_eval_1_ms": pe1[0], "point_eval_1_min_ms": pe1[1], "point_eval_4096_ms": pe4096[0],
        "point_eval_4096_min_ms": pe4096[1], "point_eval_found": found, "cod_buckets": buckets,
    }))


if __name__ == "__main__":
    main()
