#!/usr/bin/env python3
"""Time the assemblies of meshes with hanging nodes per hanging mode (pfm_set_hanging_mode), in one process:

  config5   the config-5 stand-in mesh of bench.py (unit-slit square, 2^9 base cells per edge + refined band, 2.7e5 quads,
            stress split on, one-block layout), as the context chooses to run (patch overlay + general family);
  block3d   the 3-D block-refined mesh of bench.py's extra.overlay_3d (n^3 hexes, inner half refined once) under the spectral
            split (model 1): a split assembly runs the general family over all cells.

Per mesh: Jacobian and residual-only assembly, the modes alternating round by round.  Kernel time from the library's own
events around each assembly (pfm_timing_enable), median and minimum over --reps assemblies after --warmup, as
tools/bench_split3d.py does.  The gather result is compared with the default's on the timed state.  One JSON line per mesh.

    python tools/bench_hanging.py [--mesh config5 block3d] [--modes default gather atomic] [--reps 20] [--warmup 3] [--rounds 5] [--n 84]

--modes default alone also runs on an older build of the library that has no pfm_set_hanging_mode (PFM_LIB=..., tools/ab.sh):
the A/B of a build against its parent, both in the default mode."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def config5(args):
    import bench
    from cracks_amd.assembler import Assembler

    pb = bench.config5_problem(8, 1)
    asm = Assembler(pb["mesh"], blocked=False)
    asm.allocate_matrix()
    asm.set_params(pb["params"])
    asm.set_constraints(pb["node_flags"])
    asm.set_vectors(*pb["vectors"])
    return asm, pb["mesh"], "config-5 stand-in: unit-slit square with a refined band, stress split on, one-block layout"


def block3d(args):
    import oracle_api as O
    from cracks_amd import capi
    from cracks_amd import mesh as M
    from cracks_amd.assembler import Assembler

    n = args.n
    g0 = M.box_mesh(3, (n,) * 3)
    cc = g0.coords[g0.cells].mean(axis=1)
    mesh = M.refine_cells(g0, (np.abs(cc) < 5.0).all(axis=1))
    lay = M.DofLayout(mesh.n_nodes, 3, blocked=True)
    ch = M.hanging_constraints(mesh, lay)
    rng = np.random.default_rng(0)
    h = 20.0 / n / 2
    shear = 1e-2 * np.array([[0.9, 0.7, -0.3], [0.1, -0.8, 0.5], [0.4, -0.2, 0.2]])  # eigenvalues of both signs at every q-point
    u = mesh.coords @ shear.T + rng.uniform(-2e-4 * h, 2e-4 * h, (mesh.n_nodes, 3))
    sol = ch.distribute(lay.pack(u, rng.uniform(0.3, 0.9, mesh.n_nodes)))
    old = ch.distribute(lay.pack(0 * u, rng.uniform(0.3, 0.9, mesh.n_nodes)))
    prm = O.make_params(**{"lambda": 121.15}, mu=80.77, G_c=2.7, alpha_eps=2.0 * h, constant_k=1e-3, pressure=0.05, timestep=1e-3, time=2e-3,
                        old_timestep=1e-3, old_old_timestep=1e-3, timestep_number=1, decompose_stress_rhs=1.0, decompose_stress_matrix=1.0)
    asm = Assembler(mesh, blocked=True)
    asm.split_model = capi.SPLIT_SPECTRAL
    asm.allocate_matrix()
    asm.set_params(prm)
    asm.set_constraints(np.zeros(mesh.n_nodes, np.uint8))
    asm.set_vectors(sol, old, old)
    return asm, mesh, f"{n}^3 hexes with the inner half refined once, spectral split (model 1)"


def run(name, make, args):
    from cracks_amd import capi

    modes = {"default": capi.HANGING_MODE_DEFAULT, "gather": capi.HANGING_MODE_GATHER, "atomic": capi.HANGING_MODE_ATOMIC}
    arms = list(dict.fromkeys(args.modes))
    asm, mesh, what = make(args)
    only_default = arms == ["default"]  # (nothing is set then: an older build of the library runs as well)

    def configure(arm):
        if not only_default:
            asm.hanging_mode = modes[arm]

    def timed(arm, residual_only):
        configure(arm)
        for _ in range(args.warmup):
            asm.assemble_system(residual_only)
        asm.synchronize()
        asm.ctx.timing_enable(True)
        for _ in range(args.reps):
            asm.assemble_system(residual_only)
        asm.synchronize()
        ts = asm.ctx.kernel_times_ms()
        asm.ctx.timing_enable(False)
        assert ts.size == args.reps
        return ts

    rec = {"metric": "hanging_modes", "mesh": name, "workload": what, "cells": int(mesh.n_cells), "hanging_nodes": int(mesh.hn_nodes.size),
           "kernel_path": int(asm.ctx.kernel_path), "reps": args.reps, "rounds": args.rounds, "arms": arms}
    if not only_default:
        outs, info = {}, {}
        for arm in arms:
            configure(arm)
            asm.assemble_system(False)
            asm.synchronize()
            outs[arm] = [m.clone() for m in asm.system_pde_matrix] + [asm.system_pde_residual.clone()]
            info[arm] = asm.ctx.hanging_info()[1]
        rec["hanging_info"] = info
        if "gather" in outs and "default" in outs:
            rec["gather_deviation_from_default"] = max(float((a - b).abs().max() / max(1.0, float(b.abs().max())))
                                                       for a, b in zip(outs["gather"], outs["default"]))
        del outs
    for residual_only, tag in ((False, "jacobian"), (True, "residual_only")):
        ts = {arm: [] for arm in arms}
        for _ in range(args.rounds):
            for arm in arms:
                ts[arm].append(timed(arm, residual_only))
        rec[tag] = {}
        for arm in arms:
            allt = np.concatenate(ts[arm])
            rec[tag][arm] = {"ms": float(np.median(allt)), "min_ms": float(allt.min()), "round_medians_ms": [float(np.median(t)) for t in ts[arm]]}
        if "gather" in arms and "default" in arms:
            rec[tag]["gather_over_default"] = rec[tag]["gather"]["ms"] / rec[tag]["default"]["ms"]
    asm.ctx.close()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", choices=["config5", "block3d"], nargs="+", default=["config5", "block3d"])
    ap.add_argument("--modes", choices=["default", "gather", "atomic"], nargs="+", default=["default", "gather", "atomic"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the modes; the medians of all rounds are reported")
    ap.add_argument("--n", type=int, default=84, help="block3d: coarse cells per edge")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_hanging needs the GPU: nothing is measured without it")
    for name in args.mesh:
        run(name, {"config5": config5, "block3d": block3d}[name], args)


if __name__ == "__main__":
    main()
