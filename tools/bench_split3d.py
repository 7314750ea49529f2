#!/usr/bin/env python3
"""Time the 3-D stress splits (pfm_set_split_model: PFM_SPLIT_SPECTRAL, PFM_SPLIT_VOLDEV) next to the unsplit general family on
the same mesh, in one process:

  a --n^3 box (100^3 by default), the general family over all cells (the split assembly of a box context takes it by
  itself; the unsplit one is sent there with pfm_ctx_force_path(0)), Jacobian and residual-only assembly, the split off
  and on alternating round by round.

The state is a shear plus noise, so that the strain has eigenvalues of both signs at every q-point (the split does work
everywhere).  Kernel time from the library's own events around each assembly (pfm_timing_enable: zeroing of the outputs and
every colour class), median and minimum over --reps assemblies after --warmup.  The two results are compared with each other
where they must agree: in a second state of pure tension the split assembly reproduces the unsplit one.  One JSON line.

--model names the law (default: spectral, output as before).  With several models (--model spectral voldev) every round runs
the unsplit arm and one arm per model, alternating; the keys of a model's arm then carry its name instead of "split".

    python tools/bench_split3d.py [--n 100] [--reps 20] [--warmup 3] [--rounds 3] [--model {spectral,voldev} ...]

--route general lattice times something else: the residual-only assembly of PFM_SPLIT_VOLDEV on the box context itself, once per
route of pfm_set_split_route (general: the general family over all cells; lattice: k_cart_residual3<false, true>), next to
two yardstick arms with the split off -- "unsplit", what the context runs by itself (the polynomial row-owner kernels), and
"unsplit_qpoint", the q-point form k_cart_residual3<false> the law sits in (reached with a penalised monolithic scheme) --
all arms alternating round by round in one process.  The two routes are compared with each other on the timed state.

--route general lattice --model spectral does the same for PFM_SPLIT_SPECTRAL: "general" is route 0, the general family over all
cells, and "lattice" is PFM_SPLIT_ROUTE_LATTICE_ANY, k_cart_residual3<false, false, true>.  Same arms, alternation and JSON
keys, plus "model".  Without --model spectral the --route run times model 3 as before.

--jacobian --route general lattice --model voldev times the FULL assembly (Jacobian + residual_pde) of PFM_SPLIT_VOLDEV on the box
context: "general" is route 0 (the general family over all cells), "lattice" is PFM_SPLIT_ROUTE_LATTICE_JACOBIAN
(k_cart_split3_jac + k_cart_residual3<false, true>), on a state whose traces are of either sign (a deviatoric gradient plus
noise; the share of cells with a compressed q-point comes from pfm_ctx_split_route_info).  Next to them "lattice_tension", the
lattice route on a state of pure tension, and "unsplit", the full assembly with the split off (the pair k_cart_uu3 +
k_cart_phi4).  All arms alternate round by round in one process (--rounds 6 for a record).

--jacobian --overlay --route general lattice --model voldev does the same on a mesh with hanging nodes: the block-refined mesh of
bench.py's overlay_3d (the box of --n^3 hexes, 84 by default as there, with its inner half refined once), which the library runs
as a 3-D overlay (kernel path 3).  "general" is route 0 -- the parent's path, its code unchanged: the general family over all
cells with the full colour lists -- and "lattice" is PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS: the level form of
k_cart_split3_jac + k_cart_residual3<false, true> on the regular rows of both level lattices, the general family over the cells
that touch any other row.  "unsplit" is the unsplit overlay assembly of the same context (the yardstick).  The arms alternate
round by round in one process; the state is the deviatoric gradient plus noise, hanging nodes interpolated.

--jacobian --route lattice sparse --model voldev --compressed {tension,slab,half} times PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE
("sparse": k_cart_split3_mark, the unsplit k_cart_uu3 + k_cart_phi4, the sparse form of k_cart_split3_jac) next to its two
yardsticks on the same state -- "lattice", route 5, and "unsplit", the full assembly with the split off -- alternating round
by round in one process.  The states: "tension" (a dilation plus noise: no compressed cell), "slab" (the same with the node
planes z <= 5 h compressed: about 5 % of the cells of the default box) and "half" (the deviatoric gradient plus noise of the
run above: about half of the cells).  The record carries the compressed cells, the rows the split kernel recomputed, the
flagged tile-chunks and whether the sparse arm's round median is below route 5's in every round.

--jacobian --overlay --route general lattice sparse --model voldev --compressed {tension,slab,half} times
PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS_SPARSE ("sparse", route 61: per level the mark kernel, the unsplit level kernels and the
sparse level form of k_cart_split3_jac) on the block-refined mesh next to "lattice" (route 13), "general" (route 0, the parent's
path) and "unsplit" (the yardstick), all arms alternating round by round in one process.  The states: "tension" (a dilation plus
noise: no compressed cell), "slab" (the same with the node planes |z| <= 0.5 compressed, a slab through the refined block and
the coarse cells around it: about 5 % of the height) and "half" (the deviatoric gradient plus noise of the run above).  The
record carries the compressed cells, the recomputed rows, the flagged tile-chunks and whether the sparse arm's round median is
below the general arm's and below route 13's in every round.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=None, help="hexes per direction (default 100; with --overlay 84, bench.py's overlay_3d)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="off / on alternations; the medians of all rounds are reported")
    ap.add_argument("--layout", choices=["blocked", "interleaved"], default="blocked")
    ap.add_argument("--model", choices=["spectral", "voldev"], nargs="+", default=None, help="the split law(s) to time (default: spectral)")
    ap.add_argument("--route", choices=["general", "lattice", "sparse"], nargs="+", default=None,
                    help="time the residual-only assembly of model 3 (--model spectral: of model 1) per split route on the box context "
                         "instead (see above)")
    ap.add_argument("--jacobian", action="store_true", help="with --route: time the full assembly of model 3 per route (see above)")
    ap.add_argument("--overlay", action="store_true", help="with --jacobian: on the block-refined mesh of bench.py's overlay_3d (see above)")
    ap.add_argument("--compressed", choices=["tension", "slab", "half"], default=None,
                    help="with --jacobian --route lattice sparse: the state the sparse route is timed on (see above)")
    args = ap.parse_args()
    if ("sparse" in (args.route or [])) != (args.compressed is not None) or (args.compressed and not args.jacobian):
        raise SystemExit("--compressed goes with --jacobian [--overlay] --route lattice sparse --model voldev")
    if args.overlay and not args.jacobian:
        raise SystemExit("--overlay goes with --jacobian --route general lattice --model voldev")
    if args.n is None:
        args.n = 84 if args.overlay else 100
    if args.jacobian and (not args.route or (args.model or ["voldev"]) != ["voldev"]):
        raise SystemExit("--jacobian goes with --route general lattice and model voldev")
    route_spectral = bool(args.route) and args.model == ["spectral"]  # (--route without --model: model 3, as before)
    args.model = args.model or ["spectral"]

    import torch

    import oracle_api as O
    from cracks_amd import capi
    from cracks_amd import mesh as M
    from cracks_amd.assembler import Assembler

    if not torch.cuda.is_available():
        raise SystemExit("bench_split3d needs the GPU: nothing is measured without it")
    if args.overlay:
        return bench_jacobian_overlay(args, capi, M, Assembler, O)
    n = args.n
    mesh = M.box_mesh(3, n, lo=0.0, hi=float(n))
    blocked = args.layout == "blocked"
    lay = M.DofLayout(mesh.n_nodes, 3, blocked=blocked)
    rng = np.random.default_rng(0)
    shear = 1e-2 * np.array([[0.9, 0.7, -0.3], [0.1, -0.8, 0.5], [0.4, -0.2, 0.2]])
    noise = rng.uniform(-2e-4, 2e-4, (mesh.n_nodes, 3))
    phi = rng.uniform(0.3, 0.9, mesh.n_nodes)
    sol = lay.pack(mesh.coords @ shear.T + noise, phi)
    tension = lay.pack(1e-2 * mesh.coords + noise, phi)
    old = lay.pack(np.zeros((mesh.n_nodes, 3)), rng.uniform(0.3, 0.9, mesh.n_nodes))
    base = dict(mu=80.77, G_c=2.7, alpha_eps=0.5, constant_k=1e-3, pressure=0.05, timestep=1e-3, time=2e-3, old_timestep=1e-3,
                old_old_timestep=1e-3, timestep_number=1)
    prm_off = O.make_params(**{"lambda": 121.15}, **base)
    prm_on = O.make_params(**{"lambda": 121.15}, decompose_stress_rhs=1.0, decompose_stress_matrix=1.0, **base)

    asm = Assembler(mesh, blocked)
    assert asm.ctx.kernel_path == 1
    models = {"spectral": capi.SPLIT_SPECTRAL, "voldev": capi.SPLIT_VOLDEV}
    arms = list(dict.fromkeys(args.model))  # None below: the unsplit arm
    asm.split_model = models[arms[0]]
    asm.set_constraints(np.zeros(mesh.n_nodes, np.uint8))
    asm.set_vectors(sol, old, old)
    asm.allocate_matrix()

    if args.jacobian:
        dev_grad = 1e-2 * np.array([[0.9, 0.7, -0.3], [0.1, -0.8, 0.5], [0.4, -0.2, -0.1]])  # trace 0: the noise decides the sign
        mixed = lay.pack(mesh.coords @ dev_grad.T + noise, phi)
        if args.compressed:
            u = 1e-2 * mesh.coords + noise
            low = mesh.coords[:, 2] <= 5.0  # unit cells: the five cell layers below z = 5 are compressed by 1e-2
            u[low] -= 2e-2 * mesh.coords[low]
            state = {"tension": tension, "slab": lay.pack(u, phi), "half": mixed}[args.compressed]
            return bench_jacobian_sparse(args, asm, capi, mesh, prm_off, prm_on, state, old)
        return bench_jacobian(args, asm, capi, mesh, prm_off, prm_on, {"mixed": mixed, "tension": tension}, old)
    if args.route:
        return bench_routes(args, asm, capi, mesh, prm_off, prm_on, O.make_params(**{"lambda": 121.15}, outer_solver=1, gamma_penal=1e-2, **base),
                            route_spectral)

    def configure(split):
        # the unsplit assembly through the general family as well (the box's own kernels are not the yardstick here)
        asm.ctx.force_path(0)
        if split:
            asm.split_model = models[split]
        asm.set_params(prm_on if split else prm_off)

    def timed(split, residual_only):
        configure(split)
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

    # agreement where the two must agree: pure tension
    asm.set_vectors(tension, old, old)
    outs = []
    for split in [None] + arms:
        configure(split)
        asm.assemble_system(False)
        asm.synchronize()
        outs.append(([m.clone() for m in asm.system_pde_matrix], asm.system_pde_residual.clone()))
    dev = max(float((a - b).abs().max() / max(1.0, float(b.abs().max()))) for o in outs[1:] for a, b in zip(o[0] + [o[1]], outs[0][0] + [outs[0][1]]))
    del outs
    asm.set_vectors(sol, old, old)

    rec = {"metric": "split3d_general_family", "cells": int(mesh.n_cells), "layout": args.layout, "reps": args.reps, "rounds": args.rounds,
           "pure_tension_deviation_from_unsplit": dev}
    if arms != ["spectral"]:
        rec["models"] = arms
    for residual_only, tag in ((False, "jacobian"), (True, "residual_only")):
        ts = {split: [] for split in [None] + arms}
        for _ in range(args.rounds):
            for split in [None] + arms:
                ts[split].append(timed(split, residual_only))
        off = np.concatenate(ts[None])
        rec[tag] = {"unsplit_ms": float(np.median(off)), "unsplit_min_ms": float(off.min()),
                    "unsplit_round_medians_ms": [float(np.median(t)) for t in ts[None]]}
        for m in arms:
            on, key = np.concatenate(ts[m]), ("split" if len(arms) == 1 else m)
            rec[tag].update({f"{key}_ms": float(np.median(on)), f"{key}_min_ms": float(on.min()),
                             f"{key}_round_medians_ms": [float(np.median(t)) for t in ts[m]],
                             ("ratio" if len(arms) == 1 else f"{key}_ratio"): float(np.median(on) / np.median(off))})
        rec[tag]["unsplit_ms_per_1e6_cells"] = float(np.median(off) * 1e6 / mesh.n_cells)
        for m in arms:
            key = "split" if len(arms) == 1 else m
            rec[tag][f"{key}_ms_per_1e6_cells"] = float(np.median(np.concatenate(ts[m])) * 1e6 / mesh.n_cells)
    print(json.dumps(rec))


def bench_routes(args, asm, capi, mesh, prm_off, prm_on, prm_qpoint, spectral=False):
    """--route: residual-only arms on the box context (kernel path 1), alternating round by round"""
    routes = {"general": capi.SPLIT_ROUTE_GENERAL, "lattice": capi.SPLIT_ROUTE_LATTICE_ANY if spectral else capi.SPLIT_ROUTE_LATTICE}
    arms = list(dict.fromkeys(args.route)) + ["unsplit", "unsplit_qpoint"]
    asm.split_model = capi.SPLIT_SPECTRAL if spectral else capi.SPLIT_VOLDEV

    def configure(arm):
        asm.split_route = routes.get(arm, capi.SPLIT_ROUTE_GENERAL)
        asm.set_params(prm_on if arm in routes else prm_qpoint if arm == "unsplit_qpoint" else prm_off)
        assert asm.ctx.kernel_path == 1 and asm.ctx.split_route_info()[1] == int(arm == "lattice")

    def timed(arm):
        configure(arm)
        for _ in range(args.warmup):
            asm.assemble_system(True)
        asm.synchronize()
        asm.ctx.timing_enable(True)
        for _ in range(args.reps):
            asm.assemble_system(True)
        asm.synchronize()
        ts = asm.ctx.kernel_times_ms()
        asm.ctx.timing_enable(False)
        assert ts.size == args.reps
        return ts

    outs = {}
    for arm in [a for a in arms if a in routes]:
        configure(arm)
        asm.assemble_system(True)
        asm.synchronize()
        outs[arm] = (asm.system_pde_residual.clone(), asm.system_total_residual.clone())
    rec = {"metric": "split3d_routes_residual_only", "cells": int(mesh.n_cells), "layout": args.layout, "reps": args.reps, "rounds": args.rounds,
           "arms": arms}
    if spectral:
        rec["model"] = "spectral"
    if len(outs) == 2:
        rec["lattice_deviation_from_general"] = max(float((a - b).abs().max() / max(1.0, float(b.abs().max())))
                                                    for a, b in zip(outs["lattice"], outs["general"]))
    ts = {arm: [] for arm in arms}
    for _ in range(args.rounds):
        for arm in arms:
            ts[arm].append(timed(arm))
    med = {arm: float(np.median(np.concatenate(ts[arm]))) for arm in arms}
    for arm in arms:
        rec[arm] = {"ms": med[arm], "min_ms": float(np.concatenate(ts[arm]).min()), "round_medians_ms": [float(np.median(t)) for t in ts[arm]],
                    "ms_per_1e6_cells": med[arm] * 1e6 / mesh.n_cells}
    if "lattice" in med:
        rec["lattice_over_unsplit"] = med["lattice"] / med["unsplit"]
        rec["lattice_over_unsplit_qpoint"] = med["lattice"] / med["unsplit_qpoint"]
    if "lattice" in med and "general" in med:
        rec["lattice_over_general"] = med["lattice"] / med["general"]
        rec["lattice_below_general_in_every_round"] = all(np.median(l) < np.median(g) for l, g in zip(ts["lattice"], ts["general"]))
    print(json.dumps(rec))


def bench_jacobian(args, asm, capi, mesh, prm_off, prm_on, states, old):
    """--jacobian: full-assembly arms on the box context (kernel path 1), alternating round by round"""
    routes = {"general": capi.SPLIT_ROUTE_GENERAL, "lattice": capi.SPLIT_ROUTE_LATTICE_JACOBIAN, "lattice_tension": capi.SPLIT_ROUTE_LATTICE_JACOBIAN}
    arms = list(dict.fromkeys(args.route)) + ["lattice_tension", "unsplit"]
    asm.split_model = capi.SPLIT_VOLDEV
    current = [None]

    def configure(arm):
        state = "tension" if arm == "lattice_tension" else "mixed"
        if current[0] != state:
            asm.set_vectors(states[state], old, old)
            current[0] = state
        asm.split_route = routes.get(arm, capi.SPLIT_ROUTE_GENERAL)
        asm.set_params(prm_on if arm in routes else prm_off)
        assert asm.ctx.kernel_path == 1 and asm.ctx.split_route_plan()[2] == int(arm.startswith("lattice"))

    def timed(arm):
        configure(arm)
        for _ in range(args.warmup):
            asm.assemble_system(False)
        asm.synchronize()
        asm.ctx.timing_enable(True)
        for _ in range(args.reps):
            asm.assemble_system(False)
        asm.synchronize()
        ts = asm.ctx.kernel_times_ms()
        asm.ctx.timing_enable(False)
        assert ts.size == args.reps
        return ts

    outs, compressed = {}, {}
    for arm in [a for a in arms if a in routes]:
        configure(arm)
        asm.assemble_system(False)
        asm.synchronize()
        compressed[arm] = asm.ctx.split_route_plan()[3]
        if arm in ("general", "lattice"):
            outs[arm] = [m.clone() for m in asm.system_pde_matrix] + [asm.system_pde_residual.clone()]
    rec = {"metric": "split3d_routes_jacobian", "cells": int(mesh.n_cells), "layout": args.layout, "reps": args.reps, "rounds": args.rounds,
           "arms": arms, "cells_with_a_compressed_q_point": {k: v for k, v in compressed.items() if v >= 0}}
    if len(outs) == 2:
        rec["lattice_deviation_from_general"] = max(float((a - b).abs().max() / max(1.0, float(b.abs().max())))
                                                    for a, b in zip(outs["lattice"], outs["general"]))
    del outs
    ts = {arm: [] for arm in arms}
    for _ in range(args.rounds):
        for arm in arms:
            ts[arm].append(timed(arm))
    med = {arm: float(np.median(np.concatenate(ts[arm]))) for arm in arms}
    for arm in arms:
        rec[arm] = {"ms": med[arm], "min_ms": float(np.concatenate(ts[arm]).min()), "round_medians_ms": [float(np.median(t)) for t in ts[arm]],
                    "ms_per_1e6_cells": med[arm] * 1e6 / mesh.n_cells}
    if "lattice" in med:
        rec["lattice_over_unsplit"] = med["lattice"] / med["unsplit"]
        rec["lattice_tension_over_unsplit"] = med["lattice_tension"] / med["unsplit"]
    if "lattice" in med and "general" in med:
        rec["lattice_over_general"] = med["lattice"] / med["general"]
        rec["lattice_below_general_in_every_round"] = all(np.median(l) < np.median(g) for l, g in zip(ts["lattice"], ts["general"]))
    print(json.dumps(rec))


def bench_jacobian_sparse(args, asm, capi, mesh, prm_off, prm_on, state, old):
    """--jacobian --route lattice sparse --compressed: route 21 next to route 5 and the unsplit assembly on one state"""
    routes = {"lattice": capi.SPLIT_ROUTE_LATTICE_JACOBIAN, "sparse": capi.SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE}
    arms = ["lattice", "sparse", "unsplit"]
    asm.split_model = capi.SPLIT_VOLDEV
    asm.set_vectors(state, old, old)

    def configure(arm):
        asm.split_route = routes.get(arm, capi.SPLIT_ROUTE_GENERAL)
        asm.set_params(prm_on if arm in routes else prm_off)
        assert asm.ctx.kernel_path == 1 and asm.ctx.split_route_plan()[2] == int(arm in routes) and asm.ctx.split_sparse_info()[0] == int(arm == "sparse")

    def timed(arm):
        configure(arm)
        for _ in range(args.warmup):
            asm.assemble_system(False)
        asm.synchronize()
        asm.ctx.timing_enable(True)
        for _ in range(args.reps):
            asm.assemble_system(False)
        asm.synchronize()
        ts = asm.ctx.kernel_times_ms()
        asm.ctx.timing_enable(False)
        assert ts.size == args.reps
        return ts

    outs, compressed = {}, {}
    for arm in routes:
        configure(arm)
        asm.assemble_system(False)
        asm.synchronize()
        compressed[arm] = asm.ctx.split_route_plan()[3]
        outs[arm] = [m.clone() for m in asm.system_pde_matrix] + [asm.system_pde_residual.clone()]
    info = asm.ctx.split_sparse_info()
    rec = {"metric": "split3d_routes_jacobian_sparse", "state": args.compressed, "cells": int(mesh.n_cells), "nodes": int(mesh.n_nodes),
           "layout": args.layout, "reps": args.reps, "rounds": args.rounds, "arms": arms, "cells_with_a_compressed_q_point": compressed,
           "compressed_cell_fraction": compressed["sparse"] / mesh.n_cells, "rows_recomputed": info[1], "rows_recomputed_fraction": info[1] / mesh.n_nodes,
           "tile_chunks_flagged": info[2], "tile_chunks": info[3],
           "sparse_deviation_from_lattice": max(float((a - b).abs().max() / max(1.0, float(b.abs().max()))) for a, b in zip(outs["sparse"], outs["lattice"])),
           "residual_pde_same_bytes": bool(torch_equal(outs["sparse"][-1], outs["lattice"][-1]))}
    del outs
    ts = {arm: [] for arm in arms}
    for _ in range(args.rounds):
        for arm in arms:
            ts[arm].append(timed(arm))
    med = {arm: float(np.median(np.concatenate(ts[arm]))) for arm in arms}
    for arm in arms:
        rec[arm] = {"ms": med[arm], "min_ms": float(np.concatenate(ts[arm]).min()), "round_medians_ms": [float(np.median(t)) for t in ts[arm]],
                    "ms_per_1e6_cells": med[arm] * 1e6 / mesh.n_cells}
    rec["sparse_over_lattice"] = med["sparse"] / med["lattice"]
    rec["sparse_over_unsplit"] = med["sparse"] / med["unsplit"]
    rec["lattice_over_unsplit"] = med["lattice"] / med["unsplit"]
    rec["sparse_below_lattice_in_every_round"] = all(np.median(a) < np.median(b) for a, b in zip(ts["sparse"], ts["lattice"]))
    print(json.dumps(rec))


def torch_equal(a, b):
    import torch

    return torch.equal(a, b)


def bench_jacobian_overlay(args, capi, M, Assembler, O):
    """--jacobian --overlay: full-assembly arms on the overlay context (kernel path 3), alternating round by round"""
    n = args.n
    g0 = M.box_mesh(3, (n,) * 3)  # bench.py: overlay_3d
    cc = g0.coords[g0.cells].mean(axis=1)
    mesh = M.refine_cells(g0, (np.abs(cc) < 5.0).all(axis=1))
    blocked = args.layout == "blocked"
    lay = M.DofLayout(mesh.n_nodes, 3, blocked=blocked)
    ch = M.hanging_constraints(mesh, lay)
    rng = np.random.default_rng(0)
    h = 20.0 / n / 2  # the edge of a refined cell
    dev_grad = 1e-2 * np.array([[0.9, 0.7, -0.3], [0.1, -0.8, 0.5], [0.4, -0.2, -0.1]])  # trace 0: the noise decides the sign
    noise = rng.uniform(-2e-4 * h, 2e-4 * h, (mesh.n_nodes, 3))
    phi = rng.uniform(0.3, 0.9, mesh.n_nodes)
    sol = ch.distribute(lay.pack(mesh.coords @ dev_grad.T + noise, phi))
    if args.compressed in ("tension", "slab"):
        u = 1e-2 * mesh.coords + noise
        if args.compressed == "slab":  # the cells between the node planes |z| <= 0.5 are compressed by 1e-2, those across its faces stretched
            low = np.abs(mesh.coords[:, 2]) <= 0.5
            u[low] -= 2e-2 * mesh.coords[low]
        sol = ch.distribute(lay.pack(u, phi))
    old = ch.distribute(lay.pack(np.zeros((mesh.n_nodes, 3)), rng.uniform(0.3, 0.9, mesh.n_nodes)))
    base = dict(mu=80.77, G_c=2.7, alpha_eps=0.5, constant_k=1e-3, pressure=0.05, timestep=1e-3, time=2e-3, old_timestep=1e-3,
                old_old_timestep=1e-3, timestep_number=1)
    prm_off = O.make_params(**{"lambda": 121.15}, **base)
    prm_on = O.make_params(**{"lambda": 121.15}, decompose_stress_rhs=1.0, decompose_stress_matrix=1.0, **base)
    asm = Assembler(mesh, blocked)
    asm.split_model = capi.SPLIT_VOLDEV
    asm.set_constraints(np.zeros(mesh.n_nodes, np.uint8))
    asm.set_vectors(sol, old, old)
    asm.allocate_matrix()
    rows, general_cells = asm.ctx.overlay_info()
    assert asm.ctx.kernel_path == 3 and rows > 0
    routes = {"general": capi.SPLIT_ROUTE_GENERAL, "lattice": capi.SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS,
              "sparse": capi.SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS_SPARSE}
    arms = list(dict.fromkeys(args.route)) + ["unsplit"]

    def configure(arm):
        asm.split_route = routes.get(arm, capi.SPLIT_ROUTE_GENERAL)
        asm.set_params(prm_on if arm in routes else prm_off)
        assert asm.ctx.kernel_path == 3 and asm.ctx.split_route_plan()[2] == int(arm in ("lattice", "sparse"))
        assert asm.ctx.split_sparse_info()[0] == int(arm == "sparse")

    def timed(arm):
        configure(arm)
        for _ in range(args.warmup):
            asm.assemble_system(False)
        asm.synchronize()
        asm.ctx.timing_enable(True)
        for _ in range(args.reps):
            asm.assemble_system(False)
        asm.synchronize()
        ts = asm.ctx.kernel_times_ms()
        asm.ctx.timing_enable(False)
        assert ts.size == args.reps
        return ts

    outs, compressed = {}, {}
    for arm in [a for a in arms if a in routes]:
        configure(arm)
        asm.assemble_system(False)
        asm.synchronize()
        compressed[arm] = asm.ctx.split_route_plan()[3]
        if arm == "sparse":
            info = asm.ctx.split_sparse_info()
        outs[arm] = [m.clone() for m in asm.system_pde_matrix] + [asm.system_pde_residual.clone()]
    rec = {"metric": "split3d_routes_jacobian_overlay", "cells": int(mesh.n_cells), "nodes": int(mesh.n_nodes), "hanging_nodes": int(mesh.hn_nodes.size),
           "regular_rows": int(rows), "regular_row_fraction": rows / mesh.n_nodes, "cells_left_to_the_general_family": int(general_cells),
           "layout": args.layout, "reps": args.reps, "rounds": args.rounds, "arms": arms,
           "cells_with_a_compressed_q_point_among_those_of_the_level_kernels": {k: v for k, v in compressed.items() if v >= 0}}
    if "lattice" in outs and "general" in outs:
        rec["lattice_deviation_from_general"] = max(float((a - b).abs().max() / max(1.0, float(b.abs().max())))
                                                    for a, b in zip(outs["lattice"], outs["general"]))
    if "sparse" in outs:
        rec.update({"state": args.compressed, "compressed_cell_fraction_of_the_level_kernels": compressed["sparse"] / mesh.n_cells, "rows_recomputed": info[1],
                    "rows_recomputed_fraction_of_the_regular_rows": info[1] / rows, "tile_chunks_flagged": info[2], "tile_chunks": info[3]})
        for other in ("lattice", "general"):
            if other in outs:
                rec[f"sparse_deviation_from_{other}"] = max(float((a - b).abs().max() / max(1.0, float(b.abs().max())))
                                                            for a, b in zip(outs["sparse"], outs[other]))
        if "lattice" in outs:
            rec["residual_pde_same_bytes_as_lattice"] = bool(torch_equal(outs["sparse"][-1], outs["lattice"][-1]))
    del outs
    ts = {arm: [] for arm in arms}
    for _ in range(args.rounds):
        for arm in arms:
            ts[arm].append(timed(arm))
    med = {arm: float(np.median(np.concatenate(ts[arm]))) for arm in arms}
    for arm in arms:
        rec[arm] = {"ms": med[arm], "min_ms": float(np.concatenate(ts[arm]).min()), "round_medians_ms": [float(np.median(t)) for t in ts[arm]],
                    "ms_per_1e6_cells": med[arm] * 1e6 / mesh.n_cells}
    if "sparse" in med:
        rec["sparse_over_unsplit"] = med["sparse"] / med["unsplit"]
        for other in ("lattice", "general"):
            if other in med:
                rec[f"sparse_over_{other}"] = med["sparse"] / med[other]
                rec[f"sparse_below_{other}_in_every_round"] = all(np.median(a) < np.median(b) for a, b in zip(ts["sparse"], ts[other]))
    if "lattice" in med:
        rec["lattice_over_unsplit"] = med["lattice"] / med["unsplit"]
    if "lattice" in med and "general" in med:
        rec["lattice_over_general"] = med["lattice"] / med["general"]
        rec["lattice_below_general_in_every_round"] = all(np.median(l) < np.median(g) for l, g in zip(ts["lattice"], ts["general"]))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
