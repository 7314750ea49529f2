#!/usr/bin/env python3
"""Time the mesh-adaptation entries of include/pfm_newton.h next to what a host pays for the same sweep today (the
device-to-host copy of the vector(s) plus the numpy statement of cracks_amd/adapt.py):

  pfm_refine_flags     on the 3-D Sneddon box (216^3 cells by default) and on a 2-D box (1000^2)
  pfm_state_transfer   of three vectors from the base box of bench.py's `overlay_3d` (84^3 hexes) to its block-refined
                       1.1e6-hex mesh

Wall clock around each call with the device idle before and after (the flags call is synchronous, the transfer is
followed by a synchronisation), median and minimum of --reps calls.  Prints one JSON line.

    python tools/bench_adapt.py [--n3 216] [--n2 1000] [--nt 84] [--reps 20]
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
    ap.add_argument("--n3", type=int, default=216)
    ap.add_argument("--n2", type=int, default=1000)
    ap.add_argument("--nt", type=int, default=84, help="cells per axis of the transfer's base box")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    args = ap.parse_args()

    import torch

    from cracks_amd import adapt as A
    from cracks_amd import mesh as M
    from cracks_amd.assembler import Context

    def timed(fn, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return {"ms": float(np.median(ts)), "min_ms": float(np.min(ts))}

    out = {"metric": "mesh_adaptation", "reps": args.reps, "host_reps": args.host_reps}

    # ---- flags: phi falls below the threshold in a slab around y = 0 (the crack band of the Sneddon set-up)
    for tag, dim, n in (("flags_3d", 3, args.n3), ("flags_2d", 2, args.n2)):
        mesh = M.box_mesh(dim, n)
        lay = M.DofLayout(mesh.n_nodes, dim, blocked=True)
        phi = 0.5 + 0.5 * np.tanh(4.0 * (np.abs(mesh.coords[:, 1]) - 0.5))
        sol = lay.pack(np.zeros((mesh.n_nodes, dim)), phi)
        ctx = Context(mesh, True)
        ctx.state_set_host(sol, sol, sol)
        d_sol = torch.from_numpy(sol).cuda()
        level = np.zeros(mesh.n_cells, np.uint8)
        crit = dict(phi_threshold=0.8, max_level=1, cell_level=level)
        flags, n_flagged = ctx.refine_flags(**crit)  # warm-up (module load, scratch)
        want, n_want = A.refine_flags_numpy(mesh, phi, **crit)
        assert np.array_equal(flags, want) and n_flagged == n_want
        rec = {"cells": int(mesh.n_cells), "nodes": int(mesh.n_nodes), "flagged": int(n_flagged),
               "device": timed(lambda: ctx.refine_flags(**crit), args.reps)}
        h_sol = np.empty_like(sol)

        def host():
            h_sol[:] = d_sol.cpu().numpy()
            A.refine_flags_numpy(mesh, h_sol[lay.dof(np.arange(mesh.n_nodes), dim)], **crit)

        rec["host_copy_plus_numpy"] = timed(host, args.host_reps)
        rec["host_copy_only"] = timed(lambda: d_sol.cpu(), args.host_reps)
        rec["device_min_diameter"] = timed(lambda: ctx.min_cell_diameter(), args.reps)
        rec["ratio_host_over_device"] = rec["host_copy_plus_numpy"]["ms"] / rec["device"]["ms"]
        out[tag] = rec
        ctx.close()
        del ctx, d_sol, mesh, sol

    # ---- transfer of solution, old_solution, old_old_solution across the refinement of the inner half of the box
    base = M.box_mesh(3, (args.nt,) * 3)
    cc = base.coords[base.cells].mean(axis=1)
    tl = A.two_level_mesh(base, (np.abs(cc) < 5.0).all(axis=1))
    lay_s, lay_d = M.DofLayout(base.n_nodes, 3, True), M.DofLayout(tl.mesh.n_nodes, 3, True)
    rng = np.random.default_rng(0)
    vecs = [rng.standard_normal(lay_s.n_dofs) for _ in range(3)]
    src_ctx, dst_ctx = Context(base, True), Context(tl.mesh, True)
    d_src = [torch.from_numpy(v).cuda() for v in vecs]
    d_dst = [torch.full((lay_d.n_dofs,), float("nan"), dtype=torch.float64, device="cuda") for _ in vecs]
    sp, dp = [t.data_ptr() for t in d_src], [t.data_ptr() for t in d_dst]
    src_ctx.transfer_state(dst_ctx, tl.parent_cell, tl.child, sp, dp)  # warm-up
    torch.cuda.synchronize()
    want = A.transfer_numpy(base, tl.mesh, True, tl.parent_cell, tl.child, vecs)
    assert all(t.cpu().numpy().tobytes() == w.tobytes() for t, w in zip(d_dst, want))
    rec = {"src_cells": int(base.n_cells), "dst_cells": int(tl.mesh.n_cells), "dst_nodes": int(tl.mesh.n_nodes), "vectors": 3,
           "device": timed(lambda: src_ctx.transfer_state(dst_ctx, tl.parent_cell, tl.child, sp, dp), args.reps)}

    def host_transfer():
        hv = [t.cpu().numpy() for t in d_src]
        A.transfer_numpy(base, tl.mesh, True, tl.parent_cell, tl.child, hv)

    def host_round_trip():
        hv = [t.cpu().numpy() for t in d_src]
        res = A.transfer_numpy(base, tl.mesh, True, tl.parent_cell, tl.child, hv)
        for t, r in zip(d_dst, res):
            t.copy_(torch.from_numpy(r))

    rec["host_copy_plus_numpy"] = timed(host_transfer, args.host_reps)
    rec["host_copy_numpy_and_upload"] = timed(host_round_trip, args.host_reps)
    rec["ratio_host_over_device"] = rec["host_copy_plus_numpy"]["ms"] / rec["device"]["ms"]
    out["transfer_3d"] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
