#!/usr/bin/env python3
"""Time the mesh-adaptation entries of include/pfm_newton.h next to what a host pays for the same sweep today (the
device-to-host copy of the vector(s) plus the numpy statement of cracks_amd/adapt.py):

  pfm_refine_flags     on the 3-D Sneddon box (216^3 cells by default) and on a 2-D box (1000^2)
  pfm_state_transfer   of three vectors from the base box of bench.py's `overlay_3d` (84^3 hexes) to its block-refined
                       1.1e6-hex mesh
  pfm_kelly_indicator  on the 3-D box and on that block-refined mesh: the first call (which builds the face-neighbour table)
                       and later calls apart
  pfm_indicator_select among the 1e7 indicators of the 3-D box
  pfm_refine_flags_mix on the 3-D box (flags + Kelly + selection + marking)

Next to the Kelly and mix items: the host path (copy of the solution to the host at the full size plus the numpy statement on
a --host-n^3 box, a size numpy can do; both sizes are in the record), and the achieved share of the HBM peak (--hbm-peak,
8 TB/s) under the bytes model written next to each item.

Wall clock around each call with the device idle before and after (the flags call is synchronous, the transfer is
followed by a synchronisation), median and minimum of --reps calls.  Prints one JSON line.

    python tools/bench_adapt.py [--n3 216] [--n2 1000] [--nt 84] [--reps 20] [--host-n 40]
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
    ap.add_argument("--host-n", type=int, default=40, help="cells per axis of the box the numpy Kelly statement is timed on")
    ap.add_argument("--hbm-peak", type=float, default=8.0e12, help="bytes per second the shares are quoted against")
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

    out = {"metric": "mesh_adaptation", "reps": args.reps, "host_reps": args.host_reps, "hbm_peak_bytes_per_s": args.hbm_peak}

    def smooth_state(mesh, lay, phi):
        x = mesh.coords
        u = np.stack([np.sin(0.7 * x[:, d] + 0.3 * x[:, (d + 1) % mesh.dim]) for d in range(mesh.dim)], axis=1)
        return lay.pack(u, phi)

    def share(bytes_moved, ms):
        return bytes_moved / (1e-3 * ms) / args.hbm_peak

    def kelly_items(ctx, mesh, first_ms):
        """pfm_kelly_indicator on a context whose state is set.  Bytes model per cell: the cell's row of the cell table
        (nv int32), its 2 dim neighbour entries (int32 + relation byte), the coordinates and displacements of one node (on
        these meshes there are about as many nodes as cells and every node is fetched from HBM once: 2 dim doubles), 8 out."""
        dim, nv = mesh.dim, mesh.nv
        eta = torch.empty(mesh.n_cells, dtype=torch.float64, device="cuda")
        model = mesh.n_cells * (4 * nv + 2 * dim * 5 + 8) + mesh.n_nodes * 2 * dim * 8
        rec = {"cells": int(mesh.n_cells), "first_call_with_table_build_ms": first_ms,
               "device": timed(lambda: ctx.kelly_indicator(eta.data_ptr()), args.reps), "bytes_model": int(model)}
        rec["hbm_share"] = share(model, rec["device"]["ms"])
        return rec, eta

    def first_kelly(ctx, n_cells):
        eta = torch.empty(n_cells, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.kelly_indicator(eta.data_ptr())
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    # the numpy statement of the Kelly indicator and of mix, on a box numpy can do
    hm = M.box_mesh(3, args.host_n)
    hl = M.DofLayout(hm.n_nodes, 3, blocked=True)
    h_state = smooth_state(hm, hl, 0.5 + 0.5 * np.tanh(4.0 * (np.abs(hm.coords[:, 1]) - 0.5)))
    h_level = np.zeros(hm.n_cells, np.uint8)
    t0 = time.perf_counter()
    A.kelly_numpy(hm, A.nodal_values(hm, hl, h_state))
    host_kelly_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    A.refine_flags_mix_numpy(hm, A.nodal_values(hm, hl, h_state), 0.3, phi_threshold=0.8, max_level=1, cell_level=h_level)
    host_mix_ms = 1e3 * (time.perf_counter() - t0)
    host_numpy = {"cells": int(hm.n_cells), "kelly_numpy_ms": host_kelly_ms, "refine_flags_mix_numpy_ms": host_mix_ms}
    del hm, h_state

    # ---- flags: phi falls below the threshold in a slab around y = 0 (the crack band of the Sneddon set-up)
    for tag, dim, n in (("flags_3d", 3, args.n3), ("flags_2d", 2, args.n2)):
        mesh = M.box_mesh(dim, n)
        lay = M.DofLayout(mesh.n_nodes, dim, blocked=True)
        phi = 0.5 + 0.5 * np.tanh(4.0 * (np.abs(mesh.coords[:, 1]) - 0.5))
        sol = smooth_state(mesh, lay, phi)  # (the flags only read phi)
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
        if dim == 3:
            copy_ms = rec["host_copy_only"]["ms"]
            first_ms = first_kelly(ctx, mesh.n_cells)
            krec, eta = kelly_items(ctx, mesh, first_ms)
            # the host path: the copy at this size, the numpy statement at the size it can do (not scaled)
            krec["host"] = dict(host_numpy, copy_cells=int(mesh.n_cells), copy_ms=copy_ms)
            out["kelly_3d"] = krec
            ref = eta.cpu().numpy()
            k = int(0.3 * mesh.n_cells)
            t, above, equal = ctx.indicator_select(eta.data_ptr(), k)
            assert (t, above, equal) == A.indicator_select_numpy(ref, k)
            srec = {"entries": int(mesh.n_cells), "k": k, "device": timed(lambda: ctx.indicator_select(eta.data_ptr(), k), args.reps),
                    "bytes_model": int(9 * 8 * mesh.n_cells)}  # eight histogram passes and the count, 8 bytes per entry each
            srec["hbm_share"] = share(srec["bytes_model"], srec["device"]["ms"])

            def host_select():
                A.indicator_select_numpy(eta.cpu().numpy(), k)

            srec["host_copy_plus_numpy"] = timed(host_select, args.host_reps)
            out["select_3d"] = srec
            mix = lambda: ctx.refine_flags_mix(0.3, **crit)
            mflags, m_n, m_t = mix()
            want = ref.copy()
            want[A.refine_flags_numpy(mesh, phi, 0.8)[0].astype(bool)] = 0.0
            assert m_t == A.indicator_select_numpy(want, k)[0] and m_n == int((mflags != 0).sum())
            mrec = {"cells": int(mesh.n_cells), "flagged": int(m_n), "threshold": m_t, "device": timed(mix, args.reps),
                    "bytes_model": int(krec["bytes_model"] + srec["bytes_model"] + mesh.n_cells * (4 * mesh.nv + 8 * mesh.nv + 20))}
            # + the flags sweep (cell row, phi of its vertices), zeroing and marking (eta twice, the flag bytes)
            mrec["hbm_share"] = share(mrec["bytes_model"], mrec["device"]["ms"])
            mrec["host"] = dict(host_numpy, copy_cells=int(mesh.n_cells), copy_ms=copy_ms)
            out["mix_3d"] = mrec
            del eta, ref, want
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

    # ---- Kelly indicator across hanging faces: the block-refined mesh of the transfer
    sol = smooth_state(tl.mesh, lay_d, np.ones(tl.mesh.n_nodes))
    dst_ctx.state_set_host(sol, sol, sol)
    first_ms = first_kelly(dst_ctx, tl.mesh.n_cells)
    krec, eta = kelly_items(dst_ctx, tl.mesh, first_ms)
    krec["hanging_nodes"] = int(tl.mesh.hn_nodes.size)
    d_sol = torch.from_numpy(sol).cuda()
    krec["host"] = dict(host_numpy, copy_cells=int(tl.mesh.n_cells), copy_ms=timed(lambda: d_sol.cpu(), args.host_reps)["ms"])
    out["kelly_refined_block"] = krec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
