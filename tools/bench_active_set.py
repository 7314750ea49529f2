#!/usr/bin/env python3
"""Time the active-set update of a partitioned mesh with hanging nodes (cracks.cc:2826-2890) at the size of the config-5
stand-in (the mesh of ``extra.config5_standin`` in bench.py), cut into --world contexts on ONE GPU, per rank:

  (a) device     the protocol of ``pfm_active_set_exchange`` from its pieces: ``active_set_owned_device`` (synchronous: the
                 counts) + ``state_set_solution_device`` + ``halo_pack_all`` + ``halo_pack_flags_all``, then -- after the
                 transport -- ``halo_unpack_all`` + ``halo_unpack_flags_all`` + ``distribute_hanging_device``.  The transport
                 between the contexts is an in-process device copy, NOT RCCL; it is timed on its own (all ranks together) and
                 not part of (a).
  (b) host       the round trip the protocol replaces, without the host's own work (the predicate on the host, the MPI
                 exchange of the flags): solution and residual_total device -> host, ``pfm_get_constraints``,
                 ``pfm_set_constraints``, solution host -> device.

Wall time around each form with one synchronisation at its end, --reps repetitions from the same state, reported as median
and min - max per rank.  Prints one JSON line.

    python tools/bench_active_set.py [--levels 8] [--world 4] [--reps 9]
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

C_CONST = 10.0


def stats(ts):
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, default=8)
    ap.add_argument("--world", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()

    import torch

    import bench
    from cracks_amd import partition as P
    from cracks_amd.assembler import Context

    pb = bench.config5_problem(args.levels, 1)
    g, lay = pb["mesh"], pb["layout"]
    dim, N, nc = g.dim, g.n_nodes, g.dim + 1
    assert not lay.blocked
    lps = P.partition_general(g, args.world)
    vec = [np.asarray(v).reshape(N, nc) for v in pb["vectors"]]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    sync = torch.cuda.synchronize
    rec = dim + 3

    ranks = []
    for lp in lps:
        no, gid = lp.n_owned, lp.global_ids
        ctx = Context(lp.mesh, False, n_owned_nodes=no)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.set_params(pb["params"])
        flags0 = np.ascontiguousarray(pb["node_flags"][gid])
        ctx.set_constraints(flags0)
        h = [np.ascontiguousarray(v[gid[:no]].ravel()) for v in vec]
        ctx.state_set_host(*h)
        ctx.halo_register(lp.send_ptr, lp.send_nodes, lp.recv_ptr, lp.recv_nodes)
        ns, nr = int(lp.send_ptr[-1]), int(lp.recv_ptr[-1])
        ranks.append(dict(lp=lp, ctx=ctx, flags0=flags0, sol0=dev(h[0]), sol=dev(h[0]), old=dev(h[1]),
                          pde=torch.zeros(no * nc, dtype=torch.float64, device="cuda"), tot=torch.zeros(no * nc, dtype=torch.float64, device="cuda"),
                          mass=torch.zeros(max(no, 1), dtype=torch.float64, device="cuda"), cyc=torch.zeros(max(no, 1), dtype=torch.int32, device="cuda"),
                          vs=torch.zeros(max(ns, 1) * rec, dtype=torch.float64, device="cuda"), vr=torch.zeros(max(nr, 1) * rec, dtype=torch.float64, device="cuda"),
                          fs=torch.zeros(max(ns, 1), dtype=torch.uint8, device="cuda"), fr=torch.zeros(max(nr, 1), dtype=torch.uint8, device="cuda")))

    def transport():
        for r, k in enumerate(ranks):
            lp = k["lp"]
            for j, s in enumerate(lp.peers):
                js = lps[s].peers.index(r)
                a, b = int(lps[s].send_ptr[js]), int(lps[s].send_ptr[js + 1])
                o = int(lp.recv_ptr[j])
                k["vr"][o * rec:(o + b - a) * rec] = ranks[s]["vs"][a * rec:b * rec]
                k["fr"][o:o + b - a] = ranks[s]["fs"][a:b]
        sync()

    # the state every repetition starts from: ghosts imported, residual_total and diag_mass of that state on the device
    for k in ranks:
        k["ctx"].halo_pack_all(k["vs"].data_ptr())
    sync()
    transport()
    for k in ranks:
        k["ctx"].halo_unpack_all(k["vr"].data_ptr())
        k["ctx"].assemble_device(True, [], k["pde"].data_ptr(), k["tot"].data_ptr())
        k["ctx"].diag_mass_device(k["mass"].data_ptr())
        k["ctx"].sync_status()

    def reset():
        for k in ranks:
            k["sol"].copy_(k["sol0"])
            k["cyc"].zero_()
            k["ctx"].set_constraints(k["flags0"])
        sync()

    def phase1(k):
        c = k["ctx"]
        k["counts"] = c.active_set_owned_device(k["tot"].data_ptr(), k["mass"].data_ptr(), C_CONST, k["sol"].data_ptr(), k["old"].data_ptr(),
                                                k["cyc"].data_ptr())
        c.state_set_solution_device(k["sol"].data_ptr())
        c.halo_pack_all(k["vs"].data_ptr())
        c.halo_pack_flags_all(k["fs"].data_ptr())
        sync()

    def phase2(k):
        c = k["ctx"]
        c.halo_unpack_all(k["vr"].data_ptr())
        c.halo_unpack_flags_all(k["fr"].data_ptr())
        c.distribute_hanging_device(k["sol"].data_ptr())
        sync()

    def host_round_trip(k):
        c = k["ctx"]
        sol_h, tot_h = k["sol"].cpu().numpy(), k["tot"].cpu().numpy()
        flags = c.get_constraints()
        c.set_constraints(flags)
        k["sol"].copy_(torch.from_numpy(sol_h))
        sync()
        return tot_h

    def timed(fn, *a):
        t0 = time.perf_counter()
        fn(*a)
        return (time.perf_counter() - t0) * 1e3

    dev_ms, host_ms, transport_ms = [[] for _ in ranks], [[] for _ in ranks], []
    for rep in range(args.reps + 1):  # the first repetition is the warm-up: first-use allocations, code objects
        reset()
        t1 = [timed(phase1, k) for k in ranks]
        tt = timed(transport)
        t2 = [timed(phase2, k) for k in ranks]
        th = [timed(host_round_trip, k) for k in ranks]
        if rep:
            transport_ms.append(tt)
            for r in range(len(ranks)):
                dev_ms[r].append(t1[r] + t2[r])
                host_ms[r].append(th[r])
    out = {"bench": "active_set", "workload": f"config-5 stand-in, levels {args.levels}, cut into {args.world} contexts on one device",
           "cells": int(g.n_cells), "nodes": int(N), "hanging_nodes": int(g.hn_nodes.size), "reps": args.reps,
           "transport": "in-process device copies between the contexts' buffers, not RCCL",
           "transport_all_ranks_ms": stats(transport_ms), "ranks": []}
    for r, k in enumerate(ranks):
        lp = k["lp"]
        out["ranks"].append({"rank": r, "owned_nodes": int(lp.n_owned), "local_nodes": int(lp.mesh.n_nodes),
                             "hanging_nodes": int(lp.mesh.hn_nodes.size), "send_nodes": int(lp.send_ptr[-1]), "recv_nodes": int(lp.recv_ptr[-1]),
                             "active": int(k["counts"][0]), "device_ms": stats(dev_ms[r]), "host_round_trip_ms": stats(host_ms[r])})
        k["ctx"].close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
