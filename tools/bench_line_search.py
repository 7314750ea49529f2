#!/usr/bin/env python3
"""Time one trial of the Newton line search (cracks.cc:2942-2957) at 216^3 cells (3-D box, blocked layout) and 1000^2 cells
(2-D box), with the vectors on the device:

  (a) composed   today's composition of entries, one trial = torch ``copy_`` / ``add_`` / ``mul_`` for the vector statements
                 (solution += update; ...; solution = saved; update *= damping) + ``assemble_nl_residual_device`` +
                 ``residual_norms``.  These entries are the parent commit's, so (a) is the parent's number.
  (b) device     ``pfm_line_search_device`` with reference = 0.0: every one of --steps trials runs, the time is divided by
                 --steps.

Wall time around each search (both forms synchronise once per trial, as the compare needs the norm on the host), --reps
searches each, reported as median and min - max per trial.  Prints one JSON line.

    python tools/bench_line_search.py [--n3 216] [--n2 1000] [--steps 10] [--reps 7]
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

DAMPING = 0.6


def one_size(dim, n, blocked, steps, reps):
    import torch

    import bench
    from cracks_amd import mesh as M
    from cracks_amd import partition as P
    from cracks_amd.assembler import Context

    lp = P.build_local_problem(dim, (n,) * dim, (1,) * dim, 0)
    mesh = lp.mesh
    h = (20.0 / n) * np.sqrt(dim)
    u, phi, po, poo, _ = bench.synthetic_state(mesh, lp.global_ids, h, dim)
    lay = M.DofLayout(mesh.n_nodes, dim, blocked=blocked)
    sol0 = lay.pack(u, phi)
    ctx = Context(mesh, blocked)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_params(bench.sneddon_params(h, dim))
    ctx.set_constraints(np.zeros(mesh.n_nodes, np.uint8))
    ctx.state_set_host(sol0, lay.pack(0 * u, po), lay.pack(0 * u, poo))
    rng = np.random.default_rng(5)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    sol_start, upd_start = dev(sol0), dev(lay.pack(rng.uniform(-1e-4, 1e-4, u.shape), rng.uniform(-0.05, 0.05, phi.shape)))
    sol, upd, saved = torch.empty_like(sol_start), torch.empty_like(sol_start), torch.empty_like(sol_start)
    pde, tot = torch.empty_like(sol_start), torch.empty_like(sol_start)

    def reset():
        sol.copy_(sol_start)
        upd.copy_(upd_start)
        torch.cuda.synchronize()

    def composed():
        saved.copy_(sol)
        for _ in range(steps):
            sol.add_(upd)
            ctx.assemble_nl_residual_device(sol.data_ptr(), pde.data_ptr(), tot.data_ptr())
            trial = ctx.residual_norms(pde.data_ptr())[0]
            if trial < 0.0:
                break
            sol.copy_(saved)
            upd.mul_(DAMPING)
        torch.cuda.synchronize()

    def device():
        r = ctx.line_search_device(sol.data_ptr(), upd.data_ptr(), pde.data_ptr(), tot.data_ptr(), 0.0, steps, DAMPING)
        torch.cuda.synchronize()
        assert r["steps"] == steps and not r["accepted"]

    out = {"dim": dim, "n": n, "layout": "blocked" if blocked else "interleaved", "dofs": int(lay.n_dofs), "kernel_path": ctx.kernel_path,
           "steps": steps, "reps": reps}
    for name, fn in (("composed", composed), ("device", device)):
        reset()
        fn()  # warm-up: first-use allocations, code objects
        ts = []
        for _ in range(reps):
            reset()
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3 / steps)
        out[name + "_ms_per_trial"] = {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n3", type=int, default=216)
    ap.add_argument("--n2", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    res = [one_size(3, args.n3, True, args.steps, args.reps), one_size(2, args.n2, True, args.steps, args.reps)]
    print(json.dumps({"bench": "line_search", "results": res}))


if __name__ == "__main__":
    main()
