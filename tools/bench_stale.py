"""The flagship Jacobian of bench.py with old_solution alternating between two arrays at every step: every assembly finds
a kept (u,u) block stale and writes it (bench.py itself never changes the old vectors, so behind its warm-up it shows
kept steps only).  One JSON line: ms per step (wall) and the mean kernel-group time of the library's event pairs.

  python tools/bench_stale.py [--n 216] [--steps 20] [--warmup 3] [--same]     # --same: old_solution stays (kept steps)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=216)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--same", action="store_true")
    args = ap.parse_args()
    import torch

    from cracks_amd import partition as P
    from cracks_amd.assembler import Assembler

    dim, n = 3, args.n
    lp = P.build_local_problem(dim, (n,) * dim, P.bench_grid(1, dim, n), 0)
    h = (20.0 / n) * np.sqrt(dim)
    u, phi, po, poo, flags = bench.synthetic_state(lp.mesh, lp.global_ids, h, dim)
    asm = Assembler(lp.mesh, blocked=True, n_owned_nodes=lp.n_owned)
    asm.set_params(bench.sneddon_params(h, dim))
    asm.set_constraints(flags)
    pack = lambda uu, pp: np.concatenate([uu.reshape(-1), pp])
    asm.set_vectors(pack(u, phi), pack(0 * u, po), pack(0 * u, poo))
    olds = [asm.old_solution.clone(), asm.old_solution.clone()]
    if not args.same:
        olds[1][dim * lp.n_owned:] = 0.5 * (olds[0][dim * lp.n_owned:] + asm.old_old_solution[dim * lp.n_owned:])
    k = [0]

    def step():
        asm.old_solution = olds[k[0] & 1]
        k[0] += 1
        asm.assemble_system(False)

    for _ in range(args.warmup):
        step()
    asm.synchronize()
    asm.ctx.timing_enable(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / args.steps * 1e3
    asm.synchronize()
    k_ms, _ = asm.ctx.kernel_time_ms()
    print(json.dumps({"n": n, "old_solution": "same" if args.same else "alternating", "ms_per_step": round(wall, 4), "kernel_ms": round(k_ms, 4),
                      "keeps_uu_block": hasattr(asm.ctx.lib, "pfm_values_keep_uu_block") and asm.ctx.values_uu_block_kept() != 0,
                      "lib": os.environ.get("PFM_LIB", "")}))


if __name__ == "__main__":
    main()
