"""The launches of the cartesian family, for comparing two builds of the library launch by launch (a change of the launchers,
of plan_cart or of the dispatch in pfm_dispatch.cpp must leave this listing as it is):

    rocprofv3 --kernel-trace --output-format csv -d DIR -o p -- python tools/launch_trace.py        # the run to trace
    python tools/launch_trace.py --list DIR > listing.txt                                            # its launches

(`PFM_LIB=<other .so>` selects the other build.)  The run makes, at the sizes of the tests and each behind a warm-up of
itself: 3-D box Jacobian, residual-only, the line-search entry, the halves 1 and 2 of the overlapped assembly, 2-D box
Jacobian and residual-only, the 3-D overlay Jacobian, and -- their colour-class launch sizes and patch-block counts come
straight from the mesh analysis of pfm_ctx_create (pfm_mesh_plan.cpp) -- the Jacobian and residual-only of the 2-D mesh with
hanging nodes of tests/sneddon_2d_1.prm (patch overlay) and of the general-family 3-D fan with a hanging node
(topology_cases.fan3d_30_hanging).  The listing has one line per dispatch in dispatch order: kernel, grid,
workgroup, LDS bytes, and the queue as the ordinal of its first appearance."""
import csv
import glob
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "tests")]


def run():
    import numpy as np
    import torch

    import cases
    import topology_cases
    from gpu_util import make_context
    from test_gpu_dispatch import BOX2, BOX3, Buffers, _call, _halves, _line_search
    from test_gpu_cart import box_case
    from test_gpu_overlay3d import refined_block_case

    def steps(c, box3=False, residual=False):
        ctx = make_context(c)
        ctx.state_set_host(c.sol, c.old, c.oldold)
        bufs = Buffers(ctx)
        todo = [lambda: _call(ctx, bufs, False)]
        if box3 or residual:
            todo.append(lambda: _call(ctx, bufs, True))
        if box3:
            todo += [lambda: _line_search(ctx, bufs, c.sol), lambda: _halves(ctx, bufs, False), lambda: _halves(ctx, bufs, True)]
        for f in todo:
            for _ in range(2):  # warm-up, then the call
                f()
                torch.cuda.synchronize()
        ctx.close()

    steps(box_case(*BOX3, True), box3=True)
    steps(box_case(*BOX3, False), box3=True)
    steps(box_case(*BOX2, True), residual=True)
    steps(refined_block_case((12, 10, 12), True))
    steps(cases.kat_sneddon_2d(), residual=True)
    steps(topology_cases.fan3d_30_hanging(), residual=True)
    print("launch_trace: done")


def listing(directory):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        sys.exit("no *kernel_trace.csv under " + directory)
    rows = []
    for f in files:
        rows += list(csv.DictReader(open(f)))
    col = lambda row, *names: next((row[n] for n in names if n in row), "?")
    rows.sort(key=lambda r: int(col(r, "Dispatch_Id", "Correlation_Id")))
    queues = {}
    for r in rows:
        q = queues.setdefault(col(r, "Queue_Id"), len(queues))
        name = col(r, "Kernel_Name").replace("(anonymous namespace)::", "").split("(")[0]
        grid = "x".join(col(r, "Grid_Size_" + a, "Grid_Size") for a in "XYZ")
        wg = "x".join(col(r, "Workgroup_Size_" + a, "Workgroup_Size") for a in "XYZ")
        print(f"{name} grid={grid} wg={wg} lds={col(r, 'LDS_Block_Size', 'Group_Segment_Size')} queue={q}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--list":
        listing(sys.argv[2])
    else:
        run()
