"""The assembly dispatch of pfm_dispatch.cpp (plan_assembly, assemble_box / assemble_overlay / assemble_general) on paths the
other suites do not reach: every entry point in sequence on one context, the level lattices of the 3-D overlay on streams
of their own, the timing intervals of whole and half assemblies, and the error returns in front of the kernels."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cracks_amd import capi
from cracks_amd.assembler import Context, node_flags_from_dof_flags
from gpu_util import make_context
from test_gpu_cart import BOXES, _full, box_case
from test_gpu_overlay3d import refined_block_case

pytestmark = pytest.mark.gpu
SENT = 1.2345e300
PFM_ERR_BAD_ARG = 1  # include/pfm_assemble.h
BOX3 = next(b for b in BOXES if b[1] == (9, 5, 11))
BOX2 = next(b for b in BOXES if b[1] == (12, 7))


class Buffers:
    """device outputs of one context: the value blocks and both residuals"""

    def __init__(self, ctx):
        import torch

        z = lambda k: torch.empty(k, dtype=torch.float64, device="cuda")
        self.vals = [z(ctx.pattern_size(b)[1]) for b in range(ctx.n_blocks)]
        self.res = [z(ctx.n_owned_dofs), z(ctx.n_owned_dofs)]

    def outs(self, residual_only):
        return self.res if residual_only else self.vals + self.res[:1]


def _call(ctx, bufs, residual_only, fill=True, null_block=None):
    """pfm_assemble_device into bufs (poisoned first): the outputs of the call as host arrays"""
    if fill:
        for o in bufs.outs(residual_only):
            o.fill_(SENT)
    ptrs = [] if residual_only else [0 if b == null_block else v.data_ptr() for b, v in enumerate(bufs.vals)]
    ctx.assemble_device(residual_only, ptrs, bufs.res[0].data_ptr(), bufs.res[1].data_ptr())
    ctx.sync_status()
    return [o.cpu().numpy().copy() for o in bufs.outs(residual_only)]


def _halves(ctx, bufs, residual_only):
    """force_phase(1), then force_phase(2) into the same buffers"""
    ctx.force_phase(1)
    _call(ctx, bufs, residual_only)
    ctx.force_phase(2)
    out = _call(ctx, bufs, residual_only, fill=False)
    ctx.force_phase(0)
    return out


def _line_search(ctx, bufs, sol):
    import torch

    d_sol = torch.from_numpy(np.ascontiguousarray(sol)).cuda()
    for o in bufs.res:
        o.fill_(SENT)
    ctx.assemble_nl_residual_device(d_sol.data_ptr(), bufs.res[0].data_ptr(), bufs.res[1].data_ptr())
    ctx.sync_status()
    return [o.cpu().numpy().copy() for o in bufs.res]


def _same_bits(got, want):
    return len(got) == len(want) and all(a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))
                                         for a, b in zip(got, want))


CASES = {"box3": lambda blocked: box_case(*BOX3, blocked), "box2": lambda blocked: box_case(*BOX2, blocked),
         "overlay3": lambda blocked: refined_block_case((12, 10, 12), blocked)}


@pytest.mark.parametrize("blocked", [True, False])
@pytest.mark.parametrize("kind", list(CASES))
def test_every_entry_in_sequence_on_one_context(kind, blocked):
    """Jacobian, residual-only, the fused line-search call (boxes), the two halves into the same buffers, the whole
    assembly after force_phase(0), and the Jacobian again -- on ONE context, each result bitwise equal to the same call on
    a fresh context in the same node state.  The row-owner kernels and the ordered gather of the 3-D overlay are
    deterministic, so anything one call leaves behind for the next (an event reused, a view left modified,
    DevView::fused_solution left set, a plan of the previous call) shows as a difference."""
    c = CASES[kind](blocked)
    box = kind != "overlay3"
    sol2 = c.sol + 1e-3 * np.random.default_rng(5).standard_normal(c.sol.shape)

    def fresh(sol):
        ctx = make_context(c)
        assert ctx.kernel_path == (1 if box else 3)
        ctx.state_set_host(sol, c.old, c.oldold)
        return ctx, Buffers(ctx)

    def reference(sol, step):
        ctx, bufs = fresh(sol)
        out = step(ctx, bufs)
        ctx.close()
        return out

    steps = [("Jacobian", lambda x, b: _call(x, b, False)), ("residual-only", lambda x, b: _call(x, b, True))]
    if box:
        steps.append(("line search", lambda x, b: _line_search(x, b, sol2)))
    steps += [("halves, Jacobian", lambda x, b: _halves(x, b, False)), ("halves, residual-only", lambda x, b: _halves(x, b, True)),
              ("whole after force_phase(0)", lambda x, b: _call(x, b, False)), ("Jacobian again", lambda x, b: _call(x, b, False))]
    ctx, bufs = fresh(c.sol)
    sol = c.sol
    for name, step in steps:
        got = step(ctx, bufs)
        want = reference(sol, step)
        assert not any((a == SENT).any() for a in got), f"{name}: entries left unwritten"
        assert _same_bits(got, want), f"{name}: differs from the same call on a fresh context"
        if name == "line search":
            sol = sol2  # the call leaves the node state at its solution
    ctx.close()


@pytest.mark.parametrize("blocked", [True, False])
def test_kernel_path_2_matches_oracle(blocked):
    """kernel path 2 (bench.py --path overlay): the general family with the cartesian (u,u) kernel on top of it"""
    _full(box_case(*BOX3, blocked), path=2)


def test_overlay3_level_lattices_on_streams_of_their_own(tmp_path):
    """PFM_OVERLAY3_CONCURRENT=1: every level lattice of the 3-D overlay on a stream of its own, forked off the context's
    stream and joined into it.  The levels write disjoint rows with the row-owner kernels: Jacobian and both residuals
    equal the default process (one level after the other) bit for bit.  The switch is read once: one process each.

    The fork needs two level lattices.  refined_block_case((12, 10, 12)) has them, confirmed from plan_patches3d /
    finish_patches3d by hand: the inner 6 x 4 x 6 coarse cells are refined into a fine level of 12 x 8 x 12 cells whose
    13 x 9 x 13 lattice keeps 9 x 5 x 9 = 405 regular rows (nodes two layers inside the block: not on its boundary, no
    cell with a hanging vertex around them); the coarse level spans the 13 x 11 x 13 lattice of the domain and keeps more
    than 429 regular rows (the three node planes x <= -6.67 alone).  Both pass the thresholds (64 rows, lattice volume
    at most 64 x rows), and the context reports kernel path 3, so the reduced colouring did not overflow."""
    here = os.path.dirname(os.path.abspath(__file__))
    script = tmp_path / "run.py"
    script.write_text(
        "import sys, numpy as np\n"
        f"sys.path[:0] = [{os.path.dirname(here)!r}, {here!r}]\n"
        "from gpu_util import make_context\n"
        "from test_gpu_overlay3d import refined_block_case\n"
        "c = refined_block_case((12, 10, 12), True)\n"
        "ctx = make_context(c)\n"
        "assert ctx.kernel_path == 3\n"
        "values, res, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)\n"
        "_, res_pde, res_tot = ctx.assemble_host(c.sol, c.old, c.oldold, True)\n"
        "np.save(sys.argv[1], np.concatenate([np.ravel(v) for v in values] + [res, res_pde, res_tot]))\n")
    keys = ("PFM_OVERLAY3_CONCURRENT", "PFM_OVERLAY3_MIN_ROWS", "PFM_OVERLAY3_MAX_TABLE", "PFM_NO_PATCH", "PFM_GENERAL_SEQUENTIAL",
            "PFM_HANGING_COLOURED", "PFM_HANGING_ATOMIC")
    got = {}
    for tag, env in (("default", {}), ("concurrent", {"PFM_OVERLAY3_CONCURRENT": "1"})):
        f = tmp_path / f"{tag}.npy"
        e = {k: v for k, v in os.environ.items() if k not in keys}
        e.update(env)
        subprocess.run([sys.executable, str(script), str(f)], check=True, env=e, timeout=600)
        got[tag] = np.load(f)
    assert got["concurrent"].shape == got["default"].shape
    assert np.array_equal(got["concurrent"].view(np.int64), got["default"].view(np.int64))


def test_timing_intervals_of_whole_and_half_assemblies():
    """pfm_timing_enable: one interval per whole assembly, and one per half that pfm_ctx_force_phase selects"""
    c = box_case(*BOX3, True)
    ctx = make_context(c)
    ctx.state_set_host(c.sol, c.old, c.oldold)
    bufs = Buffers(ctx)
    ctx.timing_enable(True)
    for residual_only in (False, True, False):
        _call(ctx, bufs, residual_only)
    for phase in (1, 2):
        ctx.force_phase(phase)
        _call(ctx, bufs, False, fill=phase == 1)
    ctx.force_phase(0)
    t = ctx.kernel_times_ms()
    assert t.shape == (5,) and np.isfinite(t).all() and (t > 0.0).all(), t
    ms, n = ctx.kernel_time_ms()
    assert n == 5 and np.isfinite(ms) and ms > 0.0
    assert ctx.kernel_time_ms()[1] == 0
    ctx.close()


@pytest.mark.parametrize("blocked", [True, False])
def test_errors_in_front_of_the_kernels_leave_a_usable_context(blocked):
    c = box_case(*BOX3, blocked)
    ctx = Context(c.mesh, blocked)
    ctx.set_constraints(node_flags_from_dof_flags(c.layout, c.cu.flag, c.ch.flag))
    ctx.state_set_host(c.sol, c.old, c.oldold)
    bufs = Buffers(ctx)
    with pytest.raises(capi.PfmError, match="pfm_set_params has not been called") as ei:
        _call(ctx, bufs, False)
    assert ei.value.status == PFM_ERR_BAD_ARG
    ctx.set_params(c.params)
    with pytest.raises(capi.PfmError, match="null matrix block") as ei:
        _call(ctx, bufs, False, null_block=ctx.n_blocks - 1)
    assert ei.value.status == PFM_ERR_BAD_ARG
    got = _call(ctx, bufs, False)
    ref = make_context(c)
    ref.state_set_host(c.sol, c.old, c.oldold)
    want = _call(ref, Buffers(ref), False)
    assert not any((a == SENT).any() for a in got) and _same_bits(got, want)
    ctx.close()
    ref.close()
    _full(c, path=1)
