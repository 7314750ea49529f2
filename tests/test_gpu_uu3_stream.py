"""k_cart_uu3 on the smallest box that reaches every path of its plane loop, against the CPU oracle.

The box has 17 x 9 x 6 cells, i.e. 18 x 10 x 7 nodes: with tiles of 8 x 4 nodes that is two full tile columns and a partial
one in x and the same in y.  Exactly one tile -- nodes 8..15 x 4..7 -- is interior, and on the planes 1 to 5 all of its 32
rows have 27 neighbours: those five tile-planes take the regular copy-out (16-byte stores, node groups without clamps),
every other tile-plane the face path.  The w*g phase reads its (cell, z-level) word, the node phase forms the cross-half
sums of the oz = 0 slots behind the finished dot of the residual rows; the cases run them

  (a) without any constraint flag (no masked node phase anywhere),
  (b) with u = 0 on the boundary and one flagged node inside the regular tile (masked node phase, the placeholder of a
      constrained row, cross-half sums of masked entries, the drained request wait behind an irregular plane),
  (c) as (b) in chunks of 2 and of 3 planes: chunk seams, the prologue of every chunk, a last chunk of one plane,
  (d) with per-cell Lame coefficients (the HET instantiation),
  (e) in the interleaved layout (NCOL = 4),
  (f) with the residual from the matrix rows (the default, RES on: all of the above) and with PFM_RES_KERNEL=1 (RES off:
      the switch is read once per process, hence a child process).

Every case holds each matrix entry and the residual to the bar of tests/gpu_util.py (1e-12 max(1, |x_ref|_inf), then the
per-entry, per-block and per-row scales of tests/parity_scale.py) and assembles twice: the row-owner kernel has no atomics
and a fixed order of every sum, so the two results are the same bits.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import parity_scale as PS
from cracks_amd import mesh as M
from cracks_amd.assembler import Context
from gpu_util import TOL, blocks_to_global, linf_scaled, make_context
from test_gpu_cart import box_case, heterogeneous, oracle

pytestmark = pytest.mark.gpu
N = (17, 9, 6)
NX, NY = N[0] + 1, N[1] + 1
FLAGGED = 10 + NX * (5 + NY * 3)  # node (10, 5, 3): inside the regular tile, on its middle plane
KINDS = ("free", "flagged", "het", "interleaved")


def make_case(kind):
    c = box_case(3, N, -10.0, 10.0, kind != "interleaved")
    lay = c.layout
    if kind == "free":
        c.cu = M.update_constraints(c.mesh, lay, [])
    else:  # u = 0 on the boundary (box_case) and the components 0 and 2 of one interior node
        extra = [int(lay.dof(np.array([FLAGGED]), comp)[0]) for comp in (0, 2)]
        c.cu = M.update_constraints(c.mesh, lay, np.union1d(M.sneddon_dirichlet_dofs(c.mesh, lay), extra))
    if kind == "het":
        heterogeneous(c, seed=11)
    c.name = f"uu3 stream {kind}"
    return c


@functools.lru_cache(maxsize=None)
def reference(kind):
    """the case and the oracle's Jacobian and residual of it: computed once, shared, never written to"""
    c = make_case(kind)
    r, rp, ci = oracle(c, False)
    A_ref = sp.csr_matrix((r.values, ci, rp), shape=(c.layout.n_dofs,) * 2)
    return c, A_ref, r.residual_pde


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def against_oracle(kind, ctx, values, res_pde, tag):
    c, A_ref, ref_pde = reference(kind)
    A = blocks_to_global(ctx, c.layout, values)
    A.sort_indices()
    assert A.nnz == A_ref.nnz and (A.indptr == A_ref.indptr).all() and (A.indices == A_ref.indices).all(), tag
    assert linf_scaled(A.data, A_ref.data) < TOL, tag
    assert linf_scaled(res_pde, ref_pde) < TOL, tag
    PS.assert_matrix(A, A_ref, c.layout, TOL, f"{c.name} {tag}")
    PS.assert_residual(res_pde, ref_pde, A_ref, c.layout, c.sol, TOL, f"{c.name} {tag} residual_pde")


def assemble_twice(kind, ctx, tag):
    c = reference(kind)[0]
    assert ctx.kernel_path == 1, "a uniform box runs the row-owner kernels"
    v0, r0, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
    v1, r1, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
    assert all(same_bits(a, b) for a, b in zip(v0, v1)) and same_bits(r0, r1), f"{tag}: two assemblies differ in some bit"
    against_oracle(kind, ctx, v0, r0, tag)
    return v0, r0


@pytest.mark.parametrize("kind", KINDS)  # (a), (b), (d), (e); the residual from the rows: first half of (f)
def test_plane_loop_against_oracle(kind):
    ctx = make_context(reference(kind)[0])
    assemble_twice(kind, ctx, "default chunks")
    ctx.close()


@pytest.mark.parametrize("planes", [2, 3])  # (c): 7 planes in chunks of 2 + 2 + 2 + 1 and of 3 + 3 + 1
def test_chunk_seams_and_a_last_chunk_of_one_plane(planes):
    ctx = make_context(reference("flagged")[0])
    whole = assemble_twice("flagged", ctx, "default chunks")
    ctx.force_zchunk(Context.ZC_UU3, planes)
    assert ctx.zchunk(Context.ZC_UU3) == planes
    cut = assemble_twice("flagged", ctx, f"chunks of {planes} planes")
    # every row's sums are formed in the same order whatever chunk its plane falls in
    assert all(same_bits(a, b) for a, b in zip(whole[0], cut[0])) and same_bits(whole[1], cut[1])
    ctx.force_zchunk(Context.ZC_UU3, 0)
    ctx.close()


CHILD = """
import sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import test_gpu_uu3_stream as T
from gpu_util import make_context
out = {{}}
for kind in T.KINDS[:2]:
    c = T.make_case(kind)
    ctx = make_context(c)
    for run in range(2):
        values, res, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
        for b, v in enumerate(values):
            out[f"{{kind}}_{{run}}_v{{b}}"] = v
        out[f"{{kind}}_{{run}}_res"] = res
np.savez(sys.argv[1], **out)
"""


def test_without_the_residual_rows(tmp_path):
    """second half of (f): PFM_RES_KERNEL=1 launches the kernel without its residual rows (the quadrature kernel writes
    the residual); cases (a) and (b) in one child process"""
    here = os.path.dirname(os.path.abspath(__file__))
    script, out = tmp_path / "run.py", tmp_path / "out.npz"
    script.write_text(CHILD.format(root=os.path.dirname(here), tests=here))
    env = dict(os.environ, PFM_RES_KERNEL="1")
    subprocess.run([sys.executable, str(script), str(out)], check=True, env=env, timeout=300)
    got = np.load(out)
    for kind in KINDS[:2]:
        ctx = make_context(reference(kind)[0])  # (the pattern of the blocks)
        runs = [([got[f"{kind}_{run}_v{b}"] for b in range(ctx.n_blocks)], got[f"{kind}_{run}_res"]) for run in range(2)]
        assert all(same_bits(a, b) for a, b in zip(runs[0][0], runs[1][0])) and same_bits(runs[0][1], runs[1][1])
        against_oracle(kind, ctx, runs[0][0], runs[0][1], "PFM_RES_KERNEL=1")
        ctx.close()
