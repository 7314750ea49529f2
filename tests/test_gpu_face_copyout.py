"""The copy-outs of k_cart_uu3 and k_cart_phi4 on tile-planes off the interior path: x, y and z faces, corners, partial
tiles, tiles that hold a single node column or row (the 2^L + 1 boxes), flagged planes -- and the waits behind them.

The lattice-order loop of k_cart_uu3 maps thread <-> (node group, element of the row) and walks the rows of the tile in two
batches; the request waves wait for a counted number of stores behind a regular plane and drain behind any other.  The
boxes below put both kinds of plane in front of and behind each other, at the model's z-chunk and at forced chunks of 1 and
3 planes (every plane the first of a chunk, chunk starts on a z face and on a regular plane).  Every case: each entry of each
block and the residual against the oracle at the project's bar (1e-12 at the scale of each block, entry and row), outputs
prefilled with NaN fully overwritten, a second assembly bit for bit the first."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from cracks_amd import mesh as M
from cracks_amd.assembler import Context
from gpu_util import make_context, oracle
from test_gpu_cart import box_case
from test_gpu_face_tiles import _against_oracle, _bitwise
from test_gpu_pattern import _permuted_patterns

pytestmark = pytest.mark.gpu

# cells; nodes = cells + 1.  k_cart_uu3 tiles are 8 x 4 nodes, k_cart_phi4 tiles 7 x 7 nodes.
BOXES = [
    (13, 13, 3),  # 14 x 14 nodes: all four tiles of k_cart_phi4 full and on a face or corner; k_cart_uu3: partial last tile column
    (15, 7, 3),   # 16 x 8 nodes: all four tiles of k_cart_uu3 full and on faces
    (16, 8, 2),   # 17 x 9 nodes (2^L + 1): last tile column / row of k_cart_uu3 one node wide; every plane on or next to a z face
    (22, 22, 4),  # 23 x 23 x 5: interior, face, corner and partial tiles together; planes 1..3 regular between the z faces
]
BIG = (22, 22, 4)
FLAGS = ["dirichlet_faces", "no_flags", "interior_flags"]


def _interior_dofs(c, n):
    """displacement components of a few interior nodes and one phase-field dof of the active set: planes become masked
    away from the faces (k_cart_phi4 looks one plane up and down)"""
    nx, ny = n[0] + 1, n[1] + 1
    node = lambda i, j, k: i + nx * (j + ny * k)
    u = [(node(11, 11, 2), 0), (node(11, 11, 2), 1), (node(11, 11, 2), 2), (node(5, 16, 2), 1), (node(12, 3, 1), 0), (node(12, 3, 1), 2)]
    return [int(c.layout.dof(a, b)) for a, b in u], [int(c.layout.dof(node(8, 8, 2), 3))]


@functools.lru_cache(maxsize=None)
def _case(n, blocked, flags):
    """the case and its oracle, computed once and left unchanged"""
    c = box_case(3, n, -10.0, 10.0, blocked)  # u = 0 on all faces, as bench.synthetic_state flags them
    if flags == "no_flags":
        c.cu = M.update_constraints(c.mesh, c.layout, [])
    elif flags == "interior_flags":
        u, act = _interior_dofs(c, n)
        c.cu = M.update_constraints(c.mesh, c.layout, list(M.sneddon_dirichlet_dofs(c.mesh, c.layout)) + u, act)
    r, rp, ci = oracle(c, False)
    return c, r, sp.csr_matrix((r.values, ci, rp), shape=(c.layout.n_dofs,) * 2)


def _run(ctx, nb, shift=0):
    """One full assembly into outputs prefilled with NaN.  shift = 1: every output is a view that starts one double into a
    larger tensor (8-byte, not 16-byte aligned); the doubles in front of and behind the view must stay NaN."""
    import torch

    sizes = [ctx.pattern_size(b)[1] for b in range(nb)] + [ctx.n_owned_dofs]
    whole = [torch.full((k + 2 * shift,), np.nan, dtype=torch.float64, device="cuda") for k in sizes]
    outs = [w[shift:shift + k] for w, k in zip(whole, sizes)]
    assert all(o.data_ptr() % 16 == 8 * shift for o in outs)
    ctx.assemble_device(False, [v.data_ptr() for v in outs[:-1]], outs[-1].data_ptr(), 0)
    ctx.sync_status()
    if shift:
        for w in whole:
            assert bool(torch.isnan(w[0])) and bool(torch.isnan(w[-1])), "a store outside the value array"
    return [v.cpu().numpy() for v in outs[:-1]], outs[-1].cpu().numpy()


CASES = [(n, blocked, flags) for n in BOXES for blocked in (True, False) for flags in FLAGS
         if flags != "interior_flags" or n == BIG]  # (interior flags need interior nodes)


@pytest.mark.parametrize("n,blocked,flags", CASES,
                         ids=["-".join(["x".join(map(str, n)), "blocked" if b else "interleaved", f]) for n, b, f in CASES])
def test_face_copyout(n, blocked, flags):
    c, r, A_ref = _case(n, blocked, flags)
    ctx = make_context(c)
    assert ctx.kernel_path == 1
    nb = ctx.n_blocks
    ctx.state_set_host(c.sol, c.old, c.oldold)

    v0, r0 = _run(ctx, nb)
    _against_oracle(ctx, c, v0, r0, A_ref, r.residual_pde)
    _bitwise(v0, r0, *_run(ctx, nb), "second assembly")

    if n == BIG:
        # value arrays that are 8-byte but not 16-byte aligned
        _bitwise(v0, r0, *_run(ctx, nb, shift=1), "outputs one double into a larger tensor")
        # chunk starts on both kinds of plane: every plane alone, and chunks {0, 1, 2}, {3, 4}
        for L in (1, 3):
            for k in (Context.ZC_UU3, Context.ZC_PHI4):
                ctx.force_zchunk(k, L)
                assert ctx.zchunk(k) == L
            _bitwise(v0, r0, *_run(ctx, nb), f"z-chunks of {L}")
            _bitwise(v0, r0, *_run(ctx, nb, shift=1), f"z-chunks of {L}, outputs one double into a larger tensor")
        for k in (Context.ZC_UU3, Context.ZC_PHI4):
            ctx.force_zchunk(k, 0)

        # the same rows with their columns shuffled: every row carries a permutation, the permuted loops are taken
        pats = _permuted_patterns(ctx, 3, blocked, seed=11)
        for b, (prp, pci, _) in enumerate(pats):
            ctx.pattern_bind(b, prp, pci)
        v1, r1 = _run(ctx, nb)
        _against_oracle(ctx, c, v1, r1, A_ref, r.residual_pde)
        _bitwise(v1, r1, *_run(ctx, nb), "bound pattern, second assembly")
        _bitwise(v1, r1, [v0[b][src] for b, (_, _, src) in enumerate(pats)], r0, "bound against canonical pattern")
    ctx.close()
