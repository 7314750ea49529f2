"""The generic copy-outs of k_cart_uu3 and k_cart_phi4 (rows at the faces of the box, partial tiles, flagged planes,
interleaved layout) on the smallest boxes in which every tile class of both kernels occurs.

Both kernels pick one of two loops per tile-plane: rows in lattice order (no look-up, no wait for the stores) or rows
whose CSR slots are a permutation (CartView::row_perm).  The canonical pattern runs the first loop, a pattern bound with
shuffled columns the second; both must give the oracle's entries, overwrite every output, repeat bit for bit and agree
with each other entry for entry through the column map."""
import numpy as np
import pytest
import scipy.sparse as sp

from cracks_amd import mesh as M
from gpu_util import TOL, blocks_to_global, linf_scaled, make_context, oracle, reference_parity
from test_gpu_cart import box_case
from test_gpu_pattern import _permuted_patterns

pytestmark = pytest.mark.gpu

# cells; nodes = cells + 1.  k_cart_uu3 tiles are 8 x 4 nodes, k_cart_phi4 tiles 7 x 7 nodes.
BOXES = [
    (8, 4, 2),    # 9 x 5 x 3 nodes: only face and partial tiles
    (26, 14, 5),  # 27 x 15 x 6: interior tiles of k_cart_uu3 next to face tiles, a last tile column one node wide, several
                  # planes (the landing waits behind a generic plane)
    (22, 22, 4),  # 23 x 23 x 5: interior, face and partial tiles of k_cart_phi4
]


def _run(ctx, nb):
    """One full assembly into outputs prefilled with NaN."""
    import torch

    vals = [torch.full((ctx.pattern_size(b)[1],), np.nan, dtype=torch.float64, device="cuda") for b in range(nb)]
    res = torch.full((ctx.n_owned_dofs,), np.nan, dtype=torch.float64, device="cuda")
    ctx.assemble_device(False, [v.data_ptr() for v in vals], res.data_ptr(), 0)
    ctx.sync_status()
    return [v.cpu().numpy() for v in vals], res.cpu().numpy()


def _bitwise(va, ra, vb, rb, what):
    for b, (x, y) in enumerate(zip(va, vb)):
        bad = np.nonzero(x.view(np.int64) != y.view(np.int64))[0]
        assert bad.size == 0, (f"{what}: block {b}, {bad.size} of {x.size} entries differ, first at {bad[:8]}: {x[bad[:4]]} / {y[bad[:4]]}; "
                               f"NaN {int(np.isnan(x).sum())} / {int(np.isnan(y).sum())}")
    assert np.array_equal(ra.view(np.int64), rb.view(np.int64)), f"{what}: residual"


def _against_oracle(ctx, c, vals, res, A_ref, res_ref):
    for v in vals:
        assert not np.isnan(v).any()  # every entry of every block written
    assert not np.isnan(res).any()
    A = blocks_to_global(ctx, c.layout, [v.copy() for v in vals])  # (sort_indices works in place on the arrays it was given)
    A.sort_indices()
    assert (A.indptr == A_ref.indptr).all() and (A.indices == A_ref.indices).all()
    e_mat, e_res = linf_scaled(A.data, A_ref.data), linf_scaled(res, res_ref)
    print(f"|dA|_inf = {e_mat:.2e}, |dR|_inf = {e_res:.2e}")
    assert e_mat < TOL and e_res < TOL
    reference_parity(c.layout, c.sol, A, A_ref, [(res, res_ref, "pde")], tag="face tiles")


@pytest.mark.parametrize("flagged", [True, False], ids=["dirichlet_faces", "no_flags"])
@pytest.mark.parametrize("blocked", [True, False], ids=["blocked", "interleaved"])
@pytest.mark.parametrize("n", BOXES, ids=lambda n: "x".join(map(str, n)))
def test_face_and_partial_tiles(n, blocked, flagged):
    c = box_case(3, n, -10.0, 10.0, blocked)  # u = 0 on all faces, as bench.synthetic_state flags them
    if not flagged:
        c.cu = M.update_constraints(c.mesh, c.layout, [])
    r, rp, ci = oracle(c, False)
    A_ref = sp.csr_matrix((r.values, ci, rp), shape=(c.layout.n_dofs,) * 2)
    ctx = make_context(c)
    assert ctx.kernel_path == 1
    nb = ctx.n_blocks
    ctx.state_set_host(c.sol, c.old, c.oldold)

    # canonical pattern: every row in lattice order
    v0, r0 = _run(ctx, nb)
    _against_oracle(ctx, c, v0, r0, A_ref, r.residual_pde)
    v0b, r0b = _run(ctx, nb)
    _bitwise(v0, r0, v0b, r0b, "canonical pattern, second assembly")

    # the same rows with their columns shuffled: every row carries a permutation
    pats = _permuted_patterns(ctx, 3, blocked, seed=11)
    for b, (prp, pci, _) in enumerate(pats):
        ctx.pattern_bind(b, prp, pci)
    v1, r1 = _run(ctx, nb)
    _against_oracle(ctx, c, v1, r1, A_ref, r.residual_pde)
    v1b, r1b = _run(ctx, nb)
    _bitwise(v1, r1, v1b, r1b, "bound pattern, second assembly")

    # entry for entry through the column map, bit for bit
    _bitwise(v1, r1, [v0[b][src] for b, (_, _, src) in enumerate(pats)], r0, "bound against canonical pattern")
    ctx.close()
