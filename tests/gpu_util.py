"""Helpers for the GPU parity tests: run a Case through the C ABI and put the result in
the oracle's index space (one global CSR over all dofs)."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

import oracle_api as O
import parity_scale as PS
from cracks_amd import mesh as M
from cracks_amd.assembler import Context, node_flags_from_dof_flags

TOL = 1e-12  # README: |x - x_ref|_inf < 1e-12 max(1, |x_ref|_inf)


def make_context(case, **kw) -> Context:
    ctx = Context(case.mesh, case.layout.blocked, cell_lambda=case.cell_lambda, cell_mu=case.cell_mu, **kw)
    ctx.set_params(case.params)
    ctx.set_constraints(node_flags_from_dof_flags(case.layout, case.cu.flag, case.ch.flag))
    return ctx


def blocks_to_global(ctx: Context, layout, values) -> sp.csr_matrix:
    """Assemble the per-block CSR value arrays into one matrix over the global dofs."""
    n, dim, N = layout.n_dofs, layout.dim, layout.n_nodes
    if not layout.blocked:
        rp, ci = ctx.pattern(0)
        return sp.csr_matrix((values[0], ci, rp), shape=(n, n))
    mats = []
    for b in range(4):
        rp, ci = ctx.pattern(b)
        rows = (N * dim) if b in (0, 1) else N
        cols = (N * dim) if b in (0, 2) else N
        mats.append(sp.csr_matrix((values[b], ci, rp), shape=(rows, cols)))
    return sp.bmat([[mats[0], mats[1]], [mats[2], mats[3]]], format="csr")


def linf_scaled(a, b) -> float:
    """l_inf error scaled by max(1, |reference|_inf)."""
    a = np.asarray(a)
    b = np.asarray(b)
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def oracle(c, residual_only):
    rowptr = colind = None
    if not residual_only:
        rowptr, colind = M.dof_sparsity(c.mesh, c.layout)
    r = O.assemble(c.mesh, c.layout, c.params, c.sol, c.old, c.oldold, c.cu, c.ch, residual_only,
                   rowptr, colind, c.cell_lambda, c.cell_mu)
    assert r.err == 0
    return r, rowptr, colind


def reference_matrix(c, hanging_only=False):
    """The oracle's Jacobian of a Case as one CSR over the global dofs -- the matrix the scales of tests/parity_scale.py
    come from.  hanging_only: distributed with the hanging-node constraints in the place of constraints_update."""
    rowptr, colind = M.dof_sparsity(c.mesh, c.layout)
    r = O.assemble(c.mesh, c.layout, c.params, c.sol, c.old, c.oldold, c.ch if hanging_only else c.cu, c.ch, False,
                   rowptr, colind, c.cell_lambda, c.cell_mu)
    assert r.err == 0
    return sp.csr_matrix((r.values, colind, rowptr), shape=(c.layout.n_dofs,) * 2)


def total_matrix(c, A_ref=None):
    """The reference matrix whose rows belong to residual_total: the active-set scheme (outer_solver 0) distributes that
    vector with the hanging-node constraints alone (cracks.cc:2439-2464), so its Dirichlet and active-set rows hold the
    sums of the unconstrained rows; every other scheme uses constraints_update, i.e. A_ref itself."""
    if c.params.outer_solver == 0:
        return reference_matrix(c, hanging_only=True)
    return reference_matrix(c) if A_ref is None else A_ref


def residual_parity(c, res_pde, res_tot, ref_pde, ref_tot, A_ref=None, A_tot=None, tol=TOL, tag=""):
    """The per-row and per-part checks of tests/parity_scale.py on the two vectors of a residual-only call (either may be
    None), with the scales of one oracle Jacobian of the case."""
    if A_ref is None:
        A_ref = reference_matrix(c)
    if res_pde is not None:
        PS.assert_residual(res_pde, ref_pde, A_ref, c.layout, c.sol, tol, f"{c.name} {tag} residual_pde")
    if res_tot is not None:
        if A_tot is None:
            A_tot = total_matrix(c, A_ref)
        PS.assert_residual(res_tot, ref_tot, A_tot, c.layout, c.sol, tol, f"{c.name} {tag} residual_total")


def reference_parity(layout, sol, A, A_ref, vectors=(), tol=TOL, tag="", A_tot=None):
    """The four checks of tests/parity_scale.py against a reference CSR of any origin (oracle, numpy reference, a scaled 2-D
    matrix): A (or None) per entry and per block on its own pattern, each (vector, reference, "pde" | "tot") per row and per
    part with the scales of A_ref -- of A_tot for "tot", when the scheme distributes residual_total with other constraints.
    Returns A_ref on A's pattern."""
    if A is not None:
        A.sort_indices()
        A_ref = PS.on_pattern(A_ref, A)
        PS.assert_matrix(A, A_ref, layout, tol, tag)
    for v, ref, which in vectors:
        mat = A_tot if (which == "tot" and A_tot is not None) else A_ref
        PS.assert_residual(v, ref, mat, layout, sol, tol, f"{tag} residual_{which}")
    return A_ref


def path_parity(ctx, layout, values, values_other, vectors=(), tol=TOL, tag=""):
    """One GPU path against another, no reference matrix in play: the per-block check on the matrices (blocks classified
    by the layout, so the interleaved layout's single value array is split too) and the per-part check on each pair of
    vectors.  No per-entry or per-row check: their scales belong to a reference."""
    if values is not None:
        A, B = blocks_to_global(ctx, layout, values), blocks_to_global(ctx, layout, values_other)
        A.sort_indices()
        B.sort_indices()
        blk = PS.block_of_entries(layout, PS.entry_rows(B), B.indices)
        PS.assert_blocks([A.data[blk == b] for b in range(4)], [B.data[blk == b] for b in range(4)], tol, f"{tag} (path against path)", PS.BLOCKS)
    phi = PS.is_phi(layout)
    for k, (a, b) in enumerate(vectors):
        PS.assert_parts(a, b, phi, tol, f"{tag} (path against path) vector {k}")


def full_parity(c, tol=TOL, ctx=None):
    """Full assembly, then the residual-only call, of a Case against the oracle: identical pattern, every matrix entry and
    both residuals within tol of max(1, |reference|_inf); then the four checks of tests/parity_scale.py, always at TOL.
    ctx: a context of the case to run on (default: a new one); returned."""
    if ctx is None:
        ctx = make_context(c)
    values, res_pde, _ = ctx.assemble_host(c.sol, c.old, c.oldold, residual_only=False)
    r, rowptr, colind = oracle(c, False)
    A_ref = sp.csr_matrix((r.values, colind, rowptr), shape=(c.layout.n_dofs,) * 2)
    A = blocks_to_global(ctx, c.layout, values)
    # identical pattern (the library's canonical pattern == make_sparsity_pattern stand-in)
    A.sort_indices()
    assert A.nnz == A_ref.nnz and (A.indptr == A_ref.indptr).all() and (A.indices == A_ref.indices).all()
    assert linf_scaled(A.data, A_ref.data) < tol
    assert linf_scaled(res_pde, r.residual_pde) < tol
    _, res_pde2, res_tot2 = ctx.assemble_host(c.sol, c.old, c.oldold, residual_only=True)
    r2, _, _ = oracle(c, True)
    assert linf_scaled(res_pde2, r2.residual_pde) < tol
    assert linf_scaled(res_tot2, r2.residual_total) < tol
    # the same comparisons at the scale of each entry, block, row and part (tests/parity_scale.py)
    # -- always at TOL: a caller's wider tol belongs to the whole-matrix comparison above alone
    PS.assert_matrix(A, A_ref, c.layout, TOL, c.name)
    residual_parity(c, res_pde, None, r.residual_pde, None, A_ref, tag="full")
    residual_parity(c, res_pde2, res_tot2, r2.residual_pde, r2.residual_total, A_ref, tag="residual-only")
    return ctx


def exchange_ghosts(lps, ctxs, dim: int):
    """Ghost import of a partition whose contexts all live on one device, without a communicator: every rank packs what
    its peers need with one launch (pfm_halo_pack_all) and the messages are copied into the receivers' buffers, laid out
    as pfm_halo_unpack_all reads them (per peer, field-major, ``dim + 3`` doubles per node).  Returns the receive buffers;
    unpacking them is the caller's."""
    import torch

    rec = dim + 3
    recv = [torch.zeros(int(lp.recv_ptr[-1]) * rec, dtype=torch.float64, device="cuda") for lp in lps]
    for r, lp in enumerate(lps):
        send = torch.empty(int(lp.send_ptr[-1]) * rec, dtype=torch.float64, device="cuda")
        if send.numel():
            ctxs[r].halo_pack_all(send.data_ptr())
        torch.cuda.synchronize()
        for k, s in enumerate(lp.peers):
            ko = lps[s].peers.index(r)
            o0, o1 = int(lp.send_ptr[k]) * rec, int(lp.send_ptr[k + 1]) * rec
            assert int(lps[s].recv_ptr[ko + 1] - lps[s].recv_ptr[ko]) * rec == o1 - o0
            q0 = int(lps[s].recv_ptr[ko]) * rec
            recv[s][q0:q0 + (o1 - o0)] = send[o0:o1]
    torch.cuda.synchronize()
    return recv
