"""Helpers for the GPU parity tests: run a Case through the C ABI and put the result in
the oracle's index space (one global CSR over all dofs)."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

import oracle_api as O
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


def full_parity(c, tol=TOL, ctx=None):
    """Full assembly, then the residual-only call, of a Case against the oracle: identical pattern, every matrix entry and
    both residuals within tol.  ctx: a context of the case to run on (default: a new one); returned."""
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
