"""Both halves of the overlapped assembly (pfm_assemble_overlapped, include/pfm_assemble.h) on every kernel family.

A multi-GPU host hides the ghost import behind cell work: phase 1 assembles what reads no ghost node, the import lands,
phase 2 completes the same buffers.  Every family cuts that work its own way -- the tile filter of k_cart_uu3,
k_cart_residual3, k_cart_residual2m and (per node) k_cart2d_cells, the compact boundary-tile launches of phase 2, the
Jacobian kernels that follow the cut one in phase 2, the general family and the overlays that leave everything to
phase 2 -- so each is run here: all ranks of a partition on cuda:0, the ghost import through the HIP pack / unpack
kernels, pfm_ctx_force_phase selecting a half.  Per rank, for the full and the residual-only assembly:

1. the whole assembly W writes every owned output entry and matches the reference on every owned row;
2. phase 1 with poisoned ghosts (NaN, then a different valid state: NaN can vanish in a clamp) writes only entries
   bitwise equal to W -- a ghost read in phase 1 shows although phase 2 would overwrite it;
3. phase 2 after the real import completes those buffers to W, bit for bit;
4. the whole assembly again afterwards gives W;
5. the split splits: where a rank has interior tiles, phase 1 writes most of the output of the cut kernel; the general
   family and the overlays write nothing in phase 1.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from cracks_amd import mesh as M
from cracks_amd import partition as P
from cracks_amd.assembler import Context, node_flags_from_dof_flags
import parity_scale as PS
from gpu_util import blocks_to_global, exchange_ghosts, linf_scaled, reference_matrix, total_matrix
from test_gpu_cart import box_case, dead_zone, heterogeneous, oracle

pytestmark = pytest.mark.gpu
TOL = 1e-12  # README: |x - x_ref|_inf < 1e-12 max(1, |x_ref|_inf)
SENT = 1.2345e300


# ---- global problems ------------------------------------------------------------------------------------------------
def global_case(dim, n, kind, blocked):
    """stag: staggered scheme (3-D: residual from the rows of k_cart_uu3 / k_cart_phi4); mono: monolithic (3-D: the
    quadrature residual kernel is the cut one); het: per-cell Lame coefficients; dead / mono_dead: Dirichlet lines, an
    active set and a dead zone with kappa = 0 (placeholder diagonals, the mean |diagonal| of the element); flat: dead plus
    G_c = 0 and no displacement on y > 0, where the (phi,phi) element diagonal vanishes too while the (u,u) one does not --
    the 2-D phase-field rows take their placeholder from the mean that the displacement launch left in cell_avg."""
    c = box_case(dim, n, -10.0, 10.0, blocked, monolithic=kind in ("mono", "mono_dead"))
    if kind in ("dead", "mono_dead", "flat"):
        dead_zone(c)
    if kind == "flat":
        c.params.G_c = 0.0
        c.params.gamma_penal = 0.0
        node, comp = c.layout.node_comp_of_dof()
        c.sol[(comp < dim) & (c.mesh.coords[node][:, 1] > 0.0)] = 0.0
    if kind == "het":
        heterogeneous(c, seed=7)
    return c


def _lattice_cell(g0, n):
    """lattice index of the cell whose lowest vertex is global node g0 (lexicographic box numbering)"""
    idx = np.zeros_like(g0)
    rem = g0.copy()
    mult = 1
    for d in range(len(n)):
        idx += mult * (rem % (n[d] + 1))
        rem //= n[d] + 1
        mult *= n[d]
    return idx


def _local_vector(F, g_owned, blocked):
    """dof vector over the owned nodes in the context's layout from nodal values F[global node, component]"""
    no, nc = g_owned.size, F.shape[1]
    lay = M.DofLayout(no, nc - 1, blocked)
    v = np.empty(lay.n_dofs)
    for c in range(nc):
        v[lay.dof(np.arange(no), c)] = F[g_owned, c]
    return v


class Rank:
    def __init__(self, lp, ctx, state, index, flags):
        self.lp, self.ctx, self.state, self.index = lp, ctx, state, index  # state: the device vectors of pfm_state_set
        self.flags = flags  # constraint bits of the local nodes


def _rank(index, lp, blocked, prm, flags, nodal, **kw):
    import torch

    ctx = Context(lp.mesh, blocked, n_owned_nodes=lp.n_owned, **kw)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_params(prm)
    ctx.set_constraints(flags[lp.global_ids])
    go = lp.global_ids[:lp.n_owned]
    state = [torch.from_numpy(_local_vector(F, go, blocked)).cuda() for F in nodal]
    ctx.state_set_device(*[s.data_ptr() for s in state])
    ctx.halo_register(lp.send_ptr, lp.send_nodes, lp.recv_ptr, lp.recv_nodes)
    torch.cuda.synchronize()
    return Rank(lp, ctx, state, index, flags[lp.global_ids])


def box_ranks(c, n, p):
    """every rank of the box partition p of the global case c (partition.build_local_problem)"""
    dim, blocked = len(n), c.layout.blocked
    node, comp = c.layout.node_comp_of_dof()
    nodal = []
    for v in (c.sol, c.old, c.oldold):
        F = np.empty((c.layout.n_nodes, dim + 1))
        F[node, comp] = v
        nodal.append(F)
    flags = node_flags_from_dof_flags(c.layout, c.cu.flag, c.ch.flag)
    lam = mu = None
    if c.cell_lambda is not None:  # the global case's cells are shuffled: per-cell data by lattice position
        lat = _lattice_cell(c.mesh.cells[:, 0].astype(np.int64), n)
        lam, mu = np.empty(lat.size), np.empty(lat.size)
        lam[lat], mu[lat] = c.cell_lambda, c.cell_mu
    lps = [P.build_local_problem(dim, n, p, r) for r in range(int(np.prod(p)))]
    ranks = []
    for r, lp in enumerate(lps):
        kw = {}
        if lam is not None:
            lat = _lattice_cell(lp.global_ids[lp.mesh.cells[:, 0]].astype(np.int64), n)
            kw = dict(cell_lambda=lam[lat], cell_mu=mu[lat])
        ranks.append(_rank(r, lp, blocked, c.params, flags, nodal, **kw))
        assert ranks[-1].ctx.kernel_path == 1, "sub-boxes stay on the cartesian family"
    return ranks


# ---- references in the global dof numbering ------------------------------------------------------------------------
class Reference:
    """A (scipy CSR over the global dofs, indices sorted) or None, and the two residuals"""

    def __init__(self, layout, A, res_pde, res_tot, sol=None, A_scale=None, A_tot=None):
        self.layout, self.A, self.res_pde, self.res_tot = layout, A, res_pde, res_tot
        # for the per-row scale of tests/parity_scale.py: the solution and the reference matrices whose rows belong to the two
        # vectors (None: no reference matrix at hand, the residual parts are compared at their own scale only)
        self.sol, self.A_scale, self.A_tot = sol, (A if A_scale is None else A_scale), A_tot
        if A is not None:
            A.sort_indices()
            rows = np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(A.indptr))
            self.keys = rows * A.shape[1] + A.indices


def oracle_reference(c, residual_only):
    r, rp, ci = oracle(c, residual_only)
    A = None if residual_only else sp.csr_matrix((r.values, ci, rp), shape=(c.layout.n_dofs,) * 2)
    A_scale = reference_matrix(c) if residual_only else A  # (residual-only: one oracle Jacobian of the case for the scales)
    return Reference(c.layout, A, r.residual_pde, r.residual_total, c.sol, A_scale, total_matrix(c, A_scale))


def check_against_reference(rank, W, residual_only, ref):
    """every owned row of W: the same entries as the reference's row, values within TOL"""
    lp, ctx, glay = rank.lp, rank.ctx, ref.layout
    dim, no, gi = glay.dim, lp.n_owned, lp.global_ids
    nc = dim + 1
    nn, cc = np.repeat(np.arange(no), nc), np.tile(np.arange(nc), no)
    ld = M.DofLayout(no, dim, glay.blocked).dof(nn, cc)
    gd = glay.dof(gi[nn], cc)  # the global rows this rank owns
    res = W[-2:] if residual_only else W[-1:]
    assert linf_scaled(res[0][ld], ref.res_pde[gd]) < TOL
    _rows_at_their_scale(res[0][ld], ref.res_pde[gd], ref, ref.A_scale, gd, cc == dim, f"rank {rank.index} residual_pde")
    if residual_only:
        assert linf_scaled(res[1][ld], ref.res_tot[gd]) < TOL
        _rows_at_their_scale(res[1][ld], ref.res_tot[gd], ref, ref.A_tot, gd, cc == dim, f"rank {rank.index} residual_total")
        return
    keys, vals = [], []
    for b in range(ctx.n_blocks):
        rp, ci = ctx.pattern(b)
        if glay.blocked:
            ncr, cr0 = (dim, 0) if b in (0, 1) else (1, dim)
            ncc, cc0 = (dim, 0) if b in (0, 2) else (1, dim)
        else:
            ncr = ncc = nc
            cr0 = cc0 = 0
        assert rp.size - 1 == no * ncr
        lr = np.repeat(np.arange(rp.size - 1), np.diff(rp))
        grow = glay.dof(gi[lr // ncr], cr0 + lr % ncr).astype(np.int64)
        gcol = glay.dof(gi[ci // ncc], cc0 + ci % ncc).astype(np.int64)
        keys.append(grow * ref.A.shape[1] + gcol)
        vals.append(W[b])
    keys, vals = np.concatenate(keys), np.concatenate(vals)
    # the rows' column sets: every local entry is an entry of an owned global row, no entry twice, none missing
    assert np.unique(keys).size == keys.size
    assert keys.size == int(np.diff(ref.A.indptr)[gd].sum())
    pos = np.minimum(np.searchsorted(ref.keys, keys), ref.keys.size - 1)
    assert (ref.keys[pos] == keys).all()
    assert linf_scaled(vals, ref.A.data[pos]) < TOL
    # the owned rows' entries at the scales of the global reference: d = diag(ref.A) over the global dofs, each block at its own
    grow, gcol = keys // ref.A.shape[1], keys % ref.A.shape[1]
    blk = PS.block_of_entries(glay, grow, gcol)
    for b in range(4):
        m = blk == b
        if ref.sol is not None:  # a reference proper: per entry and per block
            PS.assert_rank_block(vals[m], ref.A.data[pos][m], ref.A.diagonal(), grow[m], gcol[m], PS.BLOCKS[b], TOL, f"rank {rank.index}, owned rows")
        else:  # ref is another GPU path: the block at its own scale only
            PS.assert_blocks([vals[m]], [ref.A.data[pos][m]], TOL, f"rank {rank.index}, owned rows", [PS.BLOCKS[b]])


def _rows_at_their_scale(v, want, ref, A, gd, phi_rows, tag):
    """owned rows of a rank: per part always, per row where the reference carries its matrix and solution"""
    if A is not None and ref.sol is not None:
        PS.assert_rank_rows(v, want, A, ref.layout, ref.sol, gd, TOL, tag)
    else:
        PS.assert_parts(v, want, phi_rows, TOL, tag)


# ---- the protocol -------------------------------------------------------------------------------------------------------
def _other_state(buf, lp, dim):
    """the same messages with a different valid state: u + 1/2, every phase field f -> 1 - f"""
    b = buf.clone()
    rec = dim + 3
    for k in range(len(lp.peers)):
        m = int(lp.recv_ptr[k + 1] - lp.recv_ptr[k])
        o = int(lp.recv_ptr[k]) * rec
        b[o:o + dim * m] += 0.5
        b[o + dim * m:o + rec * m] = 1.0 - b[o + dim * m:o + rec * m]
    return b


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def placeholder_diagonals(rank):
    """(u,u) diagonal entries of the constrained displacement rows.  Where an element diagonal vanished (kappa = 0 in a
    dead zone) k_cart_phi4 adds deal.II's placeholder, the mean |diagonal| of the element, to them; it runs in phase 2,
    so phase 1 leaves these entries unfinished (and step 3 checks what phase 2 makes of them)."""
    ctx = rank.ctx
    rp, ci = ctx.pattern(0)
    nr = ctx.dim if ctx.blocked else ctx.dim + 1
    lr = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    node, c = lr // nr, lr % nr
    return (ci == lr) & (c < ctx.dim) & (((rank.flags[node].astype(np.int64) >> c) & 1) == 1)


def run_phases(rank, recv, residual_only, ref, unfinished=None, exact=True):
    """steps 1-4 for one rank; returns (W, what phase 1 left) as lists of host arrays: the value blocks and res_pde of a
    full assembly, res_pde and res_tot of a residual-only one.  unfinished: entries of block 0 that phase 1 may leave
    different from W (full assemblies); exact = False: phase 2 and the repeated whole assembly equal W to round-off only"""
    import torch

    ctx, lp, dim = rank.ctx, rank.lp, rank.ctx.dim
    z = lambda k: torch.empty(k, dtype=torch.float64, device="cuda")
    vals = [] if residual_only else [z(ctx.pattern_size(b)[1]) for b in range(ctx.n_blocks)]
    res = [z(ctx.n_owned_dofs), z(ctx.n_owned_dofs)]
    outs = res if residual_only else vals + res[:1]

    def unpack(buf):
        if buf.numel():
            ctx.halo_unpack_all(buf.data_ptr())
        torch.cuda.synchronize()

    def run(phase, fill=True):
        ctx.force_phase(phase)
        if fill:
            for o in outs:
                o.fill_(SENT)
        ctx.assemble_device(residual_only, [v.data_ptr() for v in vals], res[0].data_ptr(), res[1].data_ptr())
        ctx.sync_status()
        return [o.cpu().numpy().copy() for o in outs]

    tag = f"rank {rank.index} ({'residual only' if residual_only else 'full'})"
    unpack(recv)
    W = run(0)
    for k, w in enumerate(W):
        assert not (w == SENT).any(), f"{tag}: the whole assembly left entries of output {k} unwritten"
    check_against_reference(rank, W, residual_only, ref)
    for poison in (torch.full_like(recv, float("nan")), _other_state(recv, lp, dim)):
        unpack(poison)
        p1 = run(1)
        for k, (a, w) in enumerate(zip(p1, W)):
            bad = ~((a == SENT) | (a.view(np.int64) == w.view(np.int64)))
            if k == 0 and unfinished is not None and not residual_only:
                bad &= ~unfinished
            assert not bad.any(), f"{tag}: phase 1 wrote {int(bad.sum())} entries of output {k} that differ from W (ghost read)"
    unpack(recv)
    p2 = run(2, fill=False)
    for k, (a, w) in enumerate(zip(p2, W)):
        assert _equal(a, w, exact), (f"{tag}: phase 1 + phase 2 differ from the whole assembly in output {k}: "
                                     f"{int((a != w).sum())} entries, |dx|_inf = {linf_scaled(a, w):.2e}")
    again = run(0)
    assert all(_equal(a, w, exact) for a, w in zip(again, W)), f"{tag}: force_phase(0) does not restore the whole assembly"
    return W, p1


def _equal(a, w, exact):
    if exact:
        return _same_bits(a, w)
    return a.shape == w.shape and not (a == SENT).any() and linf_scaled(a, w) < TOL


def _share(a, mask=None):
    w = a != SENT
    if mask is not None:
        w = w[mask]
    return float(w.mean()) if w.size else 1.0


def _uu_mask(ctx):
    """entries of the (u,u) rows and columns of the single block of the interleaved layout"""
    nc = ctx.dim + 1
    rp, ci = ctx.pattern(0)
    lr = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    return (lr % nc < ctx.dim) & (ci % nc < ctx.dim)


def run_partition(ranks, refs, cut=None, general=False, unfinished=None, exact=True):
    """the protocol on every rank, full and residual-only; cut(rank, residual_only) -> [(output index, entry mask)] of
    the cut kernel's outputs that phase 1 must mostly write; unfinished(rank) -> the entries of block 0 that phase 1 may
    leave unfinished"""
    dim = ranks[0].ctx.dim
    recv = exchange_ghosts([r.lp for r in ranks], [r.ctx for r in ranks], dim)
    for residual_only in (False, True):
        for rank, buf in zip(ranks, recv):
            W, p1 = run_phases(rank, buf, residual_only, refs[residual_only], unfinished and unfinished(rank), exact)
            if general:
                assert all((a == SENT).all() for a in p1), "the general family and the overlays write nothing in phase 1"
            for k, mask in (cut(rank, residual_only) if cut else []):
                s = _share(p1[k], mask)
                assert s > 0.5, f"phase 1 wrote only {s:.2f} of output {k} of the cut kernel"


# ---- 3-D cartesian --------------------------------------------------------------------------------------------------------
# (grid, global cells, large: every rank long enough for interior tiles of every cut kernel -- z-slabs of ~30 planes,
# residual z-chunks of 4).  Partial tiles in x and y throughout (T3X x T3Y = 8 x 4, RNX x RNY = 15 x 15); (3,1,1): ghosts on
# both x faces of the middle rank; (2,2,2): ghost edges and corners; (1,1,4): two planes per inner rank, no interior tile
GRIDS3 = [((2, 1, 1), (21, 6, 7), False), ((3, 1, 1), (30, 6, 7), False), ((1, 1, 3), (9, 6, 36), False),
          ((2, 2, 2), (17, 9, 12), False), ((1, 1, 4), (9, 5, 8), False), ((1, 1, 2), (9, 8, 60), True)]


@pytest.mark.parametrize("blocked", [True, False])
@pytest.mark.parametrize("kind", ["stag", "mono", "het", "dead"])
@pytest.mark.parametrize("p,n,large", GRIDS3)
def test_cart3d_phases(p, n, large, kind, blocked):
    c = global_case(3, n, kind, blocked)
    refs = {ro: oracle_reference(c, ro) for ro in (False, True)}
    ranks = box_ranks(c, n, p)

    def cut(rank, residual_only):
        if not large:
            return []
        if residual_only:
            return [(0, None), (1, None)]
        if kind in ("mono", "het"):  # the quadrature residual kernel is cut, the Jacobian waits for phase 2
            return [(rank.ctx.n_blocks, None)]
        return [(0, None if blocked else _uu_mask(rank.ctx))]  # k_cart_uu3 is cut, k_cart_phi4 follows in phase 2

    # staggered: the placeholders of the dead zone are k_cart_phi4's, in phase 2
    run_partition(ranks, refs, cut, unfinished=placeholder_diagonals if kind in ("stag", "dead") else None)


# ---- 2-D cartesian --------------------------------------------------------------------------------------------------------
# k_cart2d_cells filters per node (blocks of O2 = 7), k_cart_residual2m per wave (62 node columns x 4 rows); (6,1): two
# node columns per inner rank, every one next to a ghost
GRIDS2 = [((2, 1), (40, 30), False), ((1, 3), (30, 60), False), ((2, 2), (40, 30), False), ((6, 1), (12, 20), False),
          ((1, 2), (60, 140), True)]


@pytest.mark.parametrize("blocked", [True, False])
@pytest.mark.parametrize("kind", ["dead", "mono_dead", "het", "flat"])
@pytest.mark.parametrize("p,n,large", GRIDS2)
def test_cart2d_phases(p, n, large, kind, blocked):
    """both launches of k_cart2d_cells are cut: the mean |diagonal| goes from the first to the second through
    CartView::cell_avg within each phase, the (u,phi) block is cleared in phase 1"""
    c = global_case(2, n, kind, blocked)
    refs = {ro: oracle_reference(c, ro) for ro in (False, True)}
    ranks = box_ranks(c, n, p)

    def cut(rank, residual_only):
        if not large:
            return []
        return [(k, None) for k in range(2 if residual_only else rank.ctx.n_blocks + 1)]

    run_partition(ranks, refs, cut)


# ---- general family, overlays --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocked", [True, False])
@pytest.mark.parametrize("kind", ["stag", "dead"])
def test_box_partition_on_the_general_family(kind, blocked):
    n = (9, 5, 6)
    c = global_case(3, n, kind, blocked)
    refs = {ro: oracle_reference(c, ro) for ro in (False, True)}
    ranks = box_ranks(c, n, (2, 1, 1))
    for r in ranks:
        r.ctx.force_path(0)
    run_partition(ranks, refs, general=True)


@pytest.mark.parametrize("kind,world", [("slit2d", 3), ("box3d", 2)])
def test_general_partition_phases(kind, world):
    """the general partitions of test_gpu_multirank (hanging nodes; 2-D: general family + cartesian overlay), against
    the single-rank assembly of the whole mesh"""
    import cases
    from cracks_amd.capi import PfmParams
    from test_partition_halo import _amr_fields, amr_mesh

    g = amr_mesh(kind)
    dim, N = g.dim, g.n_nodes
    f = _amr_fields(g, dim)
    for k, nd in enumerate(g.hn_nodes):  # nodal fields with the hanging-node constraints distributed
        sl = slice(g.hn_ptr[k], g.hn_ptr[k + 1])
        f[nd] = (g.hn_weights[sl, None] * f[g.hn_parents[sl]]).sum(axis=0)
    base = cases.kat_sneddon_3d(4) if dim == 3 else cases.kat_miehe_shear_1()
    prm = PfmParams.from_buffer_copy(bytes(base.params))
    if dim == 2:
        prm.decompose_stress_rhs = prm.decompose_stress_matrix = 1.0
        prm.timestep_number = 3
    glay = M.DofLayout(N, dim, blocked=True)
    dirichlet = M.sneddon_dirichlet_dofs if dim == 3 else M.miehe_shear_dirichlet_dofs
    gcu = M.update_constraints(g, glay, dirichlet(g, glay))
    gch = M.hanging_constraints(g, glay)
    gflags = node_flags_from_dof_flags(glay, gcu.flag, gch.flag)
    zero_u = np.zeros((N, dim))
    nodal = [np.column_stack([f[:, :dim], f[:, dim]]), np.column_stack([zero_u, f[:, dim + 1]]),
             np.column_stack([zero_u, f[:, dim + 2]])]

    ref = Context(g, True)
    ref.set_params(prm)
    ref.set_constraints(gflags)
    vecs = [_local_vector(F, np.arange(N), True) for F in nodal]
    refs = {}
    for ro in (False, True):
        values, r_pde, r_tot = ref.assemble_host(*vecs, residual_only=ro)
        A = None if ro else blocks_to_global(ref, glay, values)
        refs[ro] = Reference(glay, A, r_pde, r_tot)
    ranks = [_rank(r, lp, True, prm, gflags, nodal) for r, lp in enumerate(P.partition_general(g, world, ghost_layer="closure"))]
    # 2-D: the cells at hanging vertices add to their rows with FP64 atomics (the atomic class of the general family), in
    # an order that changes from run to run -- results agree to round-off, not bit for bit (pfm_assemble_overlapped
    # promises bits on uniform boxes); 3-D gathers them in list order
    run_partition(ranks, refs, general=True, exact=dim == 3)
