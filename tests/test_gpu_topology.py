"""The general cell kernels on the mesh topologies that reach their fallbacks (tests/topology_cases.py; that the cases do
reach them is asserted on the inputs by tests/test_topology_cases.py):

  colour overflow (a node of more than 62 cells: the atomic class, every cell adds atomically)   fan2d_closed64, fan3d_41
  node-graph row of exactly 254 neighbours, last uint8 slot 253                                  fan2d_open126
  node-graph row of 255 neighbours: PFM_ERR_UNSUPPORTED, the process stays usable                fan2d_closed127, fan3d_42
  find_slot row search (a hanging node with more parents than DevView::cslot_h holds)            hang2d_3parents, hang3d_5parents
  no reduced record (R = 0xff: more than 16 resolved nodes), gather given up                     hang3d_17resolved
  slow branch of k_hanging_gather (gathered entries into a row of more than 64 neighbours)       fan3d_30_hanging
  colour overflow next to the ordered gather (cells without a colour beside the scratch class)   fan3d_41_hanging

Every entry against the CPU oracle at the project's parity bar: l_inf error < 1e-12, scaled by max(1, |reference|_inf)."""
import numpy as np
import pytest

import topology_cases as T
from cracks_amd.capi import PfmError
from gpu_util import TOL, full_parity, make_context, oracle, reference_matrix, total_matrix

pytestmark = pytest.mark.gpu

MODES = ["default", "PFM_HANGING_ATOMIC", "PFM_HANGING_COLOURED"]


def parity_on_the_general_family(c, tol=TOL, prepare=None):
    """Parity of a new context of the case as it chooses to run, and -- should a cartesian overlay have taken the regular
    rows of a refined box mesh -- once more through the general family alone.  prepare(ctx): called before the first assembly."""
    ctx = make_context(c)
    if prepare:
        prepare(ctx)
    full_parity(c, tol, ctx)
    if ctx.kernel_path != 0:
        ctx.force_path(0)
        full_parity(c, tol, ctx)
    assert ctx.kernel_path == 0
    ctx.close()


@pytest.mark.parametrize("blocked", [True, False])
@pytest.mark.parametrize("make", T.ACCEPTED, ids=lambda f: f.__name__)
def test_accepted_topologies_match_the_oracle(make, blocked):
    parity_on_the_general_family(make(blocked))


@pytest.mark.parametrize("make", [T.fan2d_closed64, T.fan2d_open126, T.fan3d_41], ids=lambda f: f.__name__)
def test_fans_run_on_the_general_family_unasked(make):
    ctx = make_context(make())
    assert ctx.kernel_path == 0 and ctx.overlay_info()[0] == 0
    ctx.close()


def test_rows_of_255_are_refused_and_the_process_stays_usable():
    """Status 5 from the node-graph build (gather_row bounds its private row at MAX_ROW + 1 entries: a status, not a
    fault); afterwards, in the same process, the row of exactly 254 is still built and passes parity: the scratch of the
    refused builds was released and nothing is left half-built."""
    for make in T.REFUSED:
        for blocked in (True, False):
            with pytest.raises(PfmError) as ei:
                make_context(make(blocked))
            assert ei.value.status == 5 and "254 neighbours" in str(ei.value)
    parity_on_the_general_family(T.fan2d_open126())


@pytest.mark.parametrize("make", [T.fan2d_closed64, T.fan3d_41], ids=lambda f: f.__name__)
def test_colour_overflow_with_the_monolithic_penalty(make):
    c = make()
    c.params.outer_solver = 1
    c.params.gamma_penal = 10.0
    c.params.timestep_number = 2
    parity_on_the_general_family(c)


def test_colour_overflow_with_the_stress_split():
    """fan2d_closed64 with the 2-D stress split on, in the shape of test_gpu_cart.test_cart2d_split_runs_stay_on_the_general_
    family and at its bar: the spectral decomposition of the strain is the one place where the kernel's and the oracle's
    operation orders differ by more than summation order."""
    c = T.fan2d_closed64(False)
    c.params.decompose_stress_matrix = 1.0
    c.params.decompose_stress_rhs = 1.0
    c.params.timestep_number = 2
    parity_on_the_general_family(c, tol=1e-11)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("make", [T.hang3d_5parents, T.hang3d_17resolved, T.fan3d_30_hanging, T.fan3d_41_hanging], ids=lambda f: f.__name__)
def test_hanging_3d_topologies_in_every_mode(make, mode, monkeypatch):
    """The three ways the hexes at hanging vertices reach the outputs (read by pfm_ctx_create): five parents leave no slot
    table and no reduced records in any mode; 17 resolved nodes make the default give the gather up and keep the cell in the
    last class under PFM_HANGING_COLOURED; the long pole row takes gathered entries one by one in the default mode, in
    fan3d_41_hanging next to the atomic adds of the cells that found no colour."""
    if mode != "default":
        monkeypatch.setenv(mode, "1")
    parity_on_the_general_family(make())


def test_colour_overflow_next_to_the_gather_every_time():
    """fan3d_41_hanging in the default mode: the cells that found no colour add atomically from the side stream while the
    colour classes run, so the colour classes must add atomically too (pfm_dispatch.cpp: general_view keeps DevView::cell_ring
    when colours overflowed).  Plain read-modify-writes next to those atomics lose an update now and then, not every
    time: twenty Jacobians on one context, each against the oracle."""
    import scipy.sparse as sp

    from gpu_util import blocks_to_global, linf_scaled, reference_parity

    c = T.fan3d_41_hanging()
    r, rp, ci = oracle(c, False)
    A_ref = sp.csr_matrix((r.values, ci, rp), shape=(c.layout.n_dofs,) * 2)
    ctx = make_context(c)
    assert ctx.kernel_path == 0
    for _ in range(20):
        values, res, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
        A = blocks_to_global(ctx, c.layout, values)
        A.sort_indices()
        assert (A.indices == A_ref.indices).all()
        assert linf_scaled(A.data, A_ref.data) < TOL and linf_scaled(res, r.residual_pde) < TOL
        reference_parity(c.layout, c.sol, A, A_ref, [(res, r.residual_pde, "pde")], tag="topology, long rows")
    ctx.close()


def test_gather_into_a_long_row_is_bitwise_reproducible():
    """README: the ordered gather sums in list order; the slow branch of k_hanging_gather keeps that order."""
    c = T.fan3d_30_hanging()
    runs = []
    for k in range(2):
        ctx = make_context(c)
        for _ in range(2 - k):
            values, res, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
            runs.append([v.copy() for v in values] + [res.copy()])
        ctx.close()
    assert len(runs) == 3
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a.shape == b.shape and (a.view(np.int64) == b.view(np.int64)).all()


@pytest.mark.parametrize("make", [T.fan2d_open126, T.hang2d_3parents, T.hang3d_5parents, T.fan3d_30_hanging], ids=lambda f: f.__name__)
def test_bound_patterns_with_shuffled_rows(make):
    """pfm_pattern_bind of a host pattern with the neighbour nodes of every row in a seeded random order: the slot tables,
    find_slot and the reduced records read the rows in the bound order (blocks_to_global maps the values back through the
    pattern the context reports, i.e. the bound one)."""
    from test_gpu_pattern import _permuted_patterns

    c = make()

    def bind(ctx):
        pats = _permuted_patterns(ctx, c.mesh.dim, True, seed=11)
        for b, (rp, ci, _) in enumerate(pats):
            ctx.pattern_bind(b, rp, ci)
        for b, (rp, ci, _) in enumerate(pats):
            rp2, ci2 = ctx.pattern(b)
            assert (rp2 == rp).all() and (ci2 == ci).all()
        assert any((np.diff(ci[rp[r]:rp[r + 1]]) < 0).any() for rp, ci, _ in pats[3:] for r in range(rp.size - 1))

    parity_on_the_general_family(c, prepare=bind)


@pytest.mark.parametrize("blocked", [True, False])
def test_colour_overflow_on_a_partition_along_z(blocked):
    """fan3d_41 cut into its two layers, both contexts on one device: rank 0 owns the two lower planes and has the top
    plane as ghosts -- the pole row of 249 ends in ghost columns --, rank 1 owns the top plane.  Owned rows against the
    oracle's."""
    import scipy.sparse as sp
    import torch

    from cracks_amd import partition as P
    from cracks_amd.assembler import node_flags_from_dof_flags
    from gpu_util import exchange_ghosts
    from test_gpu_overlap_phases import Reference, _rank, check_against_reference

    c = T.fan3d_41(blocked)
    g, dim = c.mesh, 3
    layer = (np.arange(g.n_cells) >= g.n_cells // 2).astype(np.int64)
    assert (g.coords[g.cells[layer == 1]][:, :, 2].min(axis=1) > 0).all()
    lps = P.partition_general(g, 2, cell_rank=layer)
    n_plane = g.n_nodes // 3
    assert [lp.n_owned for lp in lps] == [2 * n_plane, n_plane] and lps[0].mesh.n_nodes == 3 * n_plane
    node, comp = c.layout.node_comp_of_dof()
    nodal = []
    for v in (c.sol, c.old, c.oldold):
        F = np.empty((g.n_nodes, dim + 1))
        F[node, comp] = v
        nodal.append(F)
    flags = node_flags_from_dof_flags(c.layout, c.cu.flag, c.ch.flag)
    ranks = [_rank(r, lp, blocked, c.params, flags, nodal) for r, lp in enumerate(lps)]
    recv = exchange_ghosts(lps, [r.ctx for r in ranks], dim)
    for residual_only in (False, True):
        r, rp, ci = oracle(c, residual_only)
        A = None if residual_only else sp.csr_matrix((r.values, ci, rp), shape=(c.layout.n_dofs,) * 2)
        A_scale = A if A is not None else reference_matrix(c)
        ref = Reference(c.layout, A, r.residual_pde, r.residual_total, c.sol, A_scale, total_matrix(c, A_scale))
        for rank, buf in zip(ranks, recv):
            ctx = rank.ctx
            assert ctx.kernel_path == 0
            if buf.numel():
                ctx.halo_unpack_all(buf.data_ptr())
            z = lambda k: torch.full((k,), np.nan, dtype=torch.float64, device="cuda")
            vals = [] if residual_only else [z(ctx.pattern_size(b)[1]) for b in range(ctx.n_blocks)]
            res = [z(ctx.n_owned_dofs), z(ctx.n_owned_dofs)]
            ctx.assemble_device(residual_only, [v.data_ptr() for v in vals], res[0].data_ptr(), res[1].data_ptr())
            ctx.sync_status()
            W = [o.cpu().numpy() for o in (res if residual_only else vals + res[:1])]
            assert all(np.isfinite(w).all() for w in W)
            check_against_reference(rank, W, residual_only, ref)
    # the pole row of rank 0: 249 entries, the 83 ghost columns last
    pole = int(np.nonzero(lps[0].global_ids == c.extra["pole"])[0][0])
    rp, ci = ranks[0].ctx.pattern(ranks[0].ctx.n_blocks - 1)
    nc = 1 if blocked else dim + 1
    row = ci[rp[pole * nc + nc - 1]:rp[pole * nc + nc]] // nc
    cols = row[::nc] if not blocked else row
    assert cols.size == 249 and (cols[-n_plane:] >= lps[0].n_owned).all() and (cols[:-n_plane] < lps[0].n_owned).all()
    for r in ranks:
        r.ctx.close()
