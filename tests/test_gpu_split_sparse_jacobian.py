"""The sparse volumetric-deviatoric split Jacobian (pfm_set_split_route with PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE = 21 or
PFM_SPLIT_ROUTE_LATTICE_ALL_SPARSE = 23; CartPlan::voldev_sparse): k_cart_split3_mark, the unsplit k_cart_uu3 and k_cart_phi4 over
the whole box, then the sparse form of k_cart_split3_jac over the rows at compressed cells, through the C ABI:

1. the interface: 21 and 23 accepted, every other value with bit 16 refused, 2-D, what pfm_ctx_split_sparse_info and
   pfm_ctx_split_route_info answer before and after pfm_set_params, under forced path 0 and under models 0 / 1;
2. the origin of every row, byte for byte: a row of a node that touches a compressed cell is route 5's, every other row is
   the unsplit assembly's (decompose_stress_matrix = 0) on the same living context; residual_pde is route 5's and the
   residual-only call's; the counts; two z-chunk lengths, repeats, a fresh context;
3. the bar: the corner states, the mixed boxes and the dead zone against the numpy reference and the general route;
4. one-sided states: tension recomputes no row and is the unsplit oracle's matrix, compression recomputes every row;
5. two ranks on one GPU, both halves of the overlapped assembly, both layouts;
6. an overlay context keeps the general family;
7. one living context through unsplit -> 21 -> unsplit -> 5 -> 23 -> model 1 -> model 3 -> 0.

States and the conditions on them: tests/split_sparse_cases.py (run on the CPU by tests/test_split_sparse_ref_cpu.py).  Bar:
1e-12 (gpu_util.TOL) on the whole matrix and on the four checks of tests/parity_scale.py, as in
tests/test_gpu_split_lattice_jacobian.py; reference: split_voldev_ref.element_matrices."""
import numpy as np
import pytest
import scipy.sparse as sp

import cases
import split_jacobian_cases as JC
import split_lattice_cases as LC
import split_sparse_cases as XC
import split_voldev_cases as SC
from cracks_amd import capi
from cracks_amd import mesh as M
from cracks_amd.assembler import node_flags_from_dof_flags
import parity_scale as PS
from gpu_util import TOL, full_parity, linf_scaled, make_context, oracle, reference_parity, total_matrix
from test_gpu_split3d import _copy, _matrix
from test_gpu_split_lattice_jacobian import PFM_ZC_UU3, _bytes, _context, _full, _residuals, against_general, check

pytestmark = pytest.mark.gpu

GENERAL, LATTICE, ANY = capi.SPLIT_ROUTE_GENERAL, capi.SPLIT_ROUTE_LATTICE, capi.SPLIT_ROUTE_LATTICE_ANY
JAC, ALL = capi.SPLIT_ROUTE_LATTICE_JACOBIAN, capi.SPLIT_ROUTE_LATTICE_ALL
SPARSE, ALL_SPARSE = capi.SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE, capi.SPLIT_ROUTE_LATTICE_ALL_SPARSE


def _nodes_of_rows(ctx, b):
    """node of every entry of value block b (blocked: three rows per node in the (u,.) blocks, one in the (phi,.) blocks;
    interleaved: four)"""
    rp, _ = ctx.pattern(b)
    per = (3 if b in (0, 1) else 1) if ctx.blocked else 4
    return np.repeat(np.arange(rp.size - 1), np.diff(rp)) // per


def _unsplit_params(c):
    return _copy(c.params, decompose_stress_matrix=0.0)


def assert_row_origins(ctx, touched, v21, v5, v0, tag):
    """every entry of every block: the bits of route 5 in the rows of touched nodes, of the unsplit assembly elsewhere"""
    n5 = n0 = 0
    for b in range(ctx.n_blocks):
        t = touched[_nodes_of_rows(ctx, b)]
        a, w5, w0 = (np.ascontiguousarray(x).view(np.int64) for x in (v21[b], v5[b], v0[b]))
        assert a.shape == w5.shape == w0.shape == t.shape
        bad5, bad0 = t & (a != w5), ~t & (a != w0)
        assert not bad5.any(), f"{tag}: block {b}: {int(bad5.sum())} entries of touched rows are not route 5's bytes"
        assert not bad0.any(), f"{tag}: block {b}: {int(bad0.sum())} entries of untouched rows are not the unsplit kernels' bytes"
        n5, n0 = n5 + int((t & (w5 != w0)).sum()), n0 + int((~t & (w5 != w0)).sum())
    return n5, n0  # entries in which the two origins differ, by kind of row


# ---------------------------------------------------------------- 1
def test_interface_refusals_and_what_the_info_calls_answer():
    c = XC.corner((5, 4, 3))
    off = LC.unsplit(c)
    assert (SPARSE, ALL_SPARSE) == (21, 23) == (JAC | 16, ALL | 16)
    never = LC_context_without_params(c)
    assert never.split_sparse_info() == (0, -1, -1, 0)  # before pfm_set_params
    never.set_split_route(SPARSE)  # (raises PFM_ERR_BAD_ARG without the feature)
    assert never.split_route == SPARSE and never.split_route_plan() == (SPARSE, 0, 0, -1) and never.split_sparse_info() == (0, -1, -1, 0)
    never.set_split_route(ALL_SPARSE)
    assert never.split_route == ALL_SPARSE
    never.set_split_route(GENERAL)
    for refused in [16, 17, 18, 19, 20, 22] + list(range(24, 32)) + [32, 37, 53]:
        with pytest.raises(capi.PfmError) as e:
            never.set_split_route(refused)
        assert e.value.status == 1 and never.split_route == GENERAL, refused
    never.close()
    # 2-D answers PFM_ERR_UNSUPPORTED, as for every lattice route
    c2 = cases.kat_miehe_shear_1()
    ctx2 = make_context(c2)
    for route in (SPARSE, ALL_SPARSE):
        with pytest.raises(capi.PfmError) as e:
            ctx2.set_split_route(route)
        assert e.value.status == 5 and ctx2.split_route == GENERAL
    with pytest.raises(capi.PfmError) as e:
        ctx2.set_split_route(29)
    assert e.value.status == 1
    assert ctx2.split_sparse_info() == (0, -1, -1, 0)
    ctx2.close()
    # (route, residual-only on the lattice, full assembly on the lattice, sparse) by route, model, split and forced path
    ctx = _context(c, route=None)
    for route in (GENERAL, LATTICE, JAC, ALL, SPARSE, ALL_SPARSE):
        ctx.set_split_route(route)
        for model in (capi.SPLIT_REFERENCE, capi.SPLIT_SPECTRAL, capi.SPLIT_VOLDEV):
            ctx.set_split_model(model)
            for split in (True, False):
                if model == capi.SPLIT_REFERENCE and split:
                    continue  # (pfm_set_params refuses the 3-D split under model 0)
                ctx.set_params(c.params if split else off.params)
                for path in (0, 1):
                    ctx.force_path(path)
                    on = split and path == 1
                    res = int(on and ((model == capi.SPLIT_VOLDEV and route & 1) or (model == capi.SPLIT_SPECTRAL and (route & 3) == 3)))
                    jac = int(on and model == capi.SPLIT_VOLDEV and (route & 4) == 4)
                    sparse = int(jac and (route & 16) == 16)
                    assert ctx.split_route_plan()[:3] == (route, res, jac), (route, model, split, path)
                    info = ctx.split_sparse_info()
                    assert info[0] == sparse and info[1:3] == (-1, -1) and (info[3] > 0) == bool(sparse), (route, model, split, path, info)
    ctx.close()
    # split_route_plan() under 21 is that of 5, but for the route -- also after an assembly
    plans = {}
    for route in (JAC, SPARSE):
        ctx = _context(c, route=route)
        before = ctx.split_route_plan()
        _full(ctx, c)
        plans[route] = (before[1:], ctx.split_route_plan()[1:])
        assert ctx.split_route_plan()[0] == route
        ctx.close()
    assert plans[SPARSE] == plans[JAC] and plans[JAC][1][2] == XC.COUNTS[(5, 4, 3)][0]


def LC_context_without_params(c):
    from cracks_amd.assembler import Context

    ctx = Context(c.mesh, True, cell_lambda=c.cell_lambda, cell_mu=c.cell_mu)
    ctx.set_split_model(capi.SPLIT_VOLDEV)
    return ctx


# ---------------------------------------------------------------- 2
def test_the_origin_of_every_row_byte_for_byte():
    shape = (17, 16, 5)
    c = XC.corner(shape, "lame")
    cells, _, rows, n_nodes, _ = XC.COUNTS[shape]
    touched = XC.touched_rows(c)
    assert touched.sum() == rows and touched.size == n_nodes == c.mesh.n_nodes
    ctx = _context(c, route=SPARSE)
    assert ctx.kernel_path == 1 and ctx.split_route_plan() == (SPARSE, 1, 1, -1) and ctx.split_sparse_info()[:3] == (1, -1, -1)
    v21, r21 = _full(ctx, c)
    info21, plan21 = ctx.split_sparse_info(), ctx.split_route_plan()
    assert _bytes(_residuals(ctx, c)[0]) == _bytes(r21), "residual_pde of the Jacobian call is the residual-only call's"
    assert ctx.split_sparse_info() == info21  # (a residual-only call leaves the counts of the last full assembly)
    ctx.set_split_route(JAC)
    assert ctx.split_sparse_info()[0] == 0
    v5, r5 = _full(ctx, c)
    plan5 = ctx.split_route_plan()
    assert ctx.split_sparse_info()[1:3] == (-1, -1), "the last full assembly did not run sparse"
    assert _bytes(r21) == _bytes(r5), "residual_pde under 21 is route 5's"
    assert plan21 == (SPARSE, 1, 1, cells) and plan5 == (JAC, 1, 1, cells)
    assert info21[0] == 1 and info21[1] == rows and 0 < info21[2] <= info21[3]
    # the unsplit assembly on the same living context: per-cell Lame, so no pair and no residual rows -- step 3's instantiations
    ctx.set_params(_unsplit_params(c))
    assert ctx.split_route_plan()[:3] == (JAC, 0, 0)
    v0, _ = _full(ctx, c)
    n5, n0 = assert_row_origins(ctx, touched, v21, v5, v0, c.name)
    print(f"split_sparse {c.name}: route 5 and the unsplit assembly differ in {n5} entries of touched rows, {n0} of the others")
    assert n5 > 0, "the state tells the two origins apart"
    first = _bytes(*v21, r21)
    # any z-chunk length: the flagged tile-chunks of tests/split_sparse_cases.py, the same bytes; twice
    ctx.set_params(c.params)
    ctx.set_split_route(SPARSE)
    for zc, (flagged, total, _) in XC.TILE_CHUNKS.items():
        ctx.force_zchunk(PFM_ZC_UU3, zc)
        info = ctx.split_sparse_info()  # ([1], [2]: still of the last sparse assembly; [3]: of the grid of the next one)
        assert ctx.zchunk(PFM_ZC_UU3) == zc and (info[0], info[3]) == (1, total)
        for _ in range(2):
            assert _bytes(*_full(ctx, c)[0], _full(ctx, c)[1]) == first, zc
            assert ctx.split_sparse_info() == (1, rows, flagged, total) and ctx.split_route_plan()[3] == cells
    ctx.force_zchunk(PFM_ZC_UU3, 0)
    assert _bytes(*_full(ctx, c)[0], _full(ctx, c)[1]) == first
    ctx.set_split_route(ALL_SPARSE)
    assert _bytes(*_full(ctx, c)[0], _full(ctx, c)[1]) == first
    ctx.close()
    fresh = _context(c, route=SPARSE)
    assert _bytes(*_full(fresh, c)[0], _full(fresh, c)[1]) == first
    assert fresh.split_sparse_info()[:2] == (1, rows)
    fresh.close()
    one = _context(c, route=LATTICE)
    assert _bytes(_residuals(one, c)[0]) == _bytes(r21)
    one.close()


# ---------------------------------------------------------------- 3
def _bar(c, ref):
    ctx = _context(c, route=SPARSE)
    assert ctx.kernel_path == 1 and ctx.split_route_plan()[:3] == (SPARSE, 1, 1) and ctx.split_sparse_info()[0] == 1
    values, res = check(f"sparse {c.name}", ctx, c, ref)  # ((u,phi): exact zeros)
    info = ctx.split_sparse_info()
    assert info[1] == int(XC.touched_rows(c).sum()) and ctx.split_route_plan()[3] == int(XC.compressed_cells(c).sum())
    against_general(f"sparse {c.name}", c, values, res)
    ctx.close()


@pytest.mark.parametrize("shape,kind", XC.CORNER_IDS, ids=[f"{s[0]}x{s[1]}x{s[2]}-{k}" for s, k in XC.CORNER_IDS])
def test_corner_states_against_the_numpy_reference_and_the_general_route(shape, kind):
    _bar(XC.corner(shape, kind), JC.ref(XC.corner, shape, kind))


@pytest.mark.parametrize("shape,kind", LC.BOX_IDS, ids=[f"{s[0]}x{s[1]}x{s[2]}-{k}" for s, k in LC.BOX_IDS])
def test_mixed_boxes_against_the_numpy_reference_and_the_general_route(shape, kind):
    _bar(LC.box_case(shape, kind), JC.ref(LC.box_case, shape, kind))


def test_dead_zone_against_the_numpy_reference_and_the_general_route():
    _bar(JC.dead_case(), JC.ref(JC.dead_case))


# ---------------------------------------------------------------- 4
def test_tension_recomputes_no_row_and_is_the_unsplit_oracle():
    c = LC.one_sided_case(+1)
    SC.assert_one_sided(c, +1)
    off = cases.Case(c.name, c.mesh, c.layout, _copy(c.params, decompose_stress_matrix=0.0, decompose_stress_rhs=0.0), c.sol, c.old, c.oldold,
                     c.cu, c.ch, None, c.cell_lambda, c.cell_mu)
    r, rowptr, colind = oracle(off, False)
    ctx = _context(c, route=SPARSE)
    assert ctx.split_route_plan()[:3] == (SPARSE, 1, 1)
    values, res = _full(ctx, c)
    A = _matrix(ctx, c, values)
    A_ref = sp.csr_matrix((r.values, colind, rowptr), shape=A.shape)
    assert A.nnz == A_ref.nnz and (A.indices == A_ref.indices).all()
    e = (linf_scaled(A.data, A_ref.data), linf_scaled(res, r.residual_pde))
    print(f"split_sparse {c.name} against the unsplit oracle: matrix {e[0]:.2e} residual {e[1]:.2e}")
    assert max(e) < TOL
    reference_parity(c.layout, c.sol, A, A_ref, [(res, r.residual_pde, "pde")], tag="split_sparse against the unsplit oracle",
                     A_tot=total_matrix(off, A_ref))
    info = ctx.split_sparse_info()
    assert info[:3] == (1, 0, 0) and info[3] > 0 and ctx.split_route_plan() == (SPARSE, 1, 1, 0)
    ctx.close()


def test_compression_everywhere_is_route_5():
    c = LC.one_sided_case(-1)
    SC.assert_one_sided(c, -1)
    ctx = _context(c, route=SPARSE)
    values, res = check(f"sparse {c.name}", ctx, c, JC.ref(LC.one_sided_case, -1))
    info = ctx.split_sparse_info()
    assert info[:2] == (1, c.mesh.n_nodes) and info[2] == info[3] > 0 and ctx.split_route_plan() == (SPARSE, 1, 1, c.mesh.n_cells)
    ctx.set_split_route(JAC)
    assert _bytes(*_full(ctx, c)[0], _full(ctx, c)[1]) == _bytes(*values, res), "every row touched: the bytes of route 5"
    ctx.close()


# ---------------------------------------------------------------- 5
@pytest.mark.parametrize("blocked", [True, False])
def test_two_ranks_and_both_halves_of_the_overlapped_assembly(blocked):
    """the corner state on (33, 5, 4) unit cells in two ranks along x, its block across the cut.  OP.run_phases: the whole
    assembly of each rank against the reference at the bar, phase 1 with poisoned ghosts writes only final values, phase 1 +
    phase 2 and the repeated whole assembly are the bytes of the whole assembly.  Then the owned rows of the touched nodes
    against the single rank, byte for byte."""
    import test_gpu_overlap_phases as OP

    from cracks_amd import partition as P

    c = XC.two_rank_corner(blocked)
    r = JC.ref(XC.two_rank_corner, blocked)
    ref = OP.Reference(c.layout, r.A, r.pde, None, c.sol)
    touched = XC.touched_rows(c)
    single = _context(c, route=SPARSE)
    values, res = check(c.name + " (one rank)", single, c, r)
    assert single.split_sparse_info()[1] == touched.sum()
    A1 = _matrix(single, c, values)
    single.close()
    off, n = LC.unsplit(c), LC.TWO_RANK_N
    node, comp = c.layout.node_comp_of_dof()
    nodal = []
    for v in (c.sol, c.old, c.oldold):
        F = np.empty((c.layout.n_nodes, 4))
        F[node, comp] = v
        nodal.append(F)
    flags = node_flags_from_dof_flags(c.layout, c.cu.flag, c.ch.flag)
    lps = [P.build_local_problem(3, n, (2, 1, 1), k, lo=0.0, hi=np.asarray(n, float)) for k in range(2)]
    ranks = [OP._rank(k, lp, blocked, off.params, flags, nodal) for k, lp in enumerate(lps)]
    for rk in ranks:
        rk.ctx.set_split_model(capi.SPLIT_VOLDEV)
        rk.ctx.set_split_route(SPARSE)
        rk.ctx.set_params(c.params)
        assert rk.lp.n_owned < rk.lp.mesh.n_nodes and rk.ctx.kernel_path == 1 and rk.ctx.split_route_plan()[:3] == (SPARSE, 1, 1)
        assert rk.ctx.split_sparse_info()[0] == 1
    recv = OP.exchange_ghosts([rk.lp for rk in ranks], [rk.ctx for rk in ranks], 3)
    counted = 0
    for rk, buf in zip(ranks, recv):
        W, p1 = OP.run_phases(rk, buf, False, ref)
        ctx, no, gi, glay = rk.ctx, rk.lp.n_owned, rk.lp.global_ids, c.layout
        nn, cc = np.repeat(np.arange(no), 4), np.tile(np.arange(4), no)
        ld, gd = M.DofLayout(no, 3, blocked).dof(nn, cc), glay.dof(gi[nn], cc)
        assert OP._same_bits(W[-1][ld], res[gd]), "residual_pde: owned rows of the rank against the single rank"
        t_owned = touched[gi[:no]]
        assert 0 < t_owned.sum() < no, "each rank has touched and untouched rows"
        assert ctx.split_sparse_info()[1] == t_owned.sum()
        counted += ctx.split_route_plan()[3]
        for b in range(ctx.n_blocks):
            rp, ci = ctx.pattern(b)
            ncr, cr0 = ((3, 0) if b in (0, 1) else (1, 3)) if blocked else (4, 0)
            ncc, cc0 = ((3, 0) if b in (0, 2) else (1, 3)) if blocked else (4, 0)
            lr = np.repeat(np.arange(rp.size - 1), np.diff(rp))
            grow = glay.dof(gi[lr // ncr], cr0 + lr % ncr)
            gcol = glay.dof(gi[ci // ncc], cc0 + ci % ncc)
            want = np.asarray(A1[grow, gcol]).ravel()
            t = t_owned[lr // ncr]
            assert OP._same_bits(W[b][t], want[t]), f"block {b}: touched owned rows of rank {rk.index} against the single rank"
            assert linf_scaled(W[b][~t], want[~t]) < TOL
        rk.ctx.close()
    assert counted == XC.compressed_cells(c).sum(), "every compressed cell is counted by the rank that owns its lowest vertex"


# ---------------------------------------------------------------- 6
def test_overlay_context_keeps_the_general_family():
    c = LC.block_case()
    ctx = _context(c, route=GENERAL)
    assert ctx.kernel_path == 3
    general = _bytes(*_full(ctx, c)[0], _full(ctx, c)[1])
    ctx.set_split_route(LATTICE)
    lattice = _bytes(*_residuals(ctx, c))
    ctx.set_split_route(SPARSE)
    assert ctx.kernel_path == 3 and ctx.split_route_plan() == (SPARSE, 1, 0, -1) and ctx.split_sparse_info() == (0, -1, -1, 0)
    assert _bytes(*_full(ctx, c)[0], _full(ctx, c)[1]) == general
    assert _bytes(*_residuals(ctx, c)) == lattice and ctx.split_sparse_info() == (0, -1, -1, 0)
    ctx.close()


# ---------------------------------------------------------------- 7
def test_one_living_context_through_the_routes_and_models():
    """unsplit -> 21 -> unsplit -> 5 -> 23 -> model 1 -> model 3 -> 0 on the interleaved corner state: every repeat is the
    bytes of its first run; the context stays a lattice context"""
    shape, kind = (17, 16, 5), "monolithic"
    c = XC.corner(shape, kind)
    off = LC.unsplit(c)
    ref = JC.ref(XC.corner, shape, kind)
    rows = XC.COUNTS[shape][2]
    ctx = _context(off, route=GENERAL)

    def run(case, route, want, model=capi.SPLIT_VOLDEV):
        ctx.set_split_model(model)
        ctx.set_split_route(route)
        ctx.set_params(case.params)
        assert ctx.kernel_path == 1 and ctx.split_route_plan()[:3] == (route,) + want
        values, res = _full(ctx, case)
        pde, tot = _residuals(ctx, case)
        return _bytes(*values, res, pde, tot)

    unsplit = run(off, GENERAL, (0, 0))
    full_parity(off, ctx=ctx)  # the unsplit state against the oracle
    sparse = run(c, SPARSE, (1, 1))
    assert ctx.split_sparse_info()[:2] == (1, rows)
    check("living context, route 21", ctx, c, ref)
    assert run(off, SPARSE, (0, 0)) == unsplit and ctx.split_sparse_info()[:3] == (0, -1, -1)
    jac = run(c, JAC, (1, 1))
    assert ctx.split_sparse_info()[:3] == (0, -1, -1) and jac[-3:] == sparse[-3:]  # (the residuals are the same bytes)
    assert run(c, ALL_SPARSE, (1, 1)) == sparse and ctx.split_sparse_info()[:2] == (1, rows)
    sp_all = run(c, ALL_SPARSE, (1, 0), capi.SPLIT_SPECTRAL)
    sp_any = run(c, ANY, (1, 0), capi.SPLIT_SPECTRAL)
    assert sp_all == sp_any and ctx.split_route_plan()[3] == -1 and ctx.split_sparse_info()[:3] == (0, -1, -1)
    assert run(c, ALL_SPARSE, (1, 1)) == sparse
    check("living context, back on model 3", ctx, c, ref)
    general = run(c, GENERAL, (0, 0))
    check("living context, route 0", ctx, c, ref)
    assert run(c, SPARSE, (1, 1)) == sparse and run(c, JAC, (1, 1)) == jac
    assert run(c, GENERAL, (0, 0)) == general and run(off, GENERAL, (0, 0)) == unsplit
    ctx.close()
