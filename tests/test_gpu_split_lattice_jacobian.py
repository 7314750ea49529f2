"""The volumetric-deviatoric split Jacobian on the row-owner lattice kernels (pfm_set_split_route with
PFM_SPLIT_ROUTE_LATTICE_JACOBIAN = 5 or PFM_SPLIT_ROUTE_LATTICE_ALL = 7: k_cart_split3_jac of cracks_amd/csrc/pfm_cart_split3.hip
for the matrix values, k_cart_residual3<false, true> for residual_pde; CartPlan::voldev_jac), through the C ABI:

1. the interface: default, refusals (4, 6, 2; 2-D), models 0 and 1 under 5 and 7, what pfm_ctx_split_route_info answers before
   and after pfm_set_params and under forced path 0, and a context that never set a route against one that went 5 -> 0;
2. boxes against the numpy reference and against the general route, all four blocks and residual_pde, the four checks of
   tests/parity_scale.py;
3. one-sided states (tension: the unsplit oracle's matrix, no compressed cell), d_mat != d_rhs;
4. bitwise: residual_pde of the full assembly under 5 is the residual-only call's under 1; repeats, a fresh context, two
   z-chunk lengths;
5. two ranks on one GPU: owned rows against the single rank, the halves of the overlapped assembly, both layouts;
6. Dirichlet faces with an active set and per-cell Lame: constrained rows and columns, placeholder diagonals, and the
   (u,u) diagonal patches next to cells whose element diagonal vanishes;
7. an overlay context under 5: the full assembly is the general route's, and the info call says so;
8. one living context through unsplit -> 5 -> unsplit -> 0 -> 7 -> model 1 -> model 3.

States, references and the conditions on them: tests/split_lattice_cases.py, tests/split_jacobian_cases.py (run on the CPU by
tests/test_split_jacobian_ref_cpu.py).  Bar: 1e-12 (gpu_util.TOL) on the whole matrix and at the scale of each entry, block
and residual row (tests/parity_scale.py)."""
import numpy as np
import pytest
import scipy.sparse as sp

import cases
import split_jacobian_cases as JC
import split_lattice_cases as LC
import split_voldev_cases as SC
from cracks_amd import capi
from cracks_amd import mesh as M
from cracks_amd.assembler import Context, node_flags_from_dof_flags
import parity_scale as PS
from gpu_util import TOL, full_parity, linf_scaled, make_context, oracle, path_parity, reference_parity, total_matrix
from test_gpu_split3d import _copy, _matrix

pytestmark = pytest.mark.gpu

GENERAL, LATTICE, ANY = capi.SPLIT_ROUTE_GENERAL, capi.SPLIT_ROUTE_LATTICE, capi.SPLIT_ROUTE_LATTICE_ANY
JAC, ALL = capi.SPLIT_ROUTE_LATTICE_JACOBIAN, capi.SPLIT_ROUTE_LATTICE_ALL
PFM_ZC_UU3 = 0  # pfm_ctx_force_zchunk: the tiles and chunks of k_cart_uu3, which k_cart_split3_jac marches over


def _context(c, route=JAC, model=capi.SPLIT_VOLDEV, **kw):
    ctx = Context(c.mesh, c.layout.blocked, cell_lambda=c.cell_lambda, cell_mu=c.cell_mu, **kw)
    ctx.set_split_model(model)
    if route is not None:
        ctx.set_split_route(route)
    ctx.set_params(c.params)
    ctx.set_constraints(node_flags_from_dof_flags(c.layout, c.cu.flag, c.ch.flag))
    return ctx


def _full(ctx, c):
    values, res, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
    return values, res


def _residuals(ctx, c):
    _, pde, tot = ctx.assemble_host(c.sol, c.old, c.oldold, True)
    return pde, tot


def _bytes(*arrays):
    return [np.ascontiguousarray(a).tobytes() for a in arrays]


def check(tag, ctx, c, ref):
    """the full assembly against the reference: the whole-matrix bar, then per entry, per block ((u,phi) exactly zero) and
    per residual row; returns (values, residual_pde)"""
    values, res = _full(ctx, c)
    A = _matrix(ctx, c, values)
    assert all(np.isfinite(v).all() for v in values) and np.isfinite(res).all()
    assert A.nnz == ref.A.nnz and (A.indptr == ref.A.indptr).all() and (A.indices == ref.A.indices).all()
    e = (linf_scaled(A.data, ref.A.data), linf_scaled(res, ref.pde))
    print(f"split_lattice_jacobian {tag}: matrix {e[0]:.2e} residual {e[1]:.2e}")
    assert max(e) < TOL, e
    reference_parity(c.layout, c.sol, A, ref.A, [(res, ref.pde, "pde")], tag=f"split_lattice_jacobian {tag}", A_tot=ref.A_tot)
    blk = PS.block_of_entries(c.layout, PS.entry_rows(A), A.indices)
    assert not A.data[blk == 1].any(), "the structurally zero (u,phi) block holds exact zeros"
    return values, res


def against_general(tag, c, values, res):
    """the same assembly on the general route, on the GPU, at the same bar"""
    g = _context(c, route=GENERAL)
    assert g.split_route_plan()[:3] == (GENERAL, 0, 0)
    values_g, res_g = _full(g, c)
    A, B = _matrix(g, c, values), _matrix(g, c, values_g)
    e = (linf_scaled(A.data, B.data), linf_scaled(res, res_g))
    print(f"split_lattice_jacobian {tag}: lattice against general route: matrix {e[0]:.2e} residual {e[1]:.2e}")
    assert max(e) < TOL, e
    path_parity(g, c.layout, values, values_g, [(res, res_g)], tag=f"split_lattice_jacobian {tag}")
    g.close()


# ---------------------------------------------------------------- 1
def test_interface_refusals_models_and_what_the_plan_answers():
    kind = "blocked/active_set/rhs1/lame/lines"
    c = LC.box_case((5, 4, 3), kind)
    off = LC.unsplit(c)
    assert (JAC, ALL) == (5, 7) == (LATTICE | 4, ANY | 4)
    never = Context(c.mesh, True, cell_lambda=c.cell_lambda, cell_mu=c.cell_mu)
    never.set_split_model(capi.SPLIT_VOLDEV)
    assert never.split_route == GENERAL and never.split_route_plan() == (GENERAL, 0, 0, -1)  # before pfm_set_params
    never.set_split_route(JAC)
    assert never.split_route_plan() == (JAC, 0, 0, -1) and never.split_route_info() == (JAC, 0)
    never.set_split_route(GENERAL)
    never.set_params(c.params)
    never.set_constraints(node_flags_from_dof_flags(c.layout, c.cu.flag, c.ch.flag))
    for unknown in (4, 6, 2, 8, -1):
        with pytest.raises(capi.PfmError) as e:
            never.set_split_route(unknown)
        assert e.value.status == 1 and never.split_route == GENERAL and never.split_route_plan() == (GENERAL, 0, 0, -1)
    first = _bytes(*_full(never, c)[0], _full(never, c)[1], *_residuals(never, c))
    never.close()
    # 2-D keeps the general route
    c2 = cases.kat_miehe_shear_1()
    ctx2 = make_context(c2)
    for route in (JAC, ALL):
        with pytest.raises(capi.PfmError) as e:
            ctx2.set_split_route(route)
        assert e.value.status == 5 and ctx2.split_route == GENERAL and ctx2.split_route_plan()[:3] == (GENERAL, 0, 0)
    ctx2.close()
    # (route, residual-only on the lattice, full assembly on the lattice) by route, model, split and forced path
    ctx = _context(c, route=None)
    for route in (GENERAL, LATTICE, ANY, JAC, ALL):
        ctx.set_split_route(route)
        for model in (capi.SPLIT_SPECTRAL, capi.SPLIT_VOLDEV):
            ctx.set_split_model(model)
            for split in (True, False):
                ctx.set_params(c.params if split else off.params)
                for path in (0, 1):
                    ctx.force_path(path)
                    on = split and path == 1
                    res = int(on and ((model == capi.SPLIT_VOLDEV and route & 1) or (model == capi.SPLIT_SPECTRAL and (route & 3) == 3)))
                    jac = int(on and model == capi.SPLIT_VOLDEV and (route & 4) == 4)
                    assert ctx.split_route_plan()[:3] == (route, res, jac), (route, model, split, path)
                    assert ctx.split_route_info() == (route, res)
    # (now: ALL, model 3, split off, path 1)  model 0 accepts the route and refuses the 3-D split as ever
    ctx.set_params(c.params)
    ctx.set_split_model(capi.SPLIT_REFERENCE)
    assert ctx.split_route_plan()[:3] == (ALL, 0, 0)
    with pytest.raises(capi.PfmError) as e:
        _full(ctx, c)
    assert e.value.status == 5
    # model 1 under 5 and 7: the full assembly is the general family's, the residual-only call follows 1 (no effect) / 3
    spectral = {}
    for route in (GENERAL, ANY, JAC, ALL):
        ctx.set_split_model(capi.SPLIT_SPECTRAL)
        ctx.set_split_route(route)
        spectral[route] = (_bytes(*_full(ctx, c)[0], _full(ctx, c)[1]), _bytes(*_residuals(ctx, c)))
    assert spectral[JAC] == spectral[GENERAL] and spectral[ALL] == spectral[ANY] and spectral[ALL][0] == spectral[GENERAL][0]
    # 5 -> 0: the bytes of a context that never set a route
    ctx.set_split_model(capi.SPLIT_VOLDEV)
    ctx.set_split_route(JAC)
    assert ctx.split_route_plan()[:3] == (JAC, 1, 1)
    check("interface", ctx, c, JC.ref(LC.box_case, (5, 4, 3), kind))
    assert ctx.split_route_plan()[3] > 0
    ctx.set_split_route(GENERAL)
    assert ctx.split_route_plan()[:3] == (GENERAL, 0, 0)
    assert _bytes(*_full(ctx, c)[0], _full(ctx, c)[1], *_residuals(ctx, c)) == first
    assert ctx.split_route_plan()[3] == -1  # the last full assembly did not run on the lattice kernel
    ctx.close()


# ---------------------------------------------------------------- 2
@pytest.mark.parametrize("shape,kind", LC.BOX_IDS, ids=[f"{s[0]}x{s[1]}x{s[2]}-{k}" for s, k in LC.BOX_IDS])
def test_boxes_against_the_numpy_reference_and_the_general_route(shape, kind):
    c = LC.box_case(shape, kind)
    share, margin = JC.conditions(c)
    ref = JC.ref(LC.box_case, shape, kind)
    ctx = _context(c)
    assert ctx.kernel_path == 1 and ctx.split_route_plan()[:3] == (JAC, 1, 1)
    values, res = check(f"{c.name} (share {share:.2f}, margin {margin:.1e})", ctx, c, ref)
    n = ctx.split_route_plan()[3]
    assert 0 < n <= c.mesh.n_cells
    against_general(c.name, c, values, res)
    ctx.close()


# ---------------------------------------------------------------- 3
def test_without_compression_it_is_the_unsplit_oracle_and_no_cell_is_compressed():
    c = LC.one_sided_case(+1)
    SC.assert_one_sided(c, +1)
    off = cases.Case(c.name, c.mesh, c.layout, _copy(c.params, decompose_stress_matrix=0.0, decompose_stress_rhs=0.0), c.sol, c.old, c.oldold,
                     c.cu, c.ch, None, c.cell_lambda, c.cell_mu)
    r, rowptr, colind = oracle(off, False)
    ctx = _context(c)
    assert ctx.split_route_plan()[:3] == (JAC, 1, 1)
    values, res = _full(ctx, c)
    A = _matrix(ctx, c, values)
    A_ref = sp.csr_matrix((r.values, colind, rowptr), shape=A.shape)
    assert A.nnz == A_ref.nnz and (A.indices == A_ref.indices).all()
    e = (linf_scaled(A.data, A_ref.data), linf_scaled(res, r.residual_pde))
    print(f"split_lattice_jacobian {c.name} against the unsplit oracle: matrix {e[0]:.2e} residual {e[1]:.2e}")
    assert max(e) < TOL
    reference_parity(c.layout, c.sol, A, A_ref, [(res, r.residual_pde, "pde")], tag="split_lattice_jacobian against the unsplit oracle",
                     A_tot=total_matrix(off, A_ref))
    assert ctx.split_route_plan() == (JAC, 1, 1, 0)
    ctx.close()


def test_compression_everywhere():
    c = LC.one_sided_case(-1)
    SC.assert_one_sided(c, -1)
    ctx = _context(c)
    check(c.name, ctx, c, JC.ref(LC.one_sided_case, -1))
    assert ctx.split_route_plan() == (JAC, 1, 1, c.mesh.n_cells)
    ctx.close()


@pytest.mark.parametrize("d_mat,d_rhs", JC.WEIGHTS)
def test_matrix_and_rhs_weights_that_differ(d_mat, d_rhs):
    c = JC.weights_case(d_mat, d_rhs)
    JC.conditions(c)
    ctx = _context(c)
    assert ctx.split_route_plan()[:3] == (JAC, 1, 1)
    values, res = check(c.name, ctx, c, JC.ref(JC.weights_case, d_mat, d_rhs))
    against_general(c.name, c, values, res)
    ctx.close()


def test_matrix_weight_zero_is_no_split_assembly():
    """decompose_stress_matrix = 0, decompose_stress_rhs = 1: the gate of the split (cracks.cc:2294) is the matrix weight, so
    nothing follows the route"""
    c = JC.weights_case(1.0, 0.0)
    z = cases.Case("jacobian/weights/mat0/rhs1", c.mesh, c.layout, _copy(c.params, decompose_stress_matrix=0.0, decompose_stress_rhs=1.0), c.sol, c.old,
                   c.oldold, c.cu, c.ch, None, c.cell_lambda, c.cell_mu)
    out = {}
    for route in (GENERAL, JAC):
        ctx = _context(z, route=route)
        assert ctx.split_route_plan()[:3] == (route, 0, 0)
        out[route] = _bytes(*_full(ctx, z)[0], _full(ctx, z)[1])
        ctx.close()
    assert out[JAC] == out[GENERAL]


# ---------------------------------------------------------------- 4
def test_bitwise_properties():
    shape, kind = (17, 16, 5), "blocked/active_set/rhs1/lame/lines"
    c = LC.box_case(shape, kind)
    ctx = _context(c)
    values, res = _full(ctx, c)
    first = _bytes(*values, res)
    assert _bytes(*_full(ctx, c)[0], _full(ctx, c)[1]) == first
    # the Jacobian call's residual_pde is the line-search residual of route 1, and of this route
    assert _bytes(_residuals(ctx, c)[0]) == _bytes(res)
    one = _context(c, route=LATTICE)
    assert _bytes(_residuals(one, c)[0]) == _bytes(res)
    one.close()
    fresh = _context(c)
    assert _bytes(*_full(fresh, c)[0], _full(fresh, c)[1]) == first
    fresh.close()
    # two forced chunk lengths: 6 planes in chunks of 1 and of 4
    assert ctx.zchunk(PFM_ZC_UU3) > 1
    for planes in (1, 4):
        ctx.force_zchunk(PFM_ZC_UU3, planes)
        assert ctx.zchunk(PFM_ZC_UU3) == planes
        assert _bytes(*_full(ctx, c)[0], _full(ctx, c)[1]) == first
    ctx.force_zchunk(PFM_ZC_UU3, 0)
    for route in (ALL,):
        ctx.set_split_route(route)
        assert _bytes(*_full(ctx, c)[0], _full(ctx, c)[1]) == first
    ctx.close()


# ---------------------------------------------------------------- 5
@pytest.mark.parametrize("blocked", [True, False])
def test_two_ranks_and_both_halves_of_the_overlapped_assembly(blocked):
    """(33, 5, 4) unit cells in two ranks along x (unit cells: the same cell size, bit for bit, on the box and on the sub-boxes).
    OP.run_phases: the whole assembly against the reference, phase 1 with poisoned
    ghosts writes only final values, phase 1 + phase 2 and the repeated whole assembly equal the whole assembly bit for bit.
    Then the owned rows of each rank against the single rank, byte for byte."""
    import test_gpu_overlap_phases as OP

    import torch

    from cracks_amd import partition as P

    c = JC.two_rank_case(blocked)
    JC.conditions(c)
    r = JC.ref(JC.two_rank_case, blocked)
    ref = OP.Reference(c.layout, r.A, r.pde, None, c.sol)
    single = _context(c)
    values, res = check(c.name + " (one rank)", single, c, r)
    A1 = _matrix(single, c, values)
    single.close()
    # OP.box_ranks with the extents of the unit cells
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
        rk.ctx.set_split_route(JAC)
        rk.ctx.set_params(c.params)
        assert rk.lp.n_owned < rk.lp.mesh.n_nodes and rk.ctx.kernel_path == 1 and rk.ctx.split_route_plan()[:3] == (JAC, 1, 1)
    recv = OP.exchange_ghosts([rk.lp for rk in ranks], [rk.ctx for rk in ranks], 3)
    for rk, buf in zip(ranks, recv):
        W, p1 = OP.run_phases(rk, buf, False, ref)
        ctx, no, gi, glay = rk.ctx, rk.lp.n_owned, rk.lp.global_ids, c.layout
        share = OP._share(p1[-1])
        assert 0.0 < share < 1.0, "each sub-box has interior and boundary tiles of the residual kernel"
        nn, cc = np.repeat(np.arange(no), 4), np.tile(np.arange(4), no)
        ld, gd = M.DofLayout(no, 3, blocked).dof(nn, cc), glay.dof(gi[nn], cc)
        # (unit cells: the cell size is 1.0 on the box and on the sub-boxes, so the rows of both kernels can be held to the bytes;
        # with extents whose h is rounded, residual_pde differs in its last bits as under route 1, tests/test_gpu_split_lattice.py)
        e = linf_scaled(W[-1][ld], res[gd])
        print(f"split_lattice_jacobian {c.name} rank {rk.index}: residual_pde against the single rank {e:.2e} "
              f"(same bits: {OP._same_bits(W[-1][ld], res[gd])})")
        assert OP._same_bits(W[-1][ld], res[gd]), "residual_pde: owned rows of the rank against the single rank"
        PS.assert_parts(W[-1][ld], res[gd], cc == 3, TOL, f"split_lattice_jacobian {c.name} rank {rk.index} residual_pde")
        for b in range(ctx.n_blocks):
            rp, ci = ctx.pattern(b)
            ncr, cr0 = ((3, 0) if b in (0, 1) else (1, 3)) if blocked else (4, 0)
            ncc, cc0 = ((3, 0) if b in (0, 2) else (1, 3)) if blocked else (4, 0)
            lr = np.repeat(np.arange(rp.size - 1), np.diff(rp))
            grow = glay.dof(gi[lr // ncr], cr0 + lr % ncr)
            gcol = glay.dof(gi[ci // ncc], cc0 + ci % ncc)
            want = np.asarray(A1[grow, gcol]).ravel()
            assert OP._same_bits(W[b], want), f"block {b}: owned rows of rank {rk.index} against the single rank"
        rk.ctx.close()


# ---------------------------------------------------------------- 6
def test_constrained_rows_columns_and_placeholder_diagonals():
    from test_gpu_split3d_routes import constrained_rows_hold_their_placeholder

    for blocked in (True, False):
        kind = "blocked/active_set/rhs1/lame/lines" if blocked else "interleaved/active_set/rhs0.5/lame/lines"
        c = LC.box_case((17, 16, 5), kind)
        ref = JC.ref(LC.box_case, (17, 16, 5), kind)
        ctx = _context(c)
        constrained_rows_hold_their_placeholder(c, ref, ctx)
        A = _matrix(ctx, c, _full(ctx, c)[0])
        lines = np.nonzero(c.cu.flag.astype(bool))[0]
        assert not A[:, lines][np.setdiff1d(np.arange(A.shape[0]), lines)].count_nonzero(), "eliminated columns hold zeros"
        ctx.close()


def test_diagonal_patches_next_to_cells_whose_element_diagonal_vanishes():
    c = JC.dead_case()
    JC.conditions(c)
    ref = JC.ref(JC.dead_case)
    ctx = _context(c)
    assert ctx.split_route_plan()[:3] == (JAC, 1, 1)
    values, res = check(c.name, ctx, c, ref)
    A = _matrix(ctx, c, values)
    lines = np.nonzero(c.cu.flag.astype(bool))[0]
    d = A.diagonal()[lines]
    print(f"split_lattice_jacobian {c.name}: placeholder diagonals in [{d.min():.3e}, {d.max():.3e}]")
    assert (d > 0.0).all() and linf_scaled(d, ref.A.diagonal()[lines]) < TOL
    against_general(c.name, c, values, res)
    ctx.close()


# ---------------------------------------------------------------- 7
def test_overlay_context_keeps_the_general_family_for_the_full_assembly():
    c = LC.block_case()
    ctx = _context(c, route=GENERAL)
    assert ctx.kernel_path == 3 and ctx.split_route_plan()[:3] == (GENERAL, 0, 0)
    general = _bytes(*_full(ctx, c)[0], _full(ctx, c)[1])
    ctx.set_split_route(LATTICE)
    lattice = _bytes(*_residuals(ctx, c))
    ctx.set_split_route(JAC)
    assert ctx.kernel_path == 3 and ctx.split_route_plan() == (JAC, 1, 0, -1)
    assert _bytes(*_full(ctx, c)[0], _full(ctx, c)[1]) == general
    assert _bytes(*_residuals(ctx, c)) == lattice and ctx.split_route_plan() == (JAC, 1, 0, -1)
    ctx.close()


# ---------------------------------------------------------------- 8
def test_one_living_context_through_the_routes_and_models():
    """unsplit -> 5 -> unsplit -> 0 -> 7 -> model 1 -> model 3 on (17, 16, 5): each state against its reference or against the
    bytes of its first run; the context stays a lattice context"""
    shape, kind = (17, 16, 5), "interleaved/active_set/rhs0.5/lame/lines"
    c = LC.box_case(shape, kind)
    off = LC.unsplit(c)
    ref = JC.ref(LC.box_case, shape, kind)
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
    jac = run(c, JAC, (1, 1))
    check("living context, route 5", ctx, c, ref)
    assert run(off, JAC, (0, 0)) == unsplit
    general = run(c, GENERAL, (0, 0))
    check("living context, route 0", ctx, c, ref)
    every = run(c, ALL, (1, 1))
    assert every == jac
    check("living context, route 7", ctx, c, ref)
    sp_all = run(c, ALL, (1, 0), capi.SPLIT_SPECTRAL)
    sp_any = run(c, ANY, (1, 0), capi.SPLIT_SPECTRAL)
    assert sp_all == sp_any and ctx.split_route_plan()[3] == -1
    assert run(c, ALL, (1, 1)) == jac
    check("living context, back on model 3", ctx, c, ref)
    assert run(c, GENERAL, (0, 0)) == general and run(off, GENERAL, (0, 0)) == unsplit
    ctx.close()
