"""The sparse volumetric-deviatoric split Jacobian on the level lattices of a 3-D overlay (pfm_set_split_route with
PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS_SPARSE = 61 or PFM_SPLIT_ROUTE_LATTICE_ALL_LEVELS_SPARSE = 63; CartPlan::voldev_sparse on a
lattice with CartView::row_of_box): per level k_cart_residual3<false, true>, the level form of k_cart_split3_mark, the unsplit
k_cart_uu3 and k_cart_phi4 of the level, then k_cart_split3_jac<NCOL, true, true> over the regular rows at compressed cells; the
general family as under route 13.  Through the C ABI:

1. the interface: 61 and 63 accepted, every other value with bit 32 refused, 2-D, what both info calls answer by route, model,
   split and forced path, before and after pfm_set_params;
2. on a box 61 is 21 and 63 is 23, byte for byte, with both halves of the overlapped assembly;
3. overlay parity: every corner kind against the numpy reference with the four checks of tests/parity_scale.py, then against
   route 13 on the same context: touched regular rows and non-regular rows byte for byte, residual_pde byte for byte, the counts
   predicted in numpy; a second call, a fresh context, z-chunks of 1 and 4 planes, PFM_OVERLAY3_CONCURRENT=1;
4. the untouched regular rows are the unsplit level kernels' bytes;
5. one-sided states: tension recomputes no row, compression recomputes every regular row and is route 13;
6. weights that differ, a bound pattern with shuffled rows;
7. two ranks in the general partition, both halves of the overlapped assembly;
8. one living context through 0 -> 61 -> 13 -> 61 -> unsplit -> 63 -> model 1 -> model 3 -> 0;
9. pfm_line_search_device under 63 is that under 15.

States and the conditions on them: tests/split_levels_sparse_cases.py (run on the CPU by
tests/test_split_levels_sparse_ref_cpu.py).  Bar: 1e-12 (gpu_util.TOL) on the whole matrix and at the scale of each entry, block,
residual row and part (tests/parity_scale.py); reference: split_jacobian_cases.Ref (split_voldev_ref.element_matrices)."""
import numpy as np
import pytest

import cases
import line_search_cases as L
import split_jacobian_cases as JC
import split_lattice_cases as LC
import split_levels_cases as VC
import split_levels_sparse_cases as YC
import split_sparse_cases as XC
import split_voldev_cases as SC
from cracks_amd import capi
from cracks_amd.assembler import node_flags_from_dof_flags
from gpu_util import TOL, blocks_to_global, linf_scaled, make_context
from test_gpu_split3d import _copy, _matrix
from test_gpu_split3d_routes import smallest_edge
from test_gpu_split_lattice_jacobian import _bytes, _context, _full, _residuals, check
from test_gpu_split_levels_jacobian import PFM_ZC_UU3, _all, _regular
from test_gpu_split_sparse_jacobian import LC_context_without_params, _nodes_of_rows

pytestmark = pytest.mark.gpu

GENERAL, LATTICE, ANY = capi.SPLIT_ROUTE_GENERAL, capi.SPLIT_ROUTE_LATTICE, capi.SPLIT_ROUTE_LATTICE_ANY
JAC, ALL = capi.SPLIT_ROUTE_LATTICE_JACOBIAN, capi.SPLIT_ROUTE_LATTICE_ALL
JACL, ALLL = capi.SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS, capi.SPLIT_ROUTE_LATTICE_ALL_LEVELS
SPARSE, ALL_SPARSE = capi.SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE, capi.SPLIT_ROUTE_LATTICE_ALL_SPARSE
# the two new route values; on the parent commit capi has no such names and pfm_set_split_route refuses 61
LS = getattr(capi, "SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS_SPARSE", 61)
ALS = getattr(capi, "SPLIT_ROUTE_LATTICE_ALL_LEVELS_SPARSE", 63)

IDS = [f"{s[0]}x{s[1]}x{s[2]}-{k}" for s, k in YC.CORNER_IDS]


def _touched(c, reg):
    return XC.touched_rows(c) & reg


def _same_rows(ctx, nodes, va, vb, tag):
    """the entries of the rows of `nodes` (bool per node) in every block: equal bytes"""
    n = 0
    for b in range(ctx.n_blocks):
        m = nodes[_nodes_of_rows(ctx, b)]
        x, y = (np.ascontiguousarray(v).view(np.int64) for v in (va[b], vb[b]))
        bad = m & (x != y)
        assert not bad.any(), f"{tag}: block {b}: {int(bad.sum())} of {int(m.sum())} entries differ in a bit"
        n += int(m.sum())
    return n


def against_13(ctx, c, reg, tag):
    """route 61 against route 13 on the same context -> (values, residual_pde, values of 13, touched regular rows)"""
    assert ctx.hanging_info()[1][4] == 0, "no floating-point atomics: the rows of the general family repeat bit for bit"
    t = _touched(c, reg)
    ctx.set_split_route(LS)
    v61, r61 = _full(ctx, c)
    info, plan = ctx.split_sparse_info(), ctx.split_route_plan()
    pde, tot = _residuals(ctx, c)
    assert ctx.split_sparse_info() == info, "a residual-only call leaves the counts of the last full assembly"
    ctx.set_split_route(JACL)
    assert ctx.split_sparse_info()[0] == 0
    v13, r13 = _full(ctx, c)
    assert ctx.split_sparse_info()[1:3] == (-1, -1), "the last full assembly did not run sparse"
    assert ctx.split_route_plan()[1:] == plan[1:], "the plan and the count of compressed cells are route 13's"
    assert _bytes(*_residuals(ctx, c)) == _bytes(pde, tot), "the residual-only call is route 13's"
    ctx.set_split_route(LS)
    n_t = _same_rows(ctx, t, v61, v13, f"{tag}: touched regular rows against route 13")
    n_g = _same_rows(ctx, ~reg, v61, v13, f"{tag}: rows of the general family against route 13")
    assert _bytes(r61) == _bytes(r13), "residual_pde is route 13's on every row"
    rows = c.layout.dof(np.repeat(np.nonzero(reg)[0], 4), np.tile(np.arange(4), int(reg.sum())))
    assert r61[rows].tobytes() == pde[rows].tobytes(), "regular rows: residual_pde of the full assembly is the residual-only call's"
    assert info[0] == 1 and info[1] == int(t.sum()), (info, int(t.sum()))
    differ = sum(int((np.ascontiguousarray(a).view(np.int64) != np.ascontiguousarray(b).view(np.int64)).sum()) for a, b in zip(v61, v13))
    print(f"split_levels_sparse {tag}: {info[1]} regular rows recomputed ({n_t} entries), {info[2]} of {info[3]} tile-chunks flagged, {plan[3]} compressed "
          f"cells counted, {n_g} entries of the general family; {differ} entries of untouched regular rows differ from route 13 in a bit")
    return v61, r61, v13, t, info, plan


# ---------------------------------------------------------------- 1
def test_interface_refusals_and_what_the_info_calls_answer():
    c = LC.block_case()
    off = LC.unsplit(c)
    assert (LS, ALS) == (61, 63) == (JACL | 16 | 32, ALLL | 16 | 32)
    never = LC_context_without_params(c)
    assert never.split_sparse_info() == (0, -1, -1, 0)  # before pfm_set_params
    never.set_split_route(LS)  # (the parent commit refuses this value: PFM_ERR_BAD_ARG)
    assert never.split_route == LS and never.split_route_plan() == (LS, 0, 0, -1) and never.split_sparse_info() == (0, -1, -1, 0)
    never.set_split_route(ALS)
    assert never.split_route == ALS and never.split_route_plan() == (ALS, 0, 0, -1)
    refused = [r for r in range(32, 64) if r not in (LS, ALS)] + [64, 93, 95, 96, 125, 127, 128 + 61, 256 + 63, (1 << 20) | 61]
    refused += [16, 17, 18, 19, 20, 22] + list(range(24, 32)) + [8, 9, 10, 11, 12, 14, 4, 6, 2, -1, -61]
    for r in refused:
        with pytest.raises(capi.PfmError) as e:
            never.set_split_route(r)
        assert e.value.status == 1 and never.split_route == ALS, r
    never.close()
    # 2-D answers PFM_ERR_UNSUPPORTED, as for every known lattice route; 29 stays PFM_ERR_BAD_ARG there
    ctx2 = make_context(cases.kat_miehe_shear_1())
    for route in (LS, ALS):
        with pytest.raises(capi.PfmError) as e:
            ctx2.set_split_route(route)
        assert e.value.status == 5 and ctx2.split_route == GENERAL
    for r in (29, 62, 45):
        with pytest.raises(capi.PfmError) as e:
            ctx2.set_split_route(r)
        assert e.value.status == 1
    assert ctx2.split_sparse_info() == (0, -1, -1, 0)
    ctx2.close()
    # (route, residual-only on the level lattices, full assembly on them, sparse) by route, model, split and forced path
    ctx = _context(c, route=None)
    assert ctx.kernel_path == 3
    for route in (GENERAL, LATTICE, JAC, SPARSE, ALL_SPARSE, JACL, ALLL, LS, ALS):
        ctx.set_split_route(route)
        for model in (capi.SPLIT_SPECTRAL, capi.SPLIT_VOLDEV):
            ctx.set_split_model(model)
            for split in (True, False):
                ctx.set_params(c.params if split else off.params)
                for path in (0, 3):
                    ctx.force_path(path)
                    on = split and path == 3
                    res = int(on and ((model == capi.SPLIT_VOLDEV and route & 1) or (model == capi.SPLIT_SPECTRAL and (route & 3) == 3)))
                    jac = int(on and model == capi.SPLIT_VOLDEV and (route & 13) == 13)
                    sparse = int(jac and (route & 48) == 48)
                    assert ctx.split_route_plan() == (route, res, jac, -1), (route, model, split, path)
                    info = ctx.split_sparse_info()
                    assert info[0] == sparse and info[1:3] == (-1, -1) and (info[3] > 0) == bool(sparse), (route, model, split, path, info)
    ctx.close()
    # 21 / 23 on an overlay: the general family, as before
    ctx = _context(c, route=SPARSE)
    assert ctx.split_route_plan() == (SPARSE, 1, 0, -1) and ctx.split_sparse_info() == (0, -1, -1, 0)
    general = _all(ctx, c)
    assert ctx.split_sparse_info() == (0, -1, -1, 0)
    ctx.set_split_route(GENERAL)
    assert _all(ctx, c) == general
    ctx.close()
    # the sparse buffers of the levels are counted in pfm_ctx_device_bytes: made on first use, kept
    ctx = _context(c, route=LS)
    before = ctx.device_bytes
    _full(ctx, c)
    first = ctx.device_bytes
    _full(ctx, c)
    n_cells = sum(int(np.prod(np.asarray(dims) - 1)) for _, _, dims in YC.LEVEL_ROWS[YC.SMALL])
    assert first - before >= n_cells + 4 * ctx.split_sparse_info()[3] and ctx.device_bytes == first
    ctx.close()


# ---------------------------------------------------------------- 2
def _device_halves(ctx, c):
    """whole assembly, then phase 1 + phase 2 into buffers filled with a sentinel -> (bytes of the whole, bytes of the halves)"""
    import torch

    z = lambda k: torch.full((k,), -7.0e77, dtype=torch.float64, device="cuda")
    ctx.state_set_host(c.sol, c.old, c.oldold)
    out = []
    for phases in ((0,), (1, 2)):
        vals, res = [z(ctx.pattern_size(b)[1]) for b in range(ctx.n_blocks)], [z(ctx.n_owned_dofs), z(ctx.n_owned_dofs)]
        for ph in phases:
            ctx.force_phase(ph)
            ctx.assemble_device(False, [v.data_ptr() for v in vals], res[0].data_ptr(), res[1].data_ptr())
            ctx.sync_status()
        out.append(_bytes(*[v.cpu().numpy() for v in vals], res[0].cpu().numpy()))
    ctx.force_phase(0)
    return out


def test_on_a_box_61_is_21_and_63_is_23_byte_for_byte():
    shape = (5, 4, 3)
    c = XC.corner(shape)
    box = _context(c, route=SPARSE)
    out = {}
    for route in (SPARSE, LS, ALL_SPARSE, ALS):
        box.set_split_route(route)
        assert box.kernel_path == 1 and box.split_route_plan()[:3] == (route, 1, 1) and box.split_sparse_info()[0] == 1
        full = _all(box, c)
        whole, halves = _device_halves(box, c)
        assert whole == halves == full, f"route {route}: phase 1 + phase 2 are the whole assembly"
        out[route] = (full, _bytes(*_residuals(box, c)), box.split_route_plan()[1:], box.split_sparse_info())
    assert out[LS] == out[SPARSE] and out[ALS] == out[ALL_SPARSE]
    assert out[LS][2][2] == XC.COUNTS[shape][0] and out[LS][3][:2] == (1, XC.COUNTS[shape][2])
    box.close()


# ---------------------------------------------------------------- 3
@pytest.mark.parametrize("shape,kind", YC.CORNER_IDS, ids=IDS)
def test_corner_states_against_the_numpy_reference_and_route_13(shape, kind, monkeypatch):
    c = YC.corner(shape, kind)
    ref = JC.ref(YC.corner, shape, kind)
    ctx = _context(c, route=LS)
    assert ctx.kernel_path == 3 and ctx.split_route_plan() == (LS, 1, 1, -1) and ctx.split_sparse_info()[:3] == (1, -1, -1)
    reg = _regular(ctx, c)
    values, res = check(f"levels_sparse {c.name}", ctx, c, ref)  # ((u,phi): exact zeros)
    first = _bytes(*values, res)
    v61, r61, _, t, info, plan = against_13(ctx, c, reg, c.name)
    assert _bytes(*v61, r61) == first, "a second call"
    assert plan == (LS, 1, 1, YC.counted_cells(c)) and plan[3] == YC.COUNTS[shape][2]
    assert info[1] == sum(lv[0] for lv in YC.LEVEL_ROWS[shape]) and 0 < info[2] < info[3]
    fresh = _context(c, route=LS)
    assert _all(fresh, c) == first, "a fresh context"
    assert fresh.split_sparse_info() == info and fresh.split_route_plan() == plan
    fresh.close()
    for planes, per_level in YC.TILE_CHUNKS[shape].items():
        ctx.force_zchunk(PFM_ZC_UU3, planes)  # (reaches every level lattice)
        flagged, total = sum(lv[0] for lv in per_level), sum(lv[1] for lv in per_level)
        assert ctx.split_sparse_info()[3] == total
        for _ in range(2):
            assert _all(ctx, c) == first, f"z-chunks of {planes} planes"
            assert ctx.split_sparse_info() == (1, info[1], flagged, total) and ctx.split_route_plan() == plan, planes
    ctx.force_zchunk(PFM_ZC_UU3, 0)
    assert _all(ctx, c) == first and ctx.split_sparse_info() == info
    ctx.set_split_route(ALS)
    assert _all(ctx, c) == first and ctx.split_sparse_info() == info, "63 under model 3 is 61"
    ctx.close()
    monkeypatch.setenv("PFM_OVERLAY3_CONCURRENT", "1")  # a stream per level lattice: read at every assembly
    par = _context(c, route=LS)
    assert _all(par, c) == first, "PFM_OVERLAY3_CONCURRENT=1"
    assert par.split_sparse_info() == info and par.split_route_plan() == plan  # one row counter, one cell counter for all levels
    assert _all(par, c) == first
    par.close()


# ---------------------------------------------------------------- 4
@pytest.mark.parametrize("shape,kind", YC.CORNER_IDS, ids=IDS)
def test_untouched_regular_rows_are_the_unsplit_level_kernels(shape, kind):
    """The unsplit overlay assembly of the same context with decompose_stress_matrix = 0 -- the parameters of the plan the sparse
    route runs its k_cart_uu3 and k_cart_phi4 with.  With per-cell Lame coefficients that plan has no residual rows either, the same
    instantiations run: equal bytes.  The blocked per-cell kind (staggered, no penalty) is also held to LC.unsplit (time step 0);
    under the monolithic scheme time step 0 drops the penalty term as well (cracks.cc:2141-2144), which is another matrix.  The
    homogeneous kind's unsplit assembly writes its residual rows in the Jacobian kernels (other instantiations): the bar."""
    c = YC.corner(shape, kind)
    lame = YC.KINDS[kind][3]
    ctx = _context(c, route=LS)
    reg = _regular(ctx, c)
    t = _touched(c, reg)
    v61, _ = _full(ctx, c)
    unsplit = [_copy(c.params, decompose_stress_matrix=0.0)] + ([LC.unsplit(c).params] if kind == "lame" else [])
    for prm in unsplit:
        ctx.set_params(prm)
        assert ctx.split_route_plan()[:3] == (LS, 0, 0) and ctx.split_sparse_info()[0] == 0
        v0, _ = _full(ctx, c)
        assert ctx.split_sparse_info()[1:3] == (-1, -1)
        if lame:
            n = _same_rows(ctx, reg & ~t, v61, v0, f"{c.name}: untouched regular rows against the unsplit overlay assembly")
            assert n > 0
        worst = 0.0
        for b in range(ctx.n_blocks):
            m = (reg & ~t)[_nodes_of_rows(ctx, b)]
            worst = max(worst, linf_scaled(v61[b][m], v0[b][m]) if m.any() and np.abs(v0[b][m]).max() > 0 else 0.0)
        print(f"split_levels_sparse {c.name}: untouched regular rows against the unsplit overlay assembly: {worst:.2e}")
        assert worst < TOL
        differ = sum(int((t[_nodes_of_rows(ctx, b)] & (v61[b] != v0[b])).sum()) for b in range(ctx.n_blocks))
        assert differ > 0, "the state tells the two origins apart"
    ctx.close()


# ---------------------------------------------------------------- 5
def test_tension_recomputes_no_row():
    c = VC.one_sided_case(+1)
    SC.assert_one_sided(c, +1)
    ctx = _context(c, route=LS)
    reg = _regular(ctx, c)
    check(f"levels_sparse {c.name}", ctx, c, JC.ref(VC.one_sided_case, +1))
    info = ctx.split_sparse_info()
    assert info[:3] == (1, 0, 0) and info[3] > 0 and ctx.split_route_plan() == (LS, 1, 1, 0)
    against_13(ctx, c, reg, c.name)
    ctx.close()


def test_compression_everywhere_recomputes_every_regular_row_and_is_route_13():
    c = VC.one_sided_case(-1)
    SC.assert_one_sided(c, -1)
    ctx = _context(c, route=LS)
    reg = _regular(ctx, c)
    values, res = check(f"levels_sparse {c.name}", ctx, c, JC.ref(VC.one_sided_case, -1))
    info = ctx.split_sparse_info()
    assert info[:2] == (1, int(reg.sum())) and 0 < info[2] <= info[3]
    assert ctx.split_route_plan() == (LS, 1, 1, VC.rows_owning_a_cell(c.mesh, reg).size)
    ctx.set_split_route(JACL)
    assert _all(ctx, c) == _bytes(*values, res), "every regular row touched: all bytes are route 13's"
    ctx.close()


# ---------------------------------------------------------------- 6
@pytest.mark.parametrize("d_mat,d_rhs", JC.WEIGHTS)
def test_matrix_and_rhs_weights_that_differ(d_mat, d_rhs):
    c = VC.weights_case(d_mat, d_rhs)
    JC.conditions(c)
    ctx = _context(c, route=LS)
    reg = _regular(ctx, c)
    assert ctx.split_route_plan()[:3] == (LS, 1, 1) and ctx.split_sparse_info()[0] == 1
    check(f"levels_sparse {c.name}", ctx, c, JC.ref(VC.weights_case, d_mat, d_rhs))
    against_13(ctx, c, reg, c.name)
    ctx.close()


def test_rows_follow_a_bound_pattern():
    """pfm_pattern_bind with shuffled rows on the (12, 10, 12) block without an active set: the sparse level kernel finds its CSR
    slots through row_perm in the bound order, as the level form does.  The block has no active set, so whole tile-planes of
    the level lattices carry no constraint flag: where such a tile-plane holds no regular row either, the interleaved
    k_cart_phi4 used to take its unguarded fast copy-out with row offsets of -1 and wrote 108 values over the rows of the
    first nodes (test_unsplit_overlay_of_the_block_without_an_active_set_against_the_oracle)."""
    from test_gpu_pattern import _permuted_patterns

    c = VC.big_block_case(False)
    ref = JC.ref(VC.big_block_case, False)
    ctx = _context(c, route=LS)
    reg = _regular(ctx, c)
    for b, (rp, ci, _) in enumerate(_permuted_patterns(ctx, 3, False, seed=11)):
        ctx.pattern_bind(b, rp, ci)
    assert ctx.kernel_path == 3 and ctx.split_route_plan()[:3] == (LS, 1, 1)
    check(c.name + " [bound pattern, route 61]", ctx, c, ref)
    against_13(ctx, c, reg, c.name + " [bound pattern]")
    ctx.close()


def test_unsplit_overlay_of_the_block_without_an_active_set_against_the_oracle():
    """The unsplit overlay assembly of the interleaved (12, 10, 12) block without an active set (decompose_stress_matrix = 0: the
    level kernels route 61 runs underneath) against the oracle.  A tile-plane of a level lattice without a constraint flag and
    without a regular row sent the interleaved k_cart_phi4 into its fast copy-out, which has no guard for absent rows (row offset
    -1): 108 values landed in the rows (node 1, phi), (node 2, u_x), (node 2, u_y), 7.6e-2 off the oracle.  Such a tile-plane now
    takes the generic copy-out, which skips absent rows."""
    import scipy.sparse as sp

    from gpu_util import oracle

    c = VC.big_block_case(False)
    un = cases.Case(c.name + "/unsplit", c.mesh, c.layout, _copy(c.params, decompose_stress_matrix=0.0, decompose_stress_rhs=0.0), c.sol, c.old,
                    c.oldold, c.cu, c.ch, None, c.cell_lambda, c.cell_mu)
    r, rowptr, colind = oracle(un, False)
    ctx = _context(un, route=GENERAL)
    assert ctx.kernel_path == 3 and ctx.split_route_plan()[:3] == (GENERAL, 0, 0)
    values, res = _full(ctx, un)
    A = _matrix(ctx, un, values)
    A_ref = sp.csr_matrix((r.values, colind, rowptr), shape=A.shape)
    A_ref.sort_indices()
    assert A.nnz == A_ref.nnz and (A.indices == A_ref.indices).all()
    e = (linf_scaled(A.data, A_ref.data), linf_scaled(res, r.residual_pde))
    print(f"split_levels_sparse {un.name} against the oracle: matrix {e[0]:.2e} residual {e[1]:.2e}")
    assert max(e) < TOL
    ctx.close()


# ---------------------------------------------------------------- 7
def test_two_ranks_in_the_general_partition_and_both_halves_of_the_overlapped_assembly():
    """The corner state on the refined (8, 8, 8) block in two ranks (partition.partition_general, ghost layer "closure"), both
    contexts on one GPU.  OP.run_partition: every owned row of a rank against the single-rank assembly under the same route at the
    bar, phase 1 writes nothing, phase 1 + phase 2 and the repeated whole assembly are the bytes of the whole assembly.  Then the
    touched owned regular rows of each rank against route 13 on the same rank, byte for byte."""
    import torch

    import test_gpu_overlap_phases as OP

    from cracks_amd import partition as P

    c = YC.corner(YC.SMALL, "lame")
    single = _context(c, route=LS)
    refs = {}
    for ro in (False, True):
        values, r_pde, r_tot = single.assemble_host(c.sol, c.old, c.oldold, ro)
        refs[ro] = OP.Reference(c.layout, None if ro else blocks_to_global(single, c.layout, values), r_pde, r_tot)
    single.close()
    node, comp = c.layout.node_comp_of_dof()
    nodal = []
    for v in (c.sol, c.old, c.oldold):
        F = np.empty((c.layout.n_nodes, 4))
        F[node, comp] = v
        nodal.append(F)
    flags = node_flags_from_dof_flags(c.layout, c.cu.flag, c.ch.flag)
    touched = XC.touched_rows(c)
    ranks = []
    for k, lp in enumerate(P.partition_general(c.mesh, 2, ghost_layer="closure")):
        rk = OP._rank(k, lp, True, LC.unsplit(c).params, flags, nodal, cell_lambda=c.cell_lambda[lp.global_cells], cell_mu=c.cell_mu[lp.global_cells])
        rk.ctx.set_split_model(capi.SPLIT_VOLDEV)
        rk.ctx.set_split_route(LS)
        rk.ctx.set_params(c.params)
        assert rk.lp.n_owned < rk.lp.mesh.n_nodes and rk.ctx.kernel_path == 3 and rk.ctx.split_route_plan()[:3] == (LS, 1, 1)
        assert rk.ctx.split_sparse_info()[0] == 1
        ranks.append(rk)
    OP.run_partition(ranks, refs, general=True)
    reg_global = VC.regular_rows(c.mesh)
    recomputed = 0
    for rk in ranks:  # (the ghosts hold the exchanged state, the phase is 0 again)
        # A rank's own regular rows are a subset of the owned ones that are regular on the whole mesh (next to the cut a row loses
        # cells to the other rank).  A touched owned row is route 13's bytes either way: recomputed if regular on this rank, a row
        # of the general family if not.  So every owned touched row is compared, and every entry that differs from route 13 must
        # lie in an untouched row that is regular on the whole mesh.
        ctx, no = rk.ctx, rk.lp.n_owned
        go = rk.lp.global_ids[:no]
        assert 0 < ctx.overlay_info()[0] <= int(reg_global[go].sum())
        t = touched[go]
        z = lambda n: torch.empty(n, dtype=torch.float64, device="cuda")
        out = {}
        for route in (LS, JACL):
            ctx.set_split_route(route)
            vals, res = [z(ctx.pattern_size(b)[1]) for b in range(ctx.n_blocks)], [z(ctx.n_owned_dofs), z(ctx.n_owned_dofs)]
            ctx.assemble_device(False, [v.data_ptr() for v in vals], res[0].data_ptr(), res[1].data_ptr())
            ctx.sync_status()
            out[route] = ([v.cpu().numpy() for v in vals], res[0].cpu().numpy(), ctx.split_route_plan()[3], ctx.split_sparse_info())
        print(f"split_levels_sparse two ranks: rank {rk.index} owns {no} nodes, {ctx.overlay_info()[0]} regular rows, {int(t.sum())} owned rows touched; {out[LS][3]}")
        assert out[LS][3][0] == 1 and 0 <= out[LS][3][1] <= int((t & reg_global[go]).sum()) and out[JACL][3][1:3] == (-1, -1)
        assert out[LS][2] == out[JACL][2] >= 0
        recomputed += out[LS][3][1]
        _same_rows(ctx, t, out[LS][0], out[JACL][0], f"rank {rk.index}: touched owned rows against route 13")
        _same_rows(ctx, ~reg_global[go], out[LS][0], out[JACL][0], f"rank {rk.index}: rows that are not regular against route 13")
        assert _bytes(out[LS][1]) == _bytes(out[JACL][1])
        ctx.close()
    assert 0 < recomputed <= int((touched & reg_global).sum())


# ---------------------------------------------------------------- 8
def test_one_living_context_through_the_routes_and_models():
    """0 -> 61 -> 13 -> 61 -> unsplit -> 63 -> model 1 -> model 3 -> 0 on the interleaved corner state of the (8, 8, 8) block: at
    each stop the bytes are those of a context that was set to that route directly"""
    c = YC.corner(YC.SMALL, "monolithic")
    off = LC.unsplit(c)
    ctx = _context(off, route=GENERAL)
    info = (ctx.kernel_path, ctx.overlay_info())
    assert info[0] == 3
    rows = sum(lv[0] for lv in YC.LEVEL_ROWS[YC.SMALL])

    def run(on, case, route, want, model=capi.SPLIT_VOLDEV):
        on.set_split_model(model)
        on.set_split_route(route)
        on.set_hanging_mode(capi.HANGING_MODE_GATHER if model == capi.SPLIT_SPECTRAL else capi.HANGING_MODE_DEFAULT)  # (model 1: atomics by default)
        on.set_params(case.params)
        assert (on.kernel_path, on.overlay_info()) == info and on.split_route_plan()[:3] == (route,) + want
        values, res = _full(on, case)
        sparse = on.split_sparse_info()
        pde, tot = _residuals(on, case)
        return _bytes(*values, res, pde, tot), sparse[:3], on.split_route_plan()[3]

    stops = [(c, GENERAL, (0, 0), capi.SPLIT_VOLDEV), (c, LS, (1, 1), capi.SPLIT_VOLDEV), (c, JACL, (1, 1), capi.SPLIT_VOLDEV),
             (c, LS, (1, 1), capi.SPLIT_VOLDEV), (off, LS, (0, 0), capi.SPLIT_VOLDEV), (c, ALS, (1, 1), capi.SPLIT_VOLDEV),
             (c, ALS, (1, 0), capi.SPLIT_SPECTRAL), (c, ALS, (1, 1), capi.SPLIT_VOLDEV), (c, GENERAL, (0, 0), capi.SPLIT_VOLDEV)]
    direct = {}
    for k, (case, route, want, model) in enumerate(stops):
        key = (case is off, route, model)
        if key not in direct:
            d = _context(case, route=route, model=model)
            direct[key] = run(d, case, route, want, model)
            d.close()
        got = run(ctx, case, route, want, model)
        assert got == direct[key], f"stop {k}: route {route}, model {model}"
        sparse = route in (LS, ALS) and want == (1, 1)
        assert got[1] == ((1, rows, got[1][2]) if sparse else (0, -1, -1)) and (got[2] >= 0) == (want[1] == 1)
    ctx.close()


# ---------------------------------------------------------------- 9
def test_device_line_search_under_63_is_that_under_15():
    import test_gpu_line_search as LS_

    c = VC.line_search_case()
    upd = L.newton_update(c, seed=5, u_amp=2e-4 * smallest_edge(c.mesh), phi_amp=0.5)
    ctxs = {ALLL: _context(c, route=ALLL), ALS: _context(c, route=ALS)}
    assert ctxs[ALLL].split_route_plan()[:3] == (ALLL, 1, 1) and ctxs[ALS].split_route_plan()[:3] == (ALS, 1, 1)
    want, _ = LS_._run_both(ctxs[ALLL], c, upd, 0.0, 4, "l2", "saved")  # exhaustion: the norm of every trial
    trials = want["trials"]
    reference = 0.5 * (trials[2] + min(trials[:2])) if trials[2] < min(trials[:2]) else 2.0 * max(trials)
    got = {}
    for route, ctx in ctxs.items():
        w, g = LS_._run_both(ctx, c, upd, reference, 4, "l2", "saved")
        LS_._compare(c, w, g, True)
        got[route] = (w, g)
    (wa, a), (wb, b) = got[ALLL], got[ALS]
    print("split_levels_sparse line search:", a["steps"], a["accepted"], a["norms"], "|", b["steps"], b["accepted"], b["norms"])
    assert b["steps"] == a["steps"] and b["accepted"] == a["accepted"] and LS_.same_bits(b["norms"], a["norms"])
    assert LS_.same_bits(np.asarray(wb["trials"], float), np.asarray(wa["trials"], float)), "the norm of every trial"
    for k in ("sol", "upd", "pde", "tot"):
        assert LS_.same_bits(b["vec"][k][0], a["vec"][k][0]) and LS_.same_bits(wb["vec"][k][0], wa["vec"][k][0]), k
    for ctx in ctxs.values():
        ctx.close()
