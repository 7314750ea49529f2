"""The spectral split residual on the row-owner lattice kernels (pfm_set_split_route, PFM_SPLIT_ROUTE_LATTICE_ANY = 3 under
PFM_SPLIT_SPECTRAL: k_cart_residual3<false, false, true> of cracks_amd/csrc/pfm_cart.hip, CartPlan::spectral), through the C ABI:

1. the interface: route 3 accepted in 3-D and refused in 2-D, 2 and -1 still refused, what pfm_ctx_split_route answers over
   routes x models x split x path, model 3 on route 3 against route 1 and route 3 -> 0 against a context that never set a
   route, byte for byte;
2. boxes against the numpy reference, both layouts, both solvers, decompose_stress_rhs 0 / 0.5 / 1, per-cell Lame, Dirichlet
   faces with an active set, use_old_timestep_pf; two z-chunk lengths and a second call give the same bytes;
3. one-sided states, zero strain, an exactly diagonal and an isotropic strain, a pure shear with a zero eigenvalue;
4. two ranks on one GPU: owned rows against the single rank, the halves of the overlapped assembly bit for bit;
5. the overlay: level lattices with the law, the general family (atomics at the hanging vertices) for the rest;
6. the fused entry pfm_assemble_nl_residual_device against its three-call form, bit for bit;
7. pfm_line_search_device under routes 0 and 3;
8. one living context through unsplit -> route 3 model 1 -> unsplit -> route 0 -> route 3 model 3 -> route 3 model 1.

States, references and the conditions on them: tests/split_lattice_spectral_cases.py (run on the CPU by
tests/test_split_lattice_spectral_ref_cpu.py).  Bar: |x - x_ref|_inf < 1e-12 max(1, |x_ref|_inf) (gpu_util.TOL), and per row and
per part (tests/parity_scale.py) as tests/test_gpu_split_lattice.py asserts them."""
import numpy as np
import pytest

import cases
import parity_scale as PS
import split_lattice_spectral_cases as XC
from cracks_amd import capi
from cracks_amd import mesh as M
from cracks_amd.assembler import Context, node_flags_from_dof_flags
from gpu_util import TOL, linf_scaled, make_context, oracle, residual_parity
from test_gpu_split3d import _copy, _matrix

pytestmark = pytest.mark.gpu

GENERAL, LATTICE, ANY = capi.SPLIT_ROUTE_GENERAL, capi.SPLIT_ROUTE_LATTICE, capi.SPLIT_ROUTE_LATTICE_ANY
SPECTRAL, VOLDEV = capi.SPLIT_SPECTRAL, capi.SPLIT_VOLDEV
PFM_ZC_RES3 = 2  # pfm_ctx_force_zchunk: k_cart_residual3


def _context(c, route=ANY, model=SPECTRAL, **kw):
    ctx = Context(c.mesh, c.layout.blocked, cell_lambda=c.cell_lambda, cell_mu=c.cell_mu, **kw)
    ctx.set_split_model(model)
    if route is not None:
        ctx.set_split_route(route)
    ctx.set_params(c.params)
    ctx.set_constraints(node_flags_from_dof_flags(c.layout, c.cu.flag, c.ch.flag))
    return ctx


def _residuals(ctx, c):
    _, pde, tot = ctx.assemble_host(c.sol, c.old, c.oldold, True)
    return pde, tot


def _full(ctx, c):
    values, res, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
    return values, res


def _bytes(*arrays):
    return [np.ascontiguousarray(a).tobytes() for a in arrays]


def _all_bytes(ctx, c):
    """the full assembly and the residual-only call"""
    values, res = _full(ctx, c)
    return _bytes(*values, res, *_residuals(ctx, c))


def scaled(tag, c, ref, pde=None, tot=None):
    """per row and per part (tests/parity_scale.py), the scales from the reference's own Jacobian of the state"""
    A_ref, A_tot = ref.matrices()
    if pde is not None:
        PS.assert_residual(pde, ref.pde, A_ref, c.layout, ref._sol, TOL, f"split_lattice_spectral {tag} residual_pde")
    if tot is not None:
        PS.assert_residual(tot, ref.tot, A_tot, c.layout, ref._sol, TOL, f"split_lattice_spectral {tag} residual_total")


def check(tag, ctx, c, ref):
    """the residual-only call against the reference; returns (residual_pde, residual_total)"""
    pde, tot = _residuals(ctx, c)
    e = (linf_scaled(pde, ref.pde), linf_scaled(tot, ref.tot))
    print(f"split_lattice_spectral {tag}: residual_pde {e[0]:.2e} residual_total {e[1]:.2e}")
    assert np.isfinite(pde).all() and np.isfinite(tot).all() and max(e) < TOL, e
    scaled(tag, c, ref, pde, tot)
    return pde, tot


# ---------------------------------------------------------------- 1
def test_interface_route_3_refusals_and_what_the_plan_answers():
    kind = "blocked/active_set/rhs1/lame/lines"
    c = XC.box_case((5, 4, 3), kind)
    off = XC.unsplit(c)
    assert (GENERAL, LATTICE, ANY) == (0, 1, 3)
    never = _context(c, route=None)
    assert never.split_route_info() == (GENERAL, 0) and never.kernel_path == 1
    first = _bytes(*_residuals(never, c))
    never.set_split_route(ANY)
    assert never.split_route == ANY and never.split_route_info() == (ANY, 1)
    for unknown in (2, -1):
        with pytest.raises(capi.PfmError) as e:
            never.set_split_route(unknown)
        assert e.value.status == 1 and never.split_route == ANY and never.split_route_info() == (ANY, 1)
    never.close()
    # 2-D keeps the general route
    ctx2 = make_context(cases.kat_miehe_shear_1())
    with pytest.raises(capi.PfmError) as e:
        ctx2.set_split_route(ANY)
    assert e.value.status == 5 and ctx2.split_route == GENERAL and ctx2.split_route_info() == (GENERAL, 0)
    ctx2.close()
    # lattice_residual: the split on, the path not forced to 0, and a route that carries the law of the model
    ctx = _context(c, route=None)
    for route in (GENERAL, LATTICE, ANY):
        ctx.set_split_route(route)
        for model in (SPECTRAL, VOLDEV):
            ctx.set_split_model(model)
            for split in (True, False):
                ctx.set_params(c.params if split else off.params)
                for path in (0, 1):
                    ctx.force_path(path)
                    want = int((route == ANY or (route == LATTICE and model == VOLDEV)) and split and path == 1)
                    assert ctx.split_route_info() == (route, want), (route, model, split, path)
    # (now: route 3, model 3, split off, path 1)  under model 3, route 3 is route 1 byte for byte
    ctx.set_params(c.params)
    assert ctx.split_route_info() == (ANY, 1)
    any3 = _all_bytes(ctx, c)
    ctx.set_split_route(LATTICE)
    assert ctx.split_route_info() == (LATTICE, 1)
    assert _all_bytes(ctx, c) == any3
    # model 1 on route 3: the law on the lattice kernel
    ctx.set_split_model(SPECTRAL)
    assert ctx.split_route_info() == (LATTICE, 0)
    ctx.set_split_route(ANY)
    assert ctx.split_route_info() == (ANY, 1) and ctx.kernel_path == 1
    check("interface", ctx, c, XC.ref(XC.box_case, (5, 4, 3), kind))
    # route 3 -> route 0: the bytes of a context that never set a route
    ctx.set_split_route(GENERAL)
    assert ctx.split_route_info() == (GENERAL, 0)
    assert _bytes(*_residuals(ctx, c)) == first
    ctx.close()
    # model 0: accepted, no effect
    plain = _context(off, route=None, model=capi.SPLIT_REFERENCE)
    unsplit = _bytes(*_residuals(plain, off))
    plain.set_split_route(ANY)
    assert plain.split_route_info() == (ANY, 0) and _bytes(*_residuals(plain, off)) == unsplit
    plain.close()


# ---------------------------------------------------------------- 2
@pytest.mark.parametrize("shape,kind", XC.BOX_IDS, ids=[f"{s[0]}x{s[1]}x{s[2]}-{k}" for s, k in XC.BOX_IDS])
def test_boxes_against_the_numpy_reference(shape, kind):
    c = XC.box_case(shape, kind)
    ref = XC.ref(XC.box_case, shape, kind)
    margin, share = XC.assert_mixed(c, ref)
    ctx = _context(c)
    assert ctx.kernel_path == 1 and ctx.split_route_info() == (ANY, 1)
    first = check(f"{c.name} (margin {margin:.3f}, share of the law {share:.1e})", ctx, c, ref)
    if shape == (17, 16, 5):
        assert ctx.zchunk(PFM_ZC_RES3) > 2  # the model's chunk of the six planes
        ctx.force_zchunk(PFM_ZC_RES3, 2)
        assert ctx.zchunk(PFM_ZC_RES3) == 2  # three chunks: seams at every tile edge
        assert _bytes(*check(c.name + " [z-chunks of 2]", ctx, c, ref)) == _bytes(*first)
        ctx.force_zchunk(PFM_ZC_RES3, 0)
    assert _bytes(*_residuals(ctx, c)) == _bytes(*first)
    ctx.close()


# ---------------------------------------------------------------- 3
def test_without_compression_it_is_the_unsplit_oracle():
    c = XC.one_sided_case(+1)
    XC.assert_one_sided(c, +1)
    off = cases.Case(c.name, c.mesh, c.layout, _copy(c.params, decompose_stress_matrix=0.0, decompose_stress_rhs=0.0), c.sol, c.old, c.oldold,
                     c.cu, c.ch, None, c.cell_lambda, c.cell_mu)
    r, _, _ = oracle(off, True)
    ctx = _context(c)
    assert ctx.split_route_info() == (ANY, 1)
    pde, tot = check(c.name, ctx, c, XC.ref(XC.one_sided_case, +1))
    e = (linf_scaled(pde, r.residual_pde), linf_scaled(tot, r.residual_total))
    print(f"split_lattice_spectral {c.name} against the unsplit oracle: {e[0]:.2e} / {e[1]:.2e}")
    assert max(e) < TOL
    residual_parity(off, pde, tot, r.residual_pde, r.residual_total, tag="split_lattice_spectral against the unsplit oracle")
    assert _bytes(*_residuals(ctx, c)) == _bytes(pde, tot)
    ctx.close()


def test_compression_everywhere():
    c = XC.one_sided_case(-1)
    XC.assert_one_sided(c, -1)
    ctx = _context(c)
    assert ctx.split_route_info() == (ANY, 1)
    first = check(c.name, ctx, c, XC.ref(XC.one_sided_case, -1))
    assert _bytes(*_residuals(ctx, c)) == _bytes(*first)
    ctx.close()


@pytest.mark.parametrize("kind", XC.EDGE)
def test_zero_diagonal_isotropic_strain_and_a_zero_eigenvalue(kind):
    c = XC.edge_case(kind)
    XC.assert_edge(c)
    ctx = _context(c)
    assert ctx.split_route_info() == (ANY, 1)
    first = check(c.name, ctx, c, XC.ref(XC.edge_case, kind))
    assert _bytes(*_residuals(ctx, c)) == _bytes(*first)
    ctx.sync_status()
    ctx.close()


# ---------------------------------------------------------------- 4
@pytest.mark.parametrize("blocked", [True, False])
def test_two_ranks_and_both_halves_of_the_overlapped_assembly(blocked):
    """(33, 5, 4) cells in two ranks along x, 17 node planes each: a tile that reads no ghost and one that does.  OP.run_phases:
    the whole assembly against the reference, phase 1 with poisoned ghosts writes only final values, phase 1 + phase 2 and
    the repeated whole assembly equal the whole assembly bit for bit."""
    import test_gpu_overlap_phases as OP

    c = XC.two_rank_case(blocked)
    r = XC.ref(XC.two_rank_case, blocked)
    XC.assert_mixed(c, r)
    ref = OP.Reference(c.layout, None, r.pde, r.tot, c.sol, *r.matrices())
    single = _context(c)
    assert single.split_route_info() == (ANY, 1)
    one = check(c.name + " (one rank)", single, c, r)
    single.close()
    ranks = OP.box_ranks(XC.unsplit(c), XC.TWO_RANK_N, (2, 1, 1))
    for rk in ranks:
        rk.ctx.set_split_model(SPECTRAL)
        rk.ctx.set_split_route(ANY)
        rk.ctx.set_params(c.params)
        assert rk.lp.n_owned < rk.lp.mesh.n_nodes and rk.ctx.kernel_path == 1 and rk.ctx.split_route_info() == (ANY, 1)
    recv = OP.exchange_ghosts([rk.lp for rk in ranks], [rk.ctx for rk in ranks], 3)
    for rk, buf in zip(ranks, recv):
        W, p1 = OP.run_phases(rk, buf, True, ref)
        no, gi = rk.lp.n_owned, rk.lp.global_ids
        nn, cc = np.repeat(np.arange(no), 4), np.tile(np.arange(4), no)
        ld, gd = M.DofLayout(no, 3, blocked).dof(nn, cc), c.layout.dof(gi[nn], cc)
        for k in (0, 1):
            e = linf_scaled(W[k][ld], one[k][gd])
            share = OP._share(p1[k])
            print(f"split_lattice_spectral {c.name} rank {rk.index} output {k}: against the single rank {e:.2e} "
                  f"(same bits: {OP._same_bits(W[k][ld], one[k][gd])}), phase 1 wrote {share:.2f}")
            assert e < TOL
            # (a rank against the single rank, owned rows only: the parts at their own scale)
            PS.assert_parts(W[k][ld], one[k][gd], cc == 3, TOL, f"split_lattice_spectral {c.name} rank {rk.index} output {k}")
            assert 0.0 < share < 1.0, "each sub-box has interior and boundary tiles"
        rk.ctx.close()


# ---------------------------------------------------------------- 5
def _rows_without_atomics(c):
    """The dofs of the nodes that no cell with a hanging vertex touches, neither as a vertex nor as a parent of one of its
    hanging vertices: what the general family adds to them comes from its ordered classes alone."""
    mesh = c.mesh
    hang = np.zeros(mesh.n_nodes, bool)
    hang[mesh.hn_nodes] = True
    touched = np.zeros(mesh.n_nodes, bool)
    touched[mesh.cells[hang[mesh.cells].any(axis=1)].ravel()] = True
    touched[mesh.hn_parents] = True
    nodes = np.nonzero(~touched)[0]
    assert 0 < nodes.size < mesh.n_nodes
    return np.sort(np.concatenate([c.layout.dof(nodes, comp) for comp in range(4)]))


def test_overlay_level_lattices_with_the_law_and_the_general_family_for_the_rest():
    """The cells at hanging vertices stay with the general family, whose spectral instantiations add with atomics: within the
    bar, but no same-bytes assertion across runs of the residual-only call."""
    c = XC.block_case()
    ref = XC.ref(XC.block_case)
    XC.assert_mixed(c, ref)
    un = _context(XC.unsplit(c))
    info = un.overlay_info()
    assert un.kernel_path == 3 and info[0] > 0 and 0 < info[1] < c.mesh.n_cells and un.split_route_info() == (ANY, 0)
    un.close()
    ctx = _context(c)
    assert ctx.kernel_path == 3 and ctx.overlay_info() == info and ctx.split_route_info() == (ANY, 1)
    first = check(c.name, ctx, c, ref)
    values, res = _full(ctx, c)
    assert linf_scaled(res, ref.pde) < TOL
    scaled(c.name + " full assembly", c, ref, res)
    ctx.set_split_route(GENERAL)
    assert ctx.split_route_info() == (GENERAL, 0) and ctx.overlay_info() == info
    values_g, res_g = _full(ctx, c)
    rows = _rows_without_atomics(c)
    A, A_g = _matrix(ctx, c, values), _matrix(ctx, c, values_g)
    assert _bytes(res[rows], A[rows].data) == _bytes(res_g[rows], A_g[rows].data)  # the full assembly does not follow the route
    assert linf_scaled(res, res_g) < TOL
    general = check(c.name + " [general route]", ctx, c, ref)
    print(f"split_lattice_spectral {c.name}: lattice against general route {linf_scaled(first[0], general[0]):.2e} / "
          f"{linf_scaled(first[1], general[1]):.2e}, {rows.size} of {c.layout.n_dofs} rows without atomics")
    ctx.close()


# ---------------------------------------------------------------- 6
@pytest.mark.parametrize("shape,kind", [((17, 16, 5), "blocked/active_set/rhs1/lame/lines"), ((5, 4, 3), "interleaved/monolithic/rhs1/lines/use_old")])
def test_fused_entry_equals_the_three_call_sequence(shape, kind):
    """pfm_assemble_nl_residual_device on a single-rank box: the kernel reads d_solution itself and publishes the node state"""
    import torch

    from test_gpu_line_search import same_bits

    c = XC.box_case(shape, kind)
    n = c.layout.n_dofs
    ctx = _context(c)
    assert ctx.split_route_info() == (ANY, 1)
    sol = torch.from_numpy(c.sol).cuda()
    other = np.where(np.arange(n) % 2 == 0, 0.25, -0.5) * np.ones(n)  # the node state before the call: not the solution
    outs, funcs = [], []
    for fused in (False, True):
        ctx.state_set_host(other, c.old, c.oldold)
        pde, tot = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda"), torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        if fused:
            ctx.assemble_nl_residual_device(sol.data_ptr(), pde.data_ptr(), tot.data_ptr())
        else:
            ctx.state_set_solution_device(sol.data_ptr())
            ctx.assemble_device(True, [], pde.data_ptr(), tot.data_ptr())
        ctx.sync_status()
        torch.cuda.synchronize()
        outs.append((pde.cpu().numpy(), tot.cpu().numpy()))
        funcs.append(ctx.functionals())
    ref = XC.ref(XC.box_case, shape, kind)
    assert linf_scaled(outs[1][0], ref.pde) < TOL and linf_scaled(outs[1][1], ref.tot) < TOL
    scaled("fused entry", c, ref, outs[1][0], outs[1][1])
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1])
    assert same_bits(np.asarray(funcs[0]), np.asarray(funcs[1])) and np.isfinite(funcs[1]).all()
    ctx.close()


# ---------------------------------------------------------------- 7
@pytest.mark.parametrize("blocked,solver,norm,restore", [(True, 0, "l2", "saved"), (False, 1, "linf", "subtract")])
def test_device_line_search_under_routes_0_and_3(blocked, solver, norm, restore):
    """The reference norm comes from newton.line_search_numpy around the numpy reference (XC.line_search_numpy_case): every
    accept / reject comparison of that search is decided by a relative gap >= 1e-9, a thousand times the bar."""
    import test_gpu_line_search as LS

    c = XC.line_search_case(blocked, solver)
    upd, trials, reference, numpy_search, _ = XC.line_search_numpy_case(blocked, solver, norm, restore)
    assert all(abs(reference - t) >= XC.LS_GAP * abs(reference) for t in trials), (reference, trials)
    ctxs = {GENERAL: _context(c, route=GENERAL), ANY: _context(c, route=ANY)}
    assert ctxs[GENERAL].split_route_info() == (GENERAL, 0) and ctxs[ANY].split_route_info() == (ANY, 1)
    got = {}
    for route, ctx in ctxs.items():
        w, g = LS._run_both(ctx, c, upd, reference, XC.LS_MAX_STEPS, norm, restore)
        LS._compare(c, w, g, True)  # the loop is the composition of the entries bit for bit, on either route
        got[route] = g
    g, l = got[GENERAL], got[ANY]
    print("split_lattice_spectral line search: numpy trial norms", trials, "reference", reference, "|", g["steps"], g["accepted"], g["norms"], "|",
          l["steps"], l["accepted"], l["norms"])
    assert l["steps"] == g["steps"] == numpy_search["steps"] and l["accepted"] == g["accepted"] == numpy_search["accepted"]
    assert all(abs(a - b) <= 1e-12 * abs(b) for a, b in zip(l["norms"], g["norms"]))
    assert LS.same_bits(l["vec"]["sol"][0], g["vec"]["sol"][0])  # a function of the step count alone
    assert LS.same_bits(l["vec"]["sol"][0], numpy_search["solution"])
    for k in ("pde", "tot"):
        assert linf_scaled(l["vec"][k][0], g["vec"][k][0]) < TOL
        PS.assert_parts(l["vec"][k][0], g["vec"][k][0], PS.is_phi(c.layout), TOL, f"split_lattice_spectral line search, route against route, {k}")
    r = XC.Ref(c, l["vec"]["sol"][0])
    assert linf_scaled(l["vec"]["pde"][0], r.pde) < TOL and linf_scaled(l["vec"]["tot"][0], r.tot) < TOL
    scaled("line search, accepted vector", c, r, l["vec"]["pde"][0], l["vec"]["tot"][0])
    for ctx in ctxs.values():
        ctx.close()


# ---------------------------------------------------------------- 8
def test_one_living_context_through_routes_and_models():
    """unsplit -> route 3 model 1 -> unsplit -> route 0 -> route 3 model 3 -> route 3 model 1 on (17, 16, 5): every repeat gives
    the bytes of its first run (full assembly and residual-only call), the context stays a lattice context"""
    shape, kind = (17, 16, 5), "interleaved/active_set/rhs0.5/lame/lines"
    c = XC.box_case(shape, kind)
    off = XC.unsplit(c)
    ref = XC.ref(XC.box_case, shape, kind)
    ctx = _context(off, route=GENERAL)

    def run(case, route, model, want):
        ctx.set_split_model(model)
        ctx.set_split_route(route)
        ctx.set_params(case.params)
        assert ctx.kernel_path == 1 and ctx.split_route_info() == (route, want)
        values, res = _full(ctx, case)
        pde, tot = _residuals(ctx, case)
        assert ctx.kernel_path == 1
        return _bytes(*values, res, pde, tot), (pde, tot)

    unsplit, _ = run(off, GENERAL, SPECTRAL, 0)
    lattice, (pde, tot) = run(c, ANY, SPECTRAL, 1)
    assert linf_scaled(pde, ref.pde) < TOL and linf_scaled(tot, ref.tot) < TOL
    scaled("living context, route 3 model 1", c, ref, pde, tot)
    assert run(off, ANY, SPECTRAL, 0)[0] == unsplit
    general, (pde_g, tot_g) = run(c, GENERAL, SPECTRAL, 0)
    assert linf_scaled(pde_g, ref.pde) < TOL and linf_scaled(tot_g, ref.tot) < TOL
    scaled("living context, route 0 model 1", c, ref, pde_g, tot_g)
    assert general[:-2] == lattice[:-2]  # the full assembly does not follow the route
    voldev, _ = run(c, ANY, VOLDEV, 1)
    assert run(c, LATTICE, VOLDEV, 1)[0] == voldev and voldev[-2:] != lattice[-2:]  # another law
    again, _ = run(c, ANY, SPECTRAL, 1)
    assert again == lattice
    assert run(c, GENERAL, SPECTRAL, 0)[0] == general and run(off, GENERAL, SPECTRAL, 0)[0] == unsplit
    ctx.close()
