"""The volumetric-deviatoric split residual on the row-owner lattice kernels (pfm_set_split_route, PFM_SPLIT_ROUTE_LATTICE:
k_cart_residual3<false, true> of cracks_amd/csrc/pfm_cart.hip, CartPlan::voldev), through the C ABI:

1. the interface: default, refusals, what pfm_ctx_split_route answers, and a context that never set a route against one
   that went LATTICE -> GENERAL, byte for byte;
2. boxes against the numpy reference, both layouts, both solvers, decompose_stress_rhs 0 / 1, per-cell Lame, Dirichlet faces
   with an active set, use_old_timestep_pf; two z-chunk lengths give the same bytes;
3. one-sided states, zero strain and a pure shear;
4. two ranks on one GPU: owned rows against the single rank, the halves of the overlapped assembly bit for bit;
5. the overlay: level lattices with the law, the general family for the rest;
6. the fused entry pfm_assemble_nl_residual_device against its three-call form, bit for bit;
7. pfm_line_search_device under both routes;
8. one living context through unsplit -> LATTICE -> unsplit -> GENERAL -> LATTICE.

States, references and the conditions on them: tests/split_lattice_cases.py (run on the CPU by
tests/test_split_lattice_ref_cpu.py).  Bar: |x - x_ref|_inf < 1e-12 max(1, |x_ref|_inf) (gpu_util.TOL)."""
import numpy as np
import pytest

import cases
import line_search_cases as L
import split_lattice_cases as LC
import split_voldev_cases as SC
from cracks_amd import capi
from cracks_amd import mesh as M
from cracks_amd.assembler import Context, node_flags_from_dof_flags
import parity_scale as PS
from gpu_util import TOL, linf_scaled, make_context, oracle, residual_parity
from test_gpu_split3d import _copy
from test_gpu_split3d_routes import smallest_edge

pytestmark = pytest.mark.gpu

GENERAL, LATTICE = capi.SPLIT_ROUTE_GENERAL, capi.SPLIT_ROUTE_LATTICE
PFM_ZC_RES3 = 2  # pfm_ctx_force_zchunk: k_cart_residual3


def _context(c, route=LATTICE, model=capi.SPLIT_VOLDEV, **kw):
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


def check(tag, ctx, c, ref):
    """the residual-only call against the reference; returns (residual_pde, residual_total)"""
    pde, tot = _residuals(ctx, c)
    e = (linf_scaled(pde, ref.pde), linf_scaled(tot, ref.tot))
    print(f"split_lattice {tag}: residual_pde {e[0]:.2e} residual_total {e[1]:.2e}")
    assert np.isfinite(pde).all() and np.isfinite(tot).all() and max(e) < TOL, e
    scaled(tag, c, ref, pde, tot)
    return pde, tot


def scaled(tag, c, ref, pde=None, tot=None):
    """per row and per part (tests/parity_scale.py), the scales from the reference's own Jacobian of the state"""
    A_ref, A_tot = ref.matrices()
    if pde is not None:
        PS.assert_residual(pde, ref.pde, A_ref, c.layout, ref._sol, TOL, f"split_lattice {tag} residual_pde")
    if tot is not None:
        PS.assert_residual(tot, ref.tot, A_tot, c.layout, ref._sol, TOL, f"split_lattice {tag} residual_total")


# ---------------------------------------------------------------- 1
def test_interface_default_refusals_and_what_the_plan_answers():
    c = LC.box_case((5, 4, 3), "blocked/active_set/rhs1/lame/lines")
    off = LC.unsplit(c)
    assert (GENERAL, LATTICE) == (0, 1)
    never = _context(c, route=None)
    assert never.split_route == GENERAL and never.split_route_info() == (GENERAL, 0) and never.kernel_path == 1
    for unknown in (2, -1):
        with pytest.raises(capi.PfmError) as e:
            never.set_split_route(unknown)
        assert e.value.status == 1 and never.split_route == GENERAL and never.split_route_info() == (GENERAL, 0)
    first = _bytes(*_residuals(never, c))
    never.close()
    # 2-D keeps the general route
    c2 = cases.kat_miehe_shear_1()
    ctx2 = make_context(c2)
    with pytest.raises(capi.PfmError) as e:
        ctx2.set_split_route(LATTICE)
    assert e.value.status == 5 and ctx2.split_route == GENERAL and ctx2.split_route_info() == (GENERAL, 0)
    ctx2.set_split_route(GENERAL)
    ctx2.close()
    # lattice_residual: exactly model 3, the split on, the path not forced to 0 -- and the route
    ctx = _context(c, route=None)
    for route in (GENERAL, LATTICE):
        ctx.set_split_route(route)
        for model in (capi.SPLIT_SPECTRAL, capi.SPLIT_VOLDEV):
            ctx.set_split_model(model)
            for split in (True, False):
                ctx.set_params(c.params if split else off.params)
                for path in (0, 1):
                    ctx.force_path(path)
                    want = int(route == LATTICE and model == capi.SPLIT_VOLDEV and split and path == 1)
                    assert ctx.split_route_info() == (route, want), (route, model, split, path)
    # (now: LATTICE, model 3, split off, path 1)  model 1 is accepted and stays with the general family
    ctx.set_params(c.params)
    ctx.set_split_model(capi.SPLIT_SPECTRAL)
    ctx.set_split_route(LATTICE)
    assert ctx.split_route_info() == (LATTICE, 0) and ctx.split_route == LATTICE
    ctx.set_split_model(capi.SPLIT_VOLDEV)
    assert ctx.split_route_info() == (LATTICE, 1) and ctx.kernel_path == 1
    check("interface", ctx, c, LC.ref(LC.box_case, (5, 4, 3), "blocked/active_set/rhs1/lame/lines"))
    # LATTICE -> GENERAL: the bytes of a context that never set a route
    ctx.set_split_route(GENERAL)
    assert ctx.split_route_info() == (GENERAL, 0)
    assert _bytes(*_residuals(ctx, c)) == first
    ctx.close()


# ---------------------------------------------------------------- 2
@pytest.mark.parametrize("shape,kind", LC.BOX_IDS, ids=[f"{s[0]}x{s[1]}x{s[2]}-{k}" for s, k in LC.BOX_IDS])
def test_boxes_against_the_numpy_reference(shape, kind):
    c = LC.box_case(shape, kind)
    share, margin = SC.assert_mixed(c)
    ref = LC.ref(LC.box_case, shape, kind)
    ctx = _context(c)
    assert ctx.kernel_path == 1 and ctx.split_route_info() == (LATTICE, 1)
    first = check(f"{c.name} (share {share:.2f}, margin {margin:.1e})", ctx, c, ref)
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
    c = LC.one_sided_case(+1)
    SC.assert_one_sided(c, +1)
    off = cases.Case(c.name, c.mesh, c.layout, _copy(c.params, decompose_stress_matrix=0.0, decompose_stress_rhs=0.0), c.sol, c.old, c.oldold,
                     c.cu, c.ch, None, c.cell_lambda, c.cell_mu)
    r, _, _ = oracle(off, True)
    ctx = _context(c)
    assert ctx.split_route_info() == (LATTICE, 1)
    pde, tot = _residuals(ctx, c)
    e = (linf_scaled(pde, r.residual_pde), linf_scaled(tot, r.residual_total))
    print(f"split_lattice {c.name} against the unsplit oracle: {e[0]:.2e} / {e[1]:.2e}")
    assert max(e) < TOL
    residual_parity(off, pde, tot, r.residual_pde, r.residual_total, tag="split_lattice against the unsplit oracle")
    ctx.close()


def test_compression_everywhere():
    c = LC.one_sided_case(-1)
    SC.assert_one_sided(c, -1)
    ctx = _context(c)
    assert ctx.split_route_info() == (LATTICE, 1)
    check(c.name, ctx, c, LC.ref(LC.one_sided_case, -1))
    ctx.close()


@pytest.mark.parametrize("kind", ["zero", "shear"])
def test_zero_strain_and_pure_shear(kind):
    c = LC.edge_case(kind)
    SC.assert_edge(c)
    ctx = _context(c)
    assert ctx.split_route_info() == (LATTICE, 1)
    first = check(c.name, ctx, c, LC.ref(LC.edge_case, kind))
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

    c = LC.two_rank_case(blocked)
    SC.assert_mixed(c)
    r = LC.ref(LC.two_rank_case, blocked)
    ref = OP.Reference(c.layout, None, r.pde, r.tot, c.sol, *r.matrices())
    single = _context(c)
    assert single.split_route_info() == (LATTICE, 1)
    one = check(c.name + " (one rank)", single, c, r)
    single.close()
    ranks = OP.box_ranks(LC.unsplit(c), LC.TWO_RANK_N, (2, 1, 1))
    for rk in ranks:
        rk.ctx.set_split_model(capi.SPLIT_VOLDEV)
        rk.ctx.set_split_route(LATTICE)
        rk.ctx.set_params(c.params)
        assert rk.lp.n_owned < rk.lp.mesh.n_nodes and rk.ctx.kernel_path == 1 and rk.ctx.split_route_info() == (LATTICE, 1)
    recv = OP.exchange_ghosts([rk.lp for rk in ranks], [rk.ctx for rk in ranks], 3)
    for rk, buf in zip(ranks, recv):
        W, p1 = OP.run_phases(rk, buf, True, ref)
        no, gi = rk.lp.n_owned, rk.lp.global_ids
        nn, cc = np.repeat(np.arange(no), 4), np.tile(np.arange(4), no)
        ld, gd = M.DofLayout(no, 3, blocked).dof(nn, cc), c.layout.dof(gi[nn], cc)
        for k in (0, 1):
            e = linf_scaled(W[k][ld], one[k][gd])
            share = OP._share(p1[k])
            print(f"split_lattice {c.name} rank {rk.index} output {k}: against the single rank {e:.2e} "
                  f"(same bits: {OP._same_bits(W[k][ld], one[k][gd])}), phase 1 wrote {share:.2f}")
            assert e < TOL
            # (a rank against the single rank, owned rows only: the parts at their own scale)
            PS.assert_parts(W[k][ld], one[k][gd], cc == 3, TOL, f"split_lattice {c.name} rank {rk.index} output {k}")
            assert 0.0 < share < 1.0, "each sub-box has interior and boundary tiles"
        rk.ctx.close()


# ---------------------------------------------------------------- 5
def test_overlay_level_lattices_with_the_law_and_the_general_family_for_the_rest():
    c = LC.block_case()
    SC.assert_mixed(c)
    ref = LC.ref(LC.block_case)
    un = _context(LC.unsplit(c))
    info = un.overlay_info()
    assert un.kernel_path == 3 and info[0] > 0 and 0 < info[1] < c.mesh.n_cells and un.split_route_info() == (LATTICE, 0)
    un.close()
    ctx = _context(c)
    assert ctx.kernel_path == 3 and ctx.overlay_info() == info and ctx.split_route_info() == (LATTICE, 1)
    first = check(c.name, ctx, c, ref)
    assert _bytes(*_residuals(ctx, c)) == _bytes(*first)
    values, res = _full(ctx, c)
    assert linf_scaled(res, ref.pde) < TOL
    scaled(c.name + " full assembly", c, ref, res)
    ctx.set_split_route(GENERAL)
    assert ctx.split_route_info() == (GENERAL, 0) and ctx.overlay_info() == info
    values_g, res_g = _full(ctx, c)
    assert _bytes(*values, res) == _bytes(*values_g, res_g)
    general = check(c.name + " [general route]", ctx, c, ref)
    print(f"split_lattice {c.name}: lattice against general route {linf_scaled(first[0], general[0]):.2e} / {linf_scaled(first[1], general[1]):.2e}")
    ctx.close()


# ---------------------------------------------------------------- 6
@pytest.mark.parametrize("shape,kind", [((17, 16, 5), "blocked/active_set/rhs1/lame/lines"), ((5, 4, 3), "interleaved/monolithic/rhs1/lines/use_old")])
def test_fused_entry_equals_the_three_call_sequence(shape, kind):
    """pfm_assemble_nl_residual_device on a single-rank box: the kernel reads d_solution itself and publishes the node state"""
    import torch

    from test_gpu_line_search import same_bits

    c = LC.box_case(shape, kind)
    n = c.layout.n_dofs
    ctx = _context(c)
    assert ctx.split_route_info() == (LATTICE, 1)
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
    ref = LC.ref(LC.box_case, shape, kind)
    assert linf_scaled(outs[1][0], ref.pde) < TOL and linf_scaled(outs[1][1], ref.tot) < TOL
    scaled("fused entry", c, ref, outs[1][0], outs[1][1])
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1])
    assert same_bits(np.asarray(funcs[0]), np.asarray(funcs[1])) and np.isfinite(funcs[1]).all()
    ctx.close()


# ---------------------------------------------------------------- 7
@pytest.mark.parametrize("blocked,solver,norm,restore", [(True, 0, "l2", "saved"), (False, 1, "linf", "subtract")])
def test_device_line_search_under_both_routes(blocked, solver, norm, restore):
    import test_gpu_line_search as LS

    c = LC.line_search_case(blocked, solver)
    SC.assert_mixed(c)
    upd = L.newton_update(c, seed=5, u_amp=2e-4 * smallest_edge(c.mesh), phi_amp=0.5)
    ctxs = {GENERAL: _context(c, route=GENERAL), LATTICE: _context(c, route=LATTICE)}
    assert ctxs[GENERAL].split_route_info() == (GENERAL, 0) and ctxs[LATTICE].split_route_info() == (LATTICE, 1)
    want, _ = LS._run_both(ctxs[GENERAL], c, upd, 0.0, 4, norm, restore)  # exhaustion: the norm of every trial
    trials = want["trials"]
    print("split_lattice line search: trial norms of the general route", trials)
    # accepted at trial 2 where the norms fall as they do on these states, at trial 0 otherwise
    reference = 0.5 * (trials[2] + min(trials[:2])) if trials[2] < min(trials[:2]) else 2.0 * max(trials)
    assert all(abs(reference - t) >= 1e-6 * abs(reference) for t in trials), (reference, trials)
    got = {}
    for route, ctx in ctxs.items():
        w, g = LS._run_both(ctx, c, upd, reference, 4, norm, restore)
        LS._compare(c, w, g, True)  # the loop is the composition of the entries bit for bit, on either route
        got[route] = g
    g, l = got[GENERAL], got[LATTICE]
    print("split_lattice line search:", g["steps"], g["accepted"], g["norms"], "|", l["steps"], l["accepted"], l["norms"])
    assert l["steps"] == g["steps"] and l["accepted"] == g["accepted"]
    assert all(abs(a - b) < TOL * max(1.0, abs(b)) for a, b in zip(l["norms"], g["norms"]))
    assert LS.same_bits(l["vec"]["sol"][0], g["vec"]["sol"][0])  # a function of the step count alone
    for k in ("pde", "tot"):
        assert linf_scaled(l["vec"][k][0], g["vec"][k][0]) < TOL
        PS.assert_parts(l["vec"][k][0], g["vec"][k][0], PS.is_phi(c.layout), TOL, f"split_lattice line search, route against route, {k}")
    r = LC.Ref(c, l["vec"]["sol"][0])
    assert linf_scaled(l["vec"]["pde"][0], r.pde) < TOL and linf_scaled(l["vec"]["tot"][0], r.tot) < TOL
    scaled("line search, accepted vector", c, r, l["vec"]["pde"][0], l["vec"]["tot"][0])
    for ctx in ctxs.values():
        ctx.close()


# ---------------------------------------------------------------- 8
def test_one_living_context_through_both_routes():
    """unsplit -> model 3 LATTICE -> unsplit -> model 3 GENERAL -> model 3 LATTICE on (17, 16, 5): every repeat gives the bytes
    of its first run (full assembly and residual-only call), the context stays a lattice context"""
    shape, kind = (17, 16, 5), "interleaved/active_set/rhs0.5/lame/lines"
    c = LC.box_case(shape, kind)
    off = LC.unsplit(c)
    ref = LC.ref(LC.box_case, shape, kind)
    ctx = _context(off, route=GENERAL)

    def run(case, route, want):
        ctx.set_split_route(route)
        ctx.set_params(case.params)
        assert ctx.kernel_path == 1 and ctx.split_route_info() == (route, want)
        values, res = _full(ctx, case)
        pde, tot = _residuals(ctx, case)
        assert ctx.kernel_path == 1
        return _bytes(*values, res, pde, tot), (pde, tot)

    unsplit, _ = run(off, GENERAL, 0)
    lattice, (pde, tot) = run(c, LATTICE, 1)
    assert linf_scaled(pde, ref.pde) < TOL and linf_scaled(tot, ref.tot) < TOL
    scaled("living context, lattice route", c, ref, pde, tot)
    assert run(off, LATTICE, 0)[0] == unsplit
    general, (pde_g, tot_g) = run(c, GENERAL, 0)
    assert linf_scaled(pde_g, ref.pde) < TOL and linf_scaled(tot_g, ref.tot) < TOL
    scaled("living context, general route", c, ref, pde_g, tot_g)
    assert general[:-2] == lattice[:-2]  # the full assembly does not follow the route
    again, _ = run(c, LATTICE, 1)
    assert again == lattice
    assert run(c, GENERAL, 0)[0] == general and run(off, GENERAL, 0)[0] == unsplit
    ctx.close()
