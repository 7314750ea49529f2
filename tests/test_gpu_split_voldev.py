"""The volumetric-deviatoric stress split of 3-D assemblies (pfm_set_split_model, PFM_SPLIT_VOLDEV; the law in
cracks_amd/csrc/pfm_split3.h, the VOLDEV instantiations of k_assemble_general):

1. the model is accepted on 3-D contexts only, the unknown models stay refused;
2. entry by entry against the numpy reference (tests/split_voldev_ref.py) on the general family and on a box context;
3. tr E >= 0 everywhere reproduces the unsplit oracle through every scatter path;
4. tr E < 0 everywhere against the reference;
5. hanging nodes with Dirichlet lines, an active set and per-cell Lame: the scratch + gather route, the same bytes twice;
6. one living overlay context through unsplit -> model 3 -> unsplit -> model 1 -> model 3;
7. two ranks and both halves of the overlapped assembly;
8. the device line search on a model-3 context;
9. zero strain and a pure shear with tr E exactly 0.

States and the conditions on them: tests/split_voldev_cases.py (run on the CPU by tests/test_split_voldev_ref_cpu.py).
Bar: |x - x_ref|_inf < 1e-12 max(1, |x_ref|_inf) (gpu_util.TOL).  Measured deviations (MI355X): DESIGN.md §2."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import cases
import line_search_cases as L
import split3d_ref as R
import split_voldev_cases as SC
import split_voldev_ref as V
from cracks_amd import capi
from cracks_amd.assembler import Context, node_flags_from_dof_flags
import parity_scale as PS
from gpu_util import TOL, linf_scaled, make_context, oracle, reference_parity, total_matrix
from test_gpu_split3d import _copy, _matrix
from test_gpu_split3d_routes import constrained_rows_hold_their_placeholder, smallest_edge

pytestmark = pytest.mark.gpu


def _context(c, model=capi.SPLIT_VOLDEV, **kw):
    ctx = Context(c.mesh, c.layout.blocked, cell_lambda=c.cell_lambda, cell_mu=c.cell_mu, **kw)
    ctx.set_split_model(model)
    ctx.set_params(c.params)
    ctx.set_constraints(node_flags_from_dof_flags(c.layout, c.cu.flag, c.ch.flag))
    return ctx


class Ref:
    """the reference of one case: matrix on the oracle's pattern, residual (of both calls), residual_total"""

    def __init__(self, c, law=V):
        Ke, Re, self.E = law.element_matrices(c.mesh, c.layout, c.params, c.sol, c.old, c.oldold, c.cell_lambda, c.cell_mu)
        self.A, self.res = R.distribute_matrix(c.mesh, c.layout, Ke, Re, c.cu)
        self.tot = R.residual_total(c.layout, c.mesh.cells, c.params, Re, c.cu, c.ch)
        # the matrix whose rows belong to residual_total (the scales of tests/parity_scale.py): under the active-set scheme the
        # same element matrices distributed with the hanging-node constraints alone
        self.A_tot = self.A if c.params.outer_solver != 0 else R.distribute_matrix(c.mesh, c.layout, Ke, Re, c.ch)[0]


@functools.lru_cache(maxsize=None)
def _ref(case, *args):
    return Ref(case(*args))


def _outputs(ctx, c):
    values, res, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
    _, pde, tot = ctx.assemble_host(c.sol, c.old, c.oldold, True)
    return values, res, pde, tot


def _bytes(out):
    values, res, pde, tot = out
    return [v.tobytes() for v in values] + [res.tobytes(), pde.tobytes(), tot.tobytes()]


def check(tag, ctx, c, ref):
    """full assembly and the residual-only call against the reference; returns the outputs"""
    out = _outputs(ctx, c)
    A = _matrix(ctx, c, out[0])
    if c.cu.flag.any():
        assert A.nnz == ref.A.nnz and (A.indptr == ref.A.indptr).all() and (A.indices == ref.A.indices).all()
        e_A = linf_scaled(A.data, ref.A.data)
    else:
        e_A = float(abs(A - ref.A).max()) / max(1.0, float(abs(ref.A).max()))
    e = (e_A, linf_scaled(out[1], ref.res), linf_scaled(out[2], ref.res), linf_scaled(out[3], ref.tot))
    print(f"split_voldev {tag}: matrix {e[0]:.2e} residual {e[1]:.2e} residual-only {e[2]:.2e} / {e[3]:.2e}")
    assert all(np.isfinite(v).all() for v in out[0]) and max(e) < TOL, e
    reference_parity(c.layout, c.sol, A, ref.A, [(out[1], ref.res, "pde"), (out[2], ref.res, "pde"), (out[3], ref.tot, "tot")], tag=f"split_voldev {tag}",
                     A_tot=ref.A_tot)
    return out


def check_unsplit_oracle(tag, ctx, c):
    """a context with the split on against the oracle with the split off: matrix, residual, both residuals of the second call"""
    off = cases.Case(c.name, c.mesh, c.layout, _copy(c.params, decompose_stress_matrix=0.0, decompose_stress_rhs=0.0), c.sol, c.old, c.oldold,
                     c.cu, c.ch, None, c.cell_lambda, c.cell_mu)
    r, rowptr, colind = oracle(off, False)
    r2, _, _ = oracle(off, True)
    out = _outputs(ctx, c)
    A = _matrix(ctx, c, out[0])
    A_ref = sp.csr_matrix((r.values, colind, rowptr), shape=A.shape)
    assert A.nnz == A_ref.nnz and (A.indices == A_ref.indices).all()
    e = (linf_scaled(A.data, A_ref.data), linf_scaled(out[1], r.residual_pde), linf_scaled(out[2], r2.residual_pde),
         linf_scaled(out[3], r2.residual_total))
    print(f"split_voldev {tag} against the unsplit oracle: matrix {e[0]:.2e} residual {e[1]:.2e} residual-only {e[2]:.2e} / {e[3]:.2e}")
    assert all(np.isfinite(v).all() for v in out[0]) and max(e) < TOL, e
    reference_parity(c.layout, c.sol, A, A_ref, [(out[1], r.residual_pde, "pde"), (out[2], r2.residual_pde, "pde"), (out[3], r2.residual_total, "tot")],
                     tag=f"split_voldev {tag} against the unsplit oracle", A_tot=total_matrix(off, A_ref))
    return out


# ---------------------------------------------------------------- 1
def test_model_3_is_accepted_in_3d_and_unknown_models_stay_refused():
    c = cases.perturbed(cases.kat_sneddon_3d(4))
    split = _copy(c.params, decompose_stress_rhs=1.0, decompose_stress_matrix=1.0, timestep_number=1)
    assert capi.SPLIT_VOLDEV == 3
    ctx = make_context(c)
    for unknown in (2, -1):
        with pytest.raises(capi.PfmError) as e:
            ctx.set_split_model(unknown)
        assert e.value.status == 1 and ctx.split_model == 0
    ctx.set_split_model(capi.SPLIT_VOLDEV)
    assert ctx.split_model == 3
    ctx.set_params(split)
    assert ctx.kernel_path == 1  # a box context: the general family takes the split assembly
    values, res, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
    assert np.isfinite(res).all() and all(np.isfinite(v).all() for v in values) and np.abs(values[0]).max() > 0 and np.abs(res).max() > 0
    _, res2, tot2 = ctx.assemble_host(c.sol, c.old, c.oldold, True)
    assert linf_scaled(res2, res) < TOL and np.isfinite(tot2).all()
    # back at model 0 with the split parameters still set: the launcher refuses, the parameters are refused again
    ctx.set_split_model(capi.SPLIT_REFERENCE)
    with pytest.raises(capi.PfmError) as e:
        ctx.assemble_host(c.sol, c.old, c.oldold, True)
    assert e.value.status == 5
    with pytest.raises(capi.PfmError) as e:
        ctx.set_params(split)
    assert e.value.status == 5
    ctx.close()
    # 2-D keeps the reference's closed form
    c2 = cases.kat_miehe_shear_1()
    ctx2 = make_context(c2)
    with pytest.raises(capi.PfmError) as e:
        ctx2.set_split_model(capi.SPLIT_VOLDEV)
    assert e.value.status == 5 and ctx2.split_model == 0
    ctx2.close()


# ---------------------------------------------------------------- 2
@pytest.mark.parametrize("kind,blocked,d,cell_lame", SC.ENTRY)
def test_entry_by_entry_against_the_numpy_reference(kind, blocked, d, cell_lame):
    """(5, 4, 3) hexes: the colour class of the even cells has 12 of them -- two workgroups of the 32-lane Jacobian form."""
    c = SC.entry_case(kind, blocked, d, cell_lame)
    share, margin = SC.assert_mixed(c)
    ref = _ref(SC.entry_case, kind, blocked, d, cell_lame)
    ctx = _context(c)
    assert ctx.kernel_path == (0 if kind == "general" else 1)
    check(f"{c.name} (share {share:.2f}, margin {margin:.1e})", ctx, c, ref)
    if kind == "box":
        # split off again: the context returns to its own kernels, which must equal the oracle
        from test_gpu_overlay3d import check_against_oracle

        off = cases.Case("off", c.mesh, c.layout, _copy(c.params, timestep_number=0), c.sol, c.old, c.oldold, c.cu, c.ch, None, c.cell_lambda, c.cell_mu)
        ctx.set_params(off.params)
        assert ctx.kernel_path == 1
        check_against_oracle(off, ctx)
    ctx.close()


# ---------------------------------------------------------------- 3
@pytest.mark.parametrize("solver", [0, 1], ids=["active_set", "monolithic"])
def test_without_compression_it_is_the_unsplit_oracle_with_dirichlet_and_active_set_flags(solver):
    c = SC.tension_case(solver)
    SC.assert_one_sided(c, +1)
    ctx = _context(c)
    check_unsplit_oracle(c.name, ctx, c)
    ctx.close()


MODES = ["scratch + gather", "PFM_HANGING_ATOMIC"]


def _set_mode(mode, monkeypatch):
    """How the cells at hanging vertices reach the outputs (read by pfm_ctx_create).  Default: the SCR instantiations write
    scratch, k_hanging_gather adds it, the plain classes run without the ring.  PFM_HANGING_ATOMIC=1: the ATOMIC
    instantiations add with FP64 atomics and the plain classes are the RING instantiations next to them."""
    if mode.startswith("PFM_"):
        monkeypatch.setenv(mode, "1")


@pytest.mark.parametrize("mode", MODES)
def test_without_compression_it_is_the_unsplit_oracle_on_hanging_nodes_with_per_cell_lame(mode, monkeypatch):
    """hetero_3d: the plain classes and the cells at hanging vertices, K' = C^T K C, in both modes of the latter"""
    _set_mode(mode, monkeypatch)
    c = SC.tension_hetero_case()
    SC.assert_one_sided(c, +1)
    ctx = _context(c)
    check_unsplit_oracle(f"{c.name} [{mode}]", ctx, c)
    ctx.close()


# ---------------------------------------------------------------- 4
@pytest.mark.parametrize("blocked", [True, False])
def test_compression_everywhere(blocked):
    """tr E < 0 at every q-point: sigma- carries the whole volumetric stress and C- the bulk modulus; d = (1, 1)"""
    c = SC.compression_case(blocked)
    SC.assert_one_sided(c, -1)
    ctx = _context(c)
    check(c.name, ctx, c, _ref(SC.compression_case, blocked))
    ctx.close()


# ---------------------------------------------------------------- 5
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("blocked,solver", SC.HANGING)
def test_hanging_nodes_dirichlet_lines_active_set_and_per_cell_lame(blocked, solver, mode, monkeypatch):
    """hang3d_mesh: 120 cells, 72 hanging nodes.  The cells at hanging vertices take scratch + gather under this model, so
    two assemblies give the same bytes; with PFM_HANGING_ATOMIC=1 they add atomically (no bitwise promise) next to the RING
    instantiations of the plain classes."""
    _set_mode(mode, monkeypatch)
    c = SC.hanging_case(blocked, solver)
    share, margin = SC.assert_mixed(c)
    ref = _ref(SC.hanging_case, blocked, solver)
    ctx = _context(c)
    first = check(f"{c.name} [{mode}] (share {share:.2f}, margin {margin:.1e})", ctx, c, ref)
    constrained_rows_hold_their_placeholder(c, ref, ctx)
    if not mode.startswith("PFM_"):
        assert _bytes(_outputs(ctx, c)) == _bytes(first)
    ctx.close()


# ---------------------------------------------------------------- 6
def test_one_living_overlay_context_through_both_models():
    """unsplit -> model 3 -> unsplit -> model 1 -> model 3 on the refined (8, 8, 8) block (960 cells): the unsplit outputs
    are the same bytes each time (against the oracle once), kernel_path and overlay_info() stay, the two model-3 results
    have the same bytes."""
    from test_gpu_overlay3d import check_against_oracle

    c = SC.block_case()
    SC.assert_mixed(c)
    ref = _ref(SC.block_case)
    off = cases.Case("step0", c.mesh, c.layout, _copy(c.params, timestep_number=0), c.sol, c.old, c.oldold, c.cu, c.ch)
    ctx = _context(off, model=capi.SPLIT_VOLDEV)
    info = ctx.overlay_info()
    state = lambda: (ctx.kernel_path, ctx.overlay_info())
    assert state() == (3, info) and info[0] > 0 and 0 < info[1] < c.mesh.n_cells
    check_against_oracle(off, ctx)
    unsplit = _bytes(_outputs(ctx, off))
    ctx.set_params(c.params)  # model 3
    first = _bytes(check("living context, model 3", ctx, c, ref))
    assert state() == (3, info)
    ctx.set_params(off.params)
    assert _bytes(_outputs(ctx, off)) == unsplit and state() == (3, info)
    ctx.set_split_model(capi.SPLIT_SPECTRAL)  # model 1 on the same context
    ctx.set_params(c.params)
    check("living context, model 1", ctx, c, Ref(c, law=R))
    assert state() == (3, info)
    ctx.set_split_model(capi.SPLIT_VOLDEV)  # and back, without the unsplit step in between
    ctx.set_params(c.params)
    assert _bytes(check("living context, model 3 again", ctx, c, ref)) == first
    assert state() == (3, info)
    ctx.set_params(off.params)
    assert _bytes(_outputs(ctx, off)) == unsplit
    ctx.close()


# ---------------------------------------------------------------- 7
@pytest.mark.parametrize("blocked", [True, False])
def test_two_ranks_and_both_halves_of_the_overlapped_assembly(blocked):
    """A conforming (6, 5, 4) box in two ranks on one GPU, as tests/test_gpu_split3d_routes.py does for the spectral law"""
    import test_gpu_overlap_phases as OP

    n = (6, 5, 4)
    c = SC.two_rank_case(blocked)
    SC.assert_mixed(c)
    ref = _ref(SC.two_rank_case, blocked)
    refs = {False: OP.Reference(c.layout, ref.A, ref.res, None, c.sol), True: OP.Reference(c.layout, None, ref.res, ref.tot, c.sol, ref.A, ref.A_tot)}
    off = cases.Case("step0", c.mesh, c.layout, _copy(c.params, timestep_number=0), c.sol, c.old, c.oldold, c.cu, c.ch)
    ranks = OP.box_ranks(off, n, (2, 1, 1))
    for r in ranks:
        r.ctx.set_split_model(capi.SPLIT_VOLDEV)
        r.ctx.set_params(c.params)
        assert r.lp.n_owned < r.lp.mesh.n_nodes  # ghosts on both
    OP.run_partition(ranks, refs, general=True)
    for r in ranks:
        r.ctx.close()


# ---------------------------------------------------------------- 8
@pytest.mark.parametrize("blocked,solver,norm,restore", SC.LINE_SEARCH)
def test_device_line_search_on_a_model_3_context(blocked, solver, norm, restore):
    """pfm_line_search_device: the composition of today's entries bit for bit, with rejected trials, twice; the residual it
    leaves against the reference at the vector it accepted"""
    import test_gpu_line_search as LS

    c = SC.line_search_case(blocked, solver)
    SC.assert_mixed(c)
    upd = L.newton_update(c, seed=5, u_amp=2e-4 * smallest_edge(c.mesh), phi_amp=0.5)
    ctx = _context(c)
    assert ctx.kernel_path == 0
    want, got = LS._run_both(ctx, c, upd, 0.0, 4, norm, restore)  # exhaustion: the norm of every trial
    assert got["steps"] == 4 and not got["accepted"]
    LS._compare(c, want, got, True)
    n0, n1, n2, _ = want["trials"]
    print("split_voldev line search: trial norms", want["trials"])
    assert n0 > n1 > n2
    runs = []
    for _ in range(2):  # a tie with trial 1, which the strict compare rejects: two rejected trials, the third accepted
        want, got = LS._run_both(ctx, c, upd, n1, 4, norm, restore)
        assert got["steps"] == 2 and got["accepted"]
        LS._compare(c, want, got, True)
        runs.append(got)
    for k in ("sol", "upd", "pde", "tot"):
        assert LS.same_bits(runs[0]["vec"][k][0], runs[1]["vec"][k][0]), k
    sol = runs[1]["vec"]["sol"][0]
    share, margin = SC.assert_mixed(c, sol)  # the accepted vector is still a mixed state with a margin
    _, Re, _ = V.element_matrices(c.mesh, c.layout, c.params, sol, c.old, c.oldold, jacobian=False)
    pde_ref = R.distribute_vector(c.layout, c.mesh.cells, Re, c.cu)
    tot_ref = R.residual_total(c.layout, c.mesh.cells, c.params, Re, c.cu, c.ch)
    e = (linf_scaled(runs[1]["vec"]["pde"][0], pde_ref), linf_scaled(runs[1]["vec"]["tot"][0], tot_ref))
    # (no reference matrix at the accepted vector: the residual parts at their own scale)
    for got_v, ref_v in ((runs[1]["vec"]["pde"][0], pde_ref), (runs[1]["vec"]["tot"][0], tot_ref)):
        PS.assert_parts(got_v, ref_v, PS.is_phi(c.layout), TOL, "split_voldev line search, accepted vector")
    print(f"split_voldev line search blocked={blocked} solver={solver}: residual at the accepted vector {e[0]:.2e} / {e[1]:.2e} "
          f"(share {share:.2f}, margin {margin:.1e})")
    assert max(e) < TOL
    ctx.close()


# ---------------------------------------------------------------- 9
@pytest.mark.parametrize("kind", ["zero", "shear"])
def test_zero_strain_and_zero_trace(kind):
    """A regular box with u = 0 and with u = (2^-7 y, 0, 0): tr E is exactly 0 at every q-point of the reference (asserted),
    h(0) = 1 makes the split the identity: the unsplit oracle, finite, the same bits twice.  (The box of the shear is
    (2, 2, 2): see split_voldev_cases.edge_case for what the device's trace is on a larger one.)"""
    c = SC.edge_case(kind)
    SC.assert_edge(c)
    ctx = _context(c)
    assert ctx.kernel_path == 1
    first = check_unsplit_oracle(c.name, ctx, c)
    assert _bytes(_outputs(ctx, c)) == _bytes(first)
    ctx.sync_status()
    ctx.close()
