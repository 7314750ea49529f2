"""The spectral stress split of 3-D assemblies on the routes that only a split assembly takes, in a state where the split
does something (strains with eigenvalues of both signs at every q-point; in pure tension it is the identity and
tests/test_gpu_split3d.py could compare with the unsplit oracle):

1. hanging nodes, Dirichlet lines and an active set on the general family: the ATOMIC and RING instantiations, the reduction
   K' = C^T K C of the 16-slot split form, the placeholder diagonals of constrained rows under the split tangent;
2. one living overlay context through the time loop: unsplit (overlay + gather), split (general family over all cells, the
   full colour lists built lazily), and back, bit for bit; a fresh context whose first assembly is a split one;
3. two ranks and both halves of the overlapped assembly;
4. the device line search on a split context.

Reference: tests/split3d_ref.py with its distribution over constraint lines, pinned to the oracle by
tests/test_split3d_ref_cpu.py.  State of every test: u = SHEAR x + noise of 2e-4 h (h: the smallest cell edge), the three phase
fields random in (0.3, 0.9), hanging nodes distributed; conditions on it asserted from the reference's strains alone.
Bar: gpu_util.TOL.  Measured deviations (MI355X): DESIGN.md §2."""
import functools

import numpy as np
import pytest

import cases
import line_search_cases as L
import split3d_ref as R
import topology_cases as T
from cracks_amd import capi
from cracks_amd import mesh as M
import parity_scale as PS
from gpu_util import TOL, linf_scaled, reference_parity
from test_gpu_split3d import LAM, MU, SHEAR, _box, _copy, _matrix, _params, _spectral_context

pytestmark = pytest.mark.gpu


# ---- state and reference ----------------------------------------------------------------------------------------------
def smallest_edge(mesh):
    X = mesh.coords[mesh.cells]
    return min(float(np.linalg.norm(X[:, v | (1 << d)] - X[:, v], axis=1).min()) for d in range(3) for v in range(8) if not v & (1 << d))


def free_interior_nodes(mesh):
    """nodes off the boundary that neither hang nor are parents"""
    ok = np.zeros(mesh.n_nodes, bool)
    ok[T._free_nodes(mesh)] = True
    for ids in mesh.boundary_nodes.values():
        ok[ids] = False
    return np.nonzero(ok)[0]


def mixed_case(name, mesh, blocked, prm, seed, lines, cell_lame=False):
    """The state recipe of this file; lines: the dofs of constraints_update next to the hanging nodes"""
    rng = np.random.default_rng(seed)
    lay = M.DofLayout(mesh.n_nodes, 3, blocked=blocked)
    h = smallest_edge(mesh)
    u = mesh.coords @ SHEAR.T + rng.uniform(-2e-4 * h, 2e-4 * h, (mesh.n_nodes, 3))
    ch = M.hanging_constraints(mesh, lay)
    cu = M.update_constraints(mesh, lay, np.asarray(sorted(int(d) for d in lines(lay, rng)), np.int64))
    sol = ch.distribute(lay.pack(u, rng.uniform(0.3, 0.9, mesh.n_nodes)))
    old = ch.distribute(lay.pack(0 * u, rng.uniform(0.3, 0.9, mesh.n_nodes)))
    oo = ch.distribute(lay.pack(0 * u, rng.uniform(0.3, 0.9, mesh.n_nodes)))
    cl = cm = None
    if cell_lame:
        f = rng.uniform(0.5, 2.0, mesh.n_cells)
        cl, cm = LAM * f, MU * f[::-1].copy()
    assert prm.decompose_stress_rhs == 1.0 and prm.decompose_stress_matrix == 1.0 and prm.timestep_number == 1
    return cases.Case(name, mesh, lay, prm, sol, old, oo, cu, ch, None, cl, cm)


def faces_and_active_set(n_active):
    """Dirichlet displacement lines on the faces and n_active phase-field lines (an active set) on free interior nodes"""
    def lines(mesh):
        def of(lay, rng):
            dd = [int(d) for d in M.sneddon_dirichlet_dofs(mesh, lay)]
            return dd + [int(lay.dof(n, 3)) for n in rng.choice(free_interior_nodes(mesh), n_active, replace=False)]
        return of
    return lines


class Ref:
    """the reference of one case: matrix on the oracle's pattern, residual (of both calls), residual_total, the margin"""

    def __init__(self, c, elements=None):
        Ke, Re, E = elements or R.element_matrices(c.mesh, c.layout, c.params, c.sol, c.old, c.oldold, c.cell_lambda, c.cell_mu)
        self.elements = (Ke, Re, E)
        self.margin, mixed = R.eigen_margin(E)
        # the condition on the inputs: the law is well conditioned and the split does something at every q-point
        assert mixed and self.margin >= 1e-2, (self.margin, mixed)
        self.A, self.res = R.distribute_matrix(c.mesh, c.layout, Ke, Re, c.cu)
        # residual_total: the oracle's rule (oracle.cpp assemble, cracks.cc:2439-2464) applied to the reference's element
        # residuals -- distributed with the hanging-node constraints alone under the active-set scheme (outer_solver 0: the
        # lines of constraints_update keep their entries), with constraints_update under every other scheme
        self.tot = R.residual_total(c.layout, c.mesh.cells, c.params, Re, c.cu, c.ch)
        # the matrix whose rows belong to residual_total (the scales of tests/parity_scale.py): under the active-set scheme the
        # same element matrices distributed with the hanging-node constraints alone
        self.A_tot = self.A if c.params.outer_solver != 0 else R.distribute_matrix(c.mesh, c.layout, Ke, Re, c.ch)[0]


def check_split(tag, ctx, c, ref):
    """full assembly (identical pattern) and the residual-only call against the reference; the four deviations"""
    values, res, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
    A = _matrix(ctx, c, values)
    assert A.nnz == ref.A.nnz and (A.indptr == ref.A.indptr).all() and (A.indices == ref.A.indices).all()
    _, pde, tot = ctx.assemble_host(c.sol, c.old, c.oldold, True)
    e = (linf_scaled(A.data, ref.A.data), linf_scaled(res, ref.res), linf_scaled(pde, ref.res), linf_scaled(tot, ref.tot))
    print(f"split3d routes {tag}: matrix {e[0]:.2e} residual {e[1]:.2e} residual-only {e[2]:.2e} / {e[3]:.2e} "
          f"(eigenvalue margin {ref.margin:.3f})")
    assert max(e) < TOL, e
    reference_parity(c.layout, c.sol, A, ref.A, [(res, ref.res, "pde"), (pde, ref.res, "pde"), (tot, ref.tot, "tot")], tag=f"split3d routes {tag}",
                     A_tot=ref.A_tot)
    return e


def constrained_rows_hold_their_placeholder(c, ref, ctx):
    """every line of constraints_update that is no hanging node: its row is its diagonal, a positive placeholder"""
    values, _, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
    A = _matrix(ctx, c, values)
    lines = np.nonzero(c.cu.flag.astype(bool) & ~c.ch.flag.astype(bool))[0]
    assert lines.size > 0
    d = A.diagonal()
    assert (d[lines] > 0.0).all() and linf_scaled(d[lines], ref.A.diagonal()[lines]) < TOL
    rows = A[lines].tocsr()
    assert (np.diff(rows.indptr) > 1).all() and np.count_nonzero(rows.data) == lines.size  # stored zeros next to it


# ---------------------------------------------------------------- 1
@pytest.mark.parametrize("blocked,solver,cell_lame", [(True, 0, False), (False, 1, False), (False, 0, True), (True, 1, True)],
                         ids=["blocked-active_set", "interleaved-monolithic", "interleaved-active_set-lame", "blocked-monolithic-lame"])
def test_hanging_nodes_dirichlet_lines_and_an_active_set(blocked, solver, cell_lame):
    """hang3d_mesh: 120 cells, 72 hanging nodes -- the cells at hanging vertices in the ATOMIC instantiation (no gather
    under the split), the others in RING classes next to them, KRED, placeholders from the split element matrix"""
    mesh = T.hang3d_mesh()
    prm = _params(outer_solver=solver, gamma_penal=1e-2 if solver == 1 else 0.0)
    c = mixed_case("hanging", mesh, blocked, prm, 40 + solver, faces_and_active_set(6)(mesh), cell_lame)
    assert mesh.hn_nodes.size == 72 and (c.cell_lambda is not None) == cell_lame
    touched = np.zeros(mesh.n_nodes, bool)
    touched[mesh.hn_nodes] = touched[mesh.hn_parents] = True
    node, _ = c.layout.node_comp_of_dof()
    lines = c.cu.flag.astype(bool) & ~c.ch.flag.astype(bool)
    assert lines.sum() > 6 and not touched[node[lines]].any()  # lines on nodes that neither hang nor are parents
    ref = Ref(c)
    ctx = _spectral_context(c)  # (kernel_path 3: an overlay context, but a split assembly runs without the overlay)
    check_split(f"hanging blocked={blocked} solver={solver} lame={cell_lame}", ctx, c, ref)
    constrained_rows_hold_their_placeholder(c, ref, ctx)
    ctx.close()


# ---------------------------------------------------------------- 2
@functools.lru_cache(maxsize=None)
def _block(n, blocked):
    """(case, reference) on the refined block of n coarse cells: mesh, Dirichlet lines and active set of the overlay tests
    (test_gpu_overlay3d.refined_block_case), the state of this file.  The element matrices are computed once per mesh."""
    from test_gpu_overlay3d import refined_block_case

    shape = refined_block_case(n, blocked)
    lines = lambda lay, rng: np.nonzero(shape.cu.flag.astype(bool) & ~shape.ch.flag.astype(bool))[0]
    c = mixed_case("refined_block", shape.mesh, blocked, _params(), 50, lines)
    assert np.array_equal(c.cu.flag, shape.cu.flag) and c.ch.flag.any()
    if blocked:
        return c, Ref(c)
    cb, rb = _block(n, True)  # the same nodal state in the other layout
    for x, y in ((c.sol, cb.sol), (c.old, cb.old), (c.oldold, cb.oldold)):
        assert all(np.array_equal(p, q) for p, q in zip(R.nodal(c.layout, x), R.nodal(cb.layout, y)))
    return c, Ref(c, rb.elements)


def _living(n, blocked):
    """a context that starts in step 0 of the time loop (timestep_number == 0: unsplit whatever else the parameters say)"""
    c, ref = _block(n, blocked)
    off = cases.Case("step0", c.mesh, c.layout, _copy(c.params, timestep_number=0), c.sol, c.old, c.oldold, c.cu, c.ch)
    return c, ref, off, _spectral_context(off)


def _outputs(ctx, c):
    values, res, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
    _, pde, tot = ctx.assemble_host(c.sol, c.old, c.oldold, True)
    return [v.tobytes() for v in values] + [res.tobytes(), pde.tobytes(), tot.tobytes()]


@pytest.mark.parametrize("blocked", [True, False])
def test_one_living_context_through_the_time_loop(blocked):
    """(a) step 0: overlay + gather, against the oracle; (b) split, against the reference; (c) step 0 again: the bytes of
    (a); (d) split again.  kernel_path and overlay_info() stay what they were; then a context that starts with the split."""
    from test_gpu_overlay3d import check_against_oracle

    n = (8, 8, 8)  # 960 cells: both level lattices keep more than the 64 regular rows an overlay level needs
    c, ref, off, ctx = _living(n, blocked)
    info = ctx.overlay_info()
    state = lambda: (ctx.kernel_path, ctx.overlay_info())
    assert state() == (3, info) and info[0] > 0 and 0 < info[1] < c.mesh.n_cells
    print(f"split3d routes living context: refined block {n}, {c.mesh.n_cells} cells, overlay rows / general cells {info}")
    check_against_oracle(off, ctx)  # (a) overlay + gather
    first = _outputs(ctx, off)
    ctx.set_params(c.params)  # (b) the split: the general family over all cells, full colour lists built now
    check_split(f"living context {n} blocked={blocked} (b)", ctx, c, ref)
    assert state() == (3, info)
    ctx.set_params(off.params)  # (c) back: every byte of (a)
    assert _outputs(ctx, off) == first
    assert state() == (3, info)
    ctx.set_params(c.params)  # (d) the colour lists are reused
    check_split(f"living context {n} blocked={blocked} (d)", ctx, c, ref)
    constrained_rows_hold_their_placeholder(c, ref, ctx)
    assert state() == (3, info)
    ctx.close()
    fresh = _spectral_context(c)  # its first assembly is a split one
    assert fresh.kernel_path == 3 and fresh.overlay_info() == info
    check_split(f"fresh context {n} blocked={blocked}", fresh, c, ref)
    assert fresh.kernel_path == 3 and fresh.overlay_info() == info
    fresh.close()


# ---------------------------------------------------------------- 3
@pytest.mark.parametrize("blocked", [True, False])
def test_two_ranks_and_both_halves_of_the_overlapped_assembly(blocked):
    """A conforming (6, 5, 4) box in two ranks on one GPU.  test_gpu_overlap_phases.run_partition: the whole assembly of
    each rank writes every owned entry and equals the single-rank reference on the owned rows (TOL); phase 1 leaves the
    sentinel-filled outputs untouched (the plan gives a split assembly nothing there); phase 2 after the import equals the
    whole assembly bit for bit, as does the whole assembly repeated (colour classes only: no atomics)."""
    import test_gpu_overlap_phases as OP

    n = (6, 5, 4)
    g = M.box_mesh(3, n)
    c = mixed_case("two_ranks", g, blocked, _params(), 60, faces_and_active_set(5)(g))
    ref = Ref(c)
    refs = {False: OP.Reference(c.layout, ref.A, ref.res, None, c.sol), True: OP.Reference(c.layout, None, ref.res, ref.tot, c.sol, ref.A, ref.A_tot)}
    # the ranks are built with the parameters of step 0 (the split is refused before the model is set), then switched
    off = cases.Case("step0", g, c.layout, _copy(c.params, timestep_number=0), c.sol, c.old, c.oldold, c.cu, c.ch)
    ranks = OP.box_ranks(off, n, (2, 1, 1))
    for r in ranks:
        r.ctx.set_split_model(capi.SPLIT_SPECTRAL)
        r.ctx.set_params(c.params)
        assert r.lp.n_owned < r.lp.mesh.n_nodes  # ghosts on both
    OP.run_partition(ranks, refs, general=True)
    for r in ranks:
        r.ctx.close()


# ---------------------------------------------------------------- 4
@pytest.mark.parametrize("blocked,solver,norm,restore", [(True, 0, "l2", "saved"), (False, 1, "linf", "subtract")])
def test_device_line_search_on_a_split_context(blocked, solver, norm, restore):
    """pfm_line_search_device on a context whose residual kernel is the split one (the scatter is not fused there): the
    composition of today's entries bit for bit (perturbed conforming box: colour classes only), with rejected trials,
    twice; the residual it leaves against the reference at the vector it accepted."""
    import test_gpu_line_search as LS

    mesh = _box((5, 4, 3), perturb=True, seed=3)
    prm = _params(outer_solver=solver, gamma_penal=1e-2 if solver == 1 else 0.0)
    c = mixed_case("line_search", mesh, blocked, prm, 70, faces_and_active_set(5)(mesh))
    Ref(c)  # the condition on the state the search starts from
    upd = L.newton_update(c, seed=5, u_amp=2e-4 * smallest_edge(mesh), phi_amp=0.5)
    ctx = _spectral_context(c)
    assert ctx.kernel_path == 0
    want, got = LS._run_both(ctx, c, upd, 0.0, 4, norm, restore)  # exhaustion: the norm of every trial
    assert got["steps"] == 4 and not got["accepted"]
    LS._compare(c, want, got, True)
    n0, n1, n2, _ = want["trials"]
    print("split3d routes line search: trial norms", want["trials"])
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
    Ke, Re, E = R.element_matrices(mesh, c.layout, c.params, sol, c.old, c.oldold, jacobian=False)
    margin, mixed = R.eigen_margin(E)
    assert mixed and margin >= 1e-2, (margin, mixed)  # the accepted vector is still a well-conditioned mixed state
    pde_ref = R.distribute_vector(c.layout, mesh.cells, Re, c.cu)
    tot_ref = R.residual_total(c.layout, mesh.cells, c.params, Re, c.cu, c.ch)
    e = (linf_scaled(runs[1]["vec"]["pde"][0], pde_ref), linf_scaled(runs[1]["vec"]["tot"][0], tot_ref))
    # (no reference matrix at the accepted vector: the residual parts at their own scale)
    for got_v, ref_v in ((runs[1]["vec"]["pde"][0], pde_ref), (runs[1]["vec"]["tot"][0], tot_ref)):
        PS.assert_parts(got_v, ref_v, PS.is_phi(c.layout), TOL, "split3d routes line search, accepted vector")
    print(f"split3d routes line search blocked={blocked} solver={solver}: residual at the accepted vector {e[0]:.2e} / {e[1]:.2e} "
          f"(eigenvalue margin {margin:.3f})")
    assert max(e) < TOL
    ctx.close()
