"""The spectral stress split of 3-D assemblies (pfm_set_split_model, PFM_SPLIT_SPECTRAL; cracks_amd/csrc/pfm_split3.h and
the 3-D SPLIT instantiations of k_assemble_general):

1. refusal under the default model and opt-in;
2. entry by entry against the numpy reference (tests/split3d_ref.py) on the general family and on a box context that
   takes the lazy route to it, and back;
3. a state in pure tension reproduces the unsplit oracle through every scatter path;
4. an extruded 2-D mesh reproduces the 2-D oracle with its closed-form split on;
5. exactly diagonal, isotropic and zero strain.

Bar: |x - x_ref|_inf < 1e-12 max(1, |x_ref|_inf) (gpu_util.TOL).  Measured deviations (MI355X): see DESIGN.md §2.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import cases
import oracle_api as O
import split3d_ref as R
from cracks_amd import capi
from cracks_amd import mesh as M
from cracks_amd import partition as P
from cracks_amd.assembler import Context, node_flags_from_dof_flags
import parity_scale as PS
from gpu_util import TOL, blocks_to_global, exchange_ghosts, linf_scaled, make_context, oracle, reference_parity, total_matrix

pytestmark = pytest.mark.gpu

LAM, MU = 121.15, 80.77
SHEAR = 1e-2 * np.array([[0.9, 0.7, -0.3], [0.1, -0.8, 0.5], [0.4, -0.2, 0.2]])  # sym part: eigenvalues of both signs


def _params(d_rhs=1.0, d_mat=1.0, **kw):
    d = dict(mu=MU, G_c=2.7, alpha_eps=0.5, constant_k=1e-3, pressure=0.05, timestep=1e-3, time=2e-3, old_timestep=1e-3,
             old_old_timestep=1e-3, timestep_number=1, decompose_stress_rhs=d_rhs, decompose_stress_matrix=d_mat)
    d.update(kw)
    return O.make_params(**{"lambda": LAM}, **d)


def _copy(prm, **kw):
    q = O.PfmParams.from_buffer_copy(bytes(prm))
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _box(shape, perturb, seed=0):
    """unit cells; perturb: interior nodes moved by up to 0.12 and no box hint (general family)"""
    mesh = M.box_mesh(3, shape, lo=0.0, hi=np.asarray(shape, float))
    if perturb:
        rng = np.random.default_rng(seed)
        inner = np.ones(mesh.n_nodes, bool)
        for ids in mesh.boundary_nodes.values():
            inner[ids] = False
        mesh.coords[inner] += rng.uniform(-0.12, 0.12, (int(inner.sum()), 3))
        mesh.box_shape = None
    return mesh


def _case(mesh, blocked, prm, grad, noise, seed, cell_lame=False, dirichlet=()):
    """u = grad x + noise, phi / phi_old / phi_oldold random in (0.3, 0.9); no constraints unless asked for"""
    rng = np.random.default_rng(seed)
    lay = M.DofLayout(mesh.n_nodes, 3, blocked=blocked)
    u = mesh.coords @ np.asarray(grad).T + rng.uniform(-noise, noise, (mesh.n_nodes, 3))
    ch = M.hanging_constraints(mesh, lay)
    cu = M.update_constraints(mesh, lay, dirichlet)
    sol = ch.distribute(lay.pack(u, rng.uniform(0.3, 0.9, mesh.n_nodes)))
    old = ch.distribute(lay.pack(0 * u, rng.uniform(0.3, 0.9, mesh.n_nodes)))
    oo = ch.distribute(lay.pack(0 * u, rng.uniform(0.3, 0.9, mesh.n_nodes)))
    cl = cm = None
    if cell_lame:
        f = rng.uniform(0.5, 2.0, mesh.n_cells)
        cl, cm = LAM * f, MU * f[::-1].copy()
    return cases.Case("split3d", mesh, lay, prm, sol, old, oo, cu, ch, None, cl, cm)


def _spectral_context(c, **kw):
    ctx = Context(c.mesh, c.layout.blocked, cell_lambda=c.cell_lambda, cell_mu=c.cell_mu, **kw)
    ctx.set_split_model(capi.SPLIT_SPECTRAL)
    ctx.set_params(c.params)
    ctx.set_constraints(node_flags_from_dof_flags(c.layout, c.cu.flag, c.ch.flag))
    return ctx


def _matrix(ctx, c, values):
    A = blocks_to_global(ctx, c.layout, values)
    A.sort_indices()
    return A


def _mat_err(A, A_ref):
    return float(abs(A - A_ref).max()) / max(1.0, float(abs(A_ref).max()))


# ---------------------------------------------------------------- 1
def test_refusal_under_the_default_model_and_opt_in():
    c = cases.perturbed(cases.kat_sneddon_3d(4))
    split = _copy(c.params, decompose_stress_rhs=1.0, decompose_stress_matrix=1.0, timestep_number=1)
    ctx = make_context(c)
    with pytest.raises(capi.PfmError) as e:
        ctx.set_params(split)  # model 0: as before
    assert e.value.status == 5
    with pytest.raises(capi.PfmError) as e:
        ctx.set_split_model(2)
    assert e.value.status == 1 and ctx.split_model == 0
    with pytest.raises(capi.PfmError) as e:
        ctx.set_split_model(-1)
    assert e.value.status == 1
    ctx.set_split_model(capi.SPLIT_SPECTRAL)
    ctx.set_params(split)
    assert ctx.kernel_path == 1  # a box context: the general family takes the split assembly
    values, res, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
    assert np.isfinite(res).all() and all(np.isfinite(v).all() for v in values) and np.abs(values[0]).max() > 0
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
        ctx2.set_split_model(capi.SPLIT_SPECTRAL)
    assert e.value.status == 5
    ctx2.set_split_model(capi.SPLIT_REFERENCE)
    ctx2.close()


# ---------------------------------------------------------------- 2
@pytest.mark.parametrize("kind,blocked,d,cell_lame", [("general", True, (1.0, 1.0), False), ("general", False, (0.0, 1.0), False),
                                                      ("general", False, (1.0, 1.0), False), ("general", True, (0.0, 1.0), True),
                                                      ("box", True, (0.0, 1.0), False), ("box", False, (1.0, 1.0), False),
                                                      ("box", False, (0.0, 1.0), False), ("box", True, (1.0, 1.0), False)])
def test_entry_by_entry_against_the_numpy_reference(kind, blocked, d, cell_lame):
    """(5, 4, 3) hexes: the colour class of the even cells has 12 of them -- two workgroups of the 32-lane Jacobian form."""
    mesh = _box((5, 4, 3), perturb=kind == "general", seed=3)
    c = _case(mesh, blocked, _params(*d, outer_solver=1, gamma_penal=1e-2), SHEAR, 2e-4, seed=21, cell_lame=cell_lame)
    A_ref, r_ref, E = R.assemble(c.mesh, c.layout, c.params, c.sol, c.old, c.oldold, c.cell_lambda, c.cell_mu)
    margin, mixed = R.eigen_margin(E)
    assert mixed and margin >= 1e-2, (margin, mixed)  # a condition on the inputs: the split is well conditioned
    ctx = _spectral_context(c)
    assert ctx.kernel_path == (0 if kind == "general" else 1)
    values, res, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
    e_A, e_R = _mat_err(_matrix(ctx, c, values), A_ref), linf_scaled(res, r_ref)
    _, res_ro, tot_ro = ctx.assemble_host(c.sol, c.old, c.oldold, True)
    e_ro, e_tot = linf_scaled(res_ro, r_ref), linf_scaled(tot_ro, r_ref)  # (no constraints: both residuals are the plain sum)
    print(f"split3d {kind} blocked={blocked} d={d}: matrix {e_A:.2e} residual {e_R:.2e} residual-only {e_ro:.2e} / {e_tot:.2e} "
          f"(eigenvalue margin {margin:.3f})")
    assert e_A < TOL and e_R < TOL and e_ro < TOL and e_tot < TOL
    # at the scale of each entry, block, row and part (no constraints: residual_total's rows are the matrix's too)
    A_on = reference_parity(c.layout, c.sol, _matrix(ctx, c, values), A_ref, [(res, r_ref, "pde"), (res_ro, r_ref, "pde"), (tot_ro, r_ref, "tot")],
                            tag=f"split3d {kind} blocked={blocked} d={d}")
    # the line-search entry on the same context
    import torch
    d_sol = torch.from_numpy(c.sol).cuda()
    d_r, d_t = torch.empty_like(d_sol), torch.empty_like(d_sol)
    ctx.assemble_nl_residual_device(d_sol.data_ptr(), d_r.data_ptr(), d_t.data_ptr())
    ctx.sync_status()
    assert linf_scaled(d_r.cpu().numpy(), r_ref) < TOL
    reference_parity(c.layout, c.sol, None, A_on, [(d_r.cpu().numpy(), r_ref, "pde")], tag="split3d line-search entry")
    if kind == "box":
        # split off again: the context returns to its own kernels, bit for bit what a fresh context computes
        off = _copy(c.params, timestep_number=0)
        ctx.set_params(off)
        v1, r1, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
        c0 = cases.Case("fresh", c.mesh, c.layout, off, c.sol, c.old, c.oldold, c.cu, c.ch, None, c.cell_lambda, c.cell_mu)
        fresh = make_context(c0)
        v0, r0, _ = fresh.assemble_host(c.sol, c.old, c.oldold, False)
        assert r1.tobytes() == r0.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(v1, v0))
        fresh.close()
    ctx.close()


# ---------------------------------------------------------------- 3
def _assert_pure_tension(c):
    _, _, E = R.assemble(c.mesh, c.layout, c.params, c.sol, c.old, c.oldold, jacobian=False, split=False)
    l = np.linalg.eigvalsh(E)
    assert l.min() > 0.0 and np.trace(E, axis1=-2, axis2=-1).min() > 0.0


def _tension_parity(c, **ctx_kw):
    """the split model on, against the oracle with the split off: matrix, residual, both residuals of the residual-only call"""
    _assert_pure_tension(c)
    off = cases.Case(c.name, c.mesh, c.layout, _copy(c.params, decompose_stress_matrix=0.0, decompose_stress_rhs=0.0), c.sol, c.old, c.oldold,
                     c.cu, c.ch, None, c.cell_lambda, c.cell_mu)
    r, rowptr, colind = oracle(off, False)
    ctx = _spectral_context(c, **ctx_kw)
    values, res, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
    A = _matrix(ctx, c, values)
    A_ref = sp.csr_matrix((r.values, colind, rowptr), shape=A.shape)
    assert A.nnz == A_ref.nnz and (A.indices == A_ref.indices).all()
    e_A, e_R = linf_scaled(A.data, A_ref.data), linf_scaled(res, r.residual_pde)
    r2, _, _ = oracle(off, True)
    _, res2, tot2 = ctx.assemble_host(c.sol, c.old, c.oldold, True)
    e_2, e_t = linf_scaled(res2, r2.residual_pde), linf_scaled(tot2, r2.residual_total)
    print(f"split3d tension {c.name}: matrix {e_A:.2e} residual {e_R:.2e} residual-only {e_2:.2e} / {e_t:.2e}")
    assert e_A < TOL and e_R < TOL and e_2 < TOL and e_t < TOL
    reference_parity(c.layout, c.sol, A, A_ref, [(res, r.residual_pde, "pde"), (res2, r2.residual_pde, "pde"), (tot2, r2.residual_total, "tot")],
                     tag=f"split3d tension {c.name}", A_tot=total_matrix(off, A_ref))
    ctx.close()


EXPAND = 1e-2 * np.eye(3)


@pytest.mark.parametrize("solver", [0, 1], ids=["active_set", "monolithic"])
def test_pure_tension_with_dirichlet_and_active_set_flags(solver):
    mesh = _box((5, 4, 3), perturb=True, seed=5)
    lay = M.DofLayout(mesh.n_nodes, 3, blocked=True)
    rng = np.random.default_rng(9)
    dd = list(M.sneddon_dirichlet_dofs(mesh, lay))  # u on the faces
    inner = np.setdiff1d(np.arange(mesh.n_nodes), np.concatenate(list(mesh.boundary_nodes.values())))
    dd += [int(lay.dof(n, 3)) for n in rng.choice(inner, 5, replace=False)]  # phase-field lines of an active set
    c = _case(mesh, True, _params(outer_solver=solver, gamma_penal=1e-2), EXPAND, 2e-4, seed=22, dirichlet=np.asarray(sorted(dd), np.int64))
    c.name = f"constraints/{solver}"
    _tension_parity(c)


def test_pure_tension_on_a_mesh_with_hanging_nodes_and_per_cell_lame():
    """tests/cases.py: the hetero_3d mesh (318 hanging nodes, per-cell Lame coefficients): the atomic class, K' = C^T K C"""
    k = cases.kat_hetero_3d()
    rng = np.random.default_rng(4)
    u = k.mesh.coords @ EXPAND.T + rng.uniform(-1e-4, 1e-4, (k.mesh.n_nodes, 3))
    phi = rng.uniform(0.3, 0.9, k.mesh.n_nodes)
    sol = k.ch.distribute(k.layout.pack(u, phi))
    dmask = k.cu.flag.astype(bool) & ~k.ch.flag.astype(bool)
    prm = _copy(k.params, decompose_stress_rhs=1.0, decompose_stress_matrix=1.0, timestep_number=1)
    c = cases.Case("hanging", k.mesh, k.layout, prm, sol, k.old, k.oldold, k.cu, k.ch, None, k.cell_lambda, k.cell_mu)
    assert dmask.any() and k.mesh.hn_nodes.size > 0 and c.cell_lambda is not None
    _tension_parity(c)


def test_pure_tension_on_two_ranks():
    """a two-rank partition as two contexts on one GPU: the owned rows of each against the single-rank unsplit oracle"""
    import torch

    n = (6, 5, 4)
    g = M.box_mesh(3, n, lo=0.0, hi=np.asarray(n, float))
    glay = M.DofLayout(g.n_nodes, 3, blocked=True)
    cg = _case(g, True, _params(), EXPAND, 2e-4, seed=23)
    _assert_pure_tension(cg)
    off = cases.Case("g", g, glay, _copy(cg.params, decompose_stress_matrix=0.0, decompose_stress_rhs=0.0), cg.sol, cg.old, cg.oldold, cg.cu, cg.ch)
    r, rowptr, colind = oracle(off, False)
    A_ref = sp.csr_matrix((r.values, colind, rowptr), shape=(glay.n_dofs,) * 2)
    ug, pg = R.nodal(glay, cg.sol)
    _, pog = R.nodal(glay, cg.old)
    _, poog = R.nodal(glay, cg.oldold)
    lps = [P.build_local_problem(3, n, P.factor_ranks(2, 3), rk, lo=0.0, hi=np.asarray(n, float)) for rk in range(2)]
    ctxs, keep = [], []
    for lp in lps:
        gi, no = lp.global_ids, lp.n_owned
        ctx = Context(lp.mesh, True, n_owned_nodes=no)
        ctx.set_split_model(capi.SPLIT_SPECTRAL)
        ctx.set_params(cg.params)
        ctx.set_constraints(np.zeros(lp.mesh.n_nodes, np.uint8))
        pack = lambda uu, pp: np.concatenate([uu[gi[:no]].reshape(-1), pp[gi[:no]]])
        vecs = [torch.from_numpy(v).cuda() for v in (pack(ug, pg), pack(0 * ug, pog), pack(0 * ug, poog))]
        ctx.state_set_device(*[v.data_ptr() for v in vecs])
        ctx.halo_register(lp.send_ptr, lp.send_nodes, lp.recv_ptr, lp.recv_nodes)
        ctxs.append(ctx)
        keep.append(vecs)
    recv = exchange_ghosts(lps, ctxs, 3)
    for ctx, buf in zip(ctxs, recv):
        if buf.numel():
            ctx.halo_unpack_all(buf.data_ptr())
    torch.cuda.synchronize()
    for lp, ctx in zip(lps, ctxs):
        gi, no = lp.global_ids, lp.n_owned
        vals = [torch.zeros(ctx.pattern_size(b)[1], dtype=torch.float64, device="cuda") for b in range(4)]
        res, tot = torch.zeros(4 * no, dtype=torch.float64, device="cuda"), torch.zeros(4 * no, dtype=torch.float64, device="cuda")
        ctx.assemble_device(False, [v.data_ptr() for v in vals], res.data_ptr(), tot.data_ptr())
        ctx.sync_status()
        gdof = np.concatenate([(gi[:no, None] * 3 + np.arange(3)[None, :]).ravel(), 3 * g.n_nodes + gi[:no]])
        assert linf_scaled(res.cpu().numpy(), r.residual_pde[gdof]) < TOL
        # the owned rows of this rank at the scales of the global reference: s_i of the global rows, d = diag(A_ref)
        PS.assert_rank_rows(res.cpu().numpy(), r.residual_pde[gdof], A_ref, glay, cg.sol, gdof, TOL, "split3d two ranks, owned rows")
        scale = max(1.0, np.abs(r.values).max())
        for b in range(4):
            rp, ci = ctx.pattern(b)
            v = vals[b].cpu().numpy()
            ncr, ncc = (3 if b in (0, 1) else 1), (3 if b in (0, 2) else 1)
            rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
            grow = gi[rows // ncr] * ncr + rows % ncr + (0 if b in (0, 1) else 3 * g.n_nodes)
            gcol = gi[ci // ncc] * ncc + ci % ncc + (0 if b in (0, 2) else 3 * g.n_nodes)
            want = np.asarray(A_ref[grow, gcol]).ravel()
            assert np.abs(v - want).max() < TOL * scale
            PS.assert_rank_block(v, want, A_ref.diagonal(), grow, gcol, PS.BLOCKS[b], TOL, "split3d two ranks")
        ctx.close()


# ---------------------------------------------------------------- 4
def test_extrusion_reproduces_the_2d_oracle_with_its_split_on():
    """A perturbed 4 x 4 quad mesh extruded by one layer of thickness h_z, u_z = 0 and u_x, u_y, phi constant in z: the 3-D
    residual summed over the two z-copies of a node, and the 3-D matrix over the z-copies of row and column node, are h_z
    times the 2-D oracle's (components x, y, phi).  gamma_penal = 0: the penalty scales with the cell diameter."""
    hz = 0.37
    m2 = M.box_mesh(2, (4, 4), lo=0.0, hi=4.0)
    rng = np.random.default_rng(31)
    inner = np.setdiff1d(np.arange(m2.n_nodes), np.concatenate(list(m2.boundary_nodes.values())))
    m2.coords[inner] += rng.uniform(-0.12, 0.12, (inner.size, 2))
    m2.box_shape = None
    n2 = m2.n_nodes
    coords3 = np.concatenate([np.c_[m2.coords, np.zeros(n2)], np.c_[m2.coords, np.full(n2, hz)]])
    cells3 = np.concatenate([m2.cells, m2.cells + n2], axis=1).astype(np.int32)
    m3 = M.Mesh(dim=3, coords=coords3, cells=cells3)
    for blocked in (True, False):
        l2, l3 = M.DofLayout(n2, 2, blocked=blocked), M.DofLayout(2 * n2, 3, blocked=blocked)
        u2 = m2.coords @ SHEAR[:2, :2].T + rng.uniform(-2e-4, 2e-4, (n2, 2))
        phis = [rng.uniform(0.3, 0.9, n2) for _ in range(3)]
        prm = _params(1.0, 1.0)
        s2 = [l2.pack(u2 if k == 0 else 0 * u2, phis[k]) for k in range(3)]
        u3 = np.c_[np.tile(u2, (2, 1)), np.zeros(2 * n2)]
        s3 = [l3.pack(u3 if k == 0 else 0 * u3, np.tile(phis[k], 2)) for k in range(3)]
        cu2, ch2 = M.update_constraints(m2, l2, []), M.hanging_constraints(m2, l2)
        c2 = cases.Case("quad", m2, l2, prm, s2[0], s2[1], s2[2], cu2, ch2)
        r, rowptr, colind = oracle(c2, False)
        A2 = sp.csr_matrix((r.values, colind, rowptr), shape=(l2.n_dofs,) * 2)
        c3 = cases.Case("extruded", m3, l3, prm, s3[0], s3[1], s3[2], M.update_constraints(m3, l3, []), M.hanging_constraints(m3, l3))
        _, _, E = R.assemble(m3, l3, prm, *s3, jacobian=False)
        assert (np.abs(E[..., 0, 1]) >= 1e-2 * np.linalg.norm(E, axis=(-2, -1))).all()  # away from the 2-D 'close to diagonal' branch
        ctx = _spectral_context(c3)
        values, res, _ = ctx.assemble_host(*s3, False)
        A3 = _matrix(ctx, c3, values)
        # S: 2-D dof (n, c) <- the 3-D dofs (n, comp(c)) and (n + n2, comp(c)), comp = x, y, phi
        rows, cols = [], []
        for c_2, c_3 in ((0, 0), (1, 1), (2, 3)):
            for z in (0, 1):
                rows.append(l2.dof(np.arange(n2), c_2))
                cols.append(l3.dof(np.arange(n2) + z * n2, c_3))
        S = sp.csr_matrix((np.ones(6 * n2), (np.concatenate(rows), np.concatenate(cols))), shape=(l2.n_dofs, l3.n_dofs))
        e_R = linf_scaled(S @ res, hz * r.residual_pde)
        e_A = _mat_err((S @ A3 @ S.T).tocsr(), hz * A2)
        print(f"split3d extrusion blocked={blocked}: matrix {e_A:.2e} residual {e_R:.2e}")
        assert e_R < TOL and e_A < TOL
        _, res_ro, _ = ctx.assemble_host(*s3, True)
        assert linf_scaled(S @ res_ro, hz * r.residual_pde) < TOL
        # the collapsed 3-D matrix against h_z times the 2-D oracle's, at the scales of the latter
        reference_parity(l2, s2[0], (S @ A3 @ S.T).tocsr(), hz * A2, [(S @ res, hz * r.residual_pde, "pde"), (S @ res_ro, hz * r.residual_pde, "pde")],
                         tag=f"split3d extrusion blocked={blocked}")
        ctx.close()


# ---------------------------------------------------------------- 5
def test_exactly_diagonal_isotropic_and_zero_strain():
    """Disconnected unit cubes with power-of-two displacement gradients (the device of test_gpu_split_corners.py): E exactly
    diag(a, a, b), a I and 0, with every combination of signs.  Finite, the numpy reference, and the same bits twice.
    (A zero eigenvalue NEXT TO non-zero ones is left out: the reference's strain carries off-diagonal noise of 1e-20 from its
    inverse Jacobian there, which decides the sign of that eigenvalue, i.e. h, at random.  With u = 0 the strain is exactly
    zero in both arithmetics.)"""
    a, b = 2.0 ** -9, 2.0 ** -11
    grads = [np.diag(g) for g in ((a, a, -b), (-a, -a, b), (a, a, b), (-a, -a, -b), (a, -b, a), (b, a, a), (a, a, a), (-a, -a, -a), (0.0, 0.0, 0.0))]
    K = len(grads)
    corner = np.array([[v & 1, (v >> 1) & 1, v >> 2] for v in range(8)], float)
    mesh = M.Mesh(dim=3, coords=np.tile(corner, (K, 1)), cells=np.arange(8 * K, dtype=np.int32).reshape(K, 8))
    lay = M.DofLayout(mesh.n_nodes, 3, blocked=False)
    u = np.concatenate([corner @ g.T for g in grads])
    rng = np.random.default_rng(3)
    sol = lay.pack(u, rng.uniform(0.3, 0.9, mesh.n_nodes))
    old = lay.pack(0 * u, rng.uniform(0.3, 0.9, mesh.n_nodes))
    c = cases.Case("corners3", mesh, lay, _params(), sol, old, old.copy(), M.update_constraints(mesh, lay, []), M.hanging_constraints(mesh, lay))
    A_ref, r_ref, _ = R.assemble(mesh, lay, c.params, c.sol, c.old, c.oldold)
    ctx = _spectral_context(c)
    values, res, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
    assert np.isfinite(res).all() and np.isfinite(values[0]).all()
    e_A, e_R = _mat_err(_matrix(ctx, c, values), A_ref), linf_scaled(res, r_ref)
    _, res_ro, tot_ro = ctx.assemble_host(c.sol, c.old, c.oldold, True)
    print(f"split3d special cases: matrix {e_A:.2e} residual {e_R:.2e} residual-only {linf_scaled(res_ro, r_ref):.2e}")
    assert e_A < TOL and e_R < TOL and linf_scaled(res_ro, r_ref) < TOL and np.isfinite(tot_ro).all()
    reference_parity(c.layout, c.sol, _matrix(ctx, c, values), A_ref, [(res, r_ref, "pde"), (res_ro, r_ref, "pde")], tag="split3d special cases")
    values2, res2, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
    assert res2.tobytes() == res.tobytes() and values2[0].tobytes() == values[0].tobytes()
    ctx.sync_status()
    ctx.close()
