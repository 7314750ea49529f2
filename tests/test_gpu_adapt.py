"""Mesh adaptation on the device (include/pfm_newton.h, pfm_adapt.hip) against the numpy statement of cracks_amd/adapt.py:
refinement flags and their count (exact), the minimum cell diameter (equal), the state transfer (bitwise), and the
reference's predictor-corrector run of tests/miehe_shear_1.output with every sweep through the C ABI."""
import numpy as np
import pytest

import adapt_cases as AC
import cases
import newton_cases as NC
from cracks_amd import adapt as A
from cracks_amd import mesh as M
from cracks_amd import partition as P
from cracks_amd.assembler import Context
from cracks_amd.capi import PfmError
from cracks_amd.newton import ActiveSetDriver, GpuAssembler
from gpu_util import make_context
from test_gpu_overlay3d import refined_block_case
from test_gpu_postproc import _exchange

pytestmark = pytest.mark.gpu


def nodal_phi(mesh, layout, sol):
    return sol[layout.dof(np.arange(mesh.n_nodes), mesh.dim)]


def check_flags(ctx, mesh, phi, **crit):
    flags, n = ctx.refine_flags(**crit)
    want, n_want = A.refine_flags_numpy(mesh, phi, **crit)
    assert flags.dtype == np.uint8 and flags.shape == (mesh.n_cells,)
    assert np.array_equal(flags, want) and n == n_want
    return n


# ---- flags -----------------------------------------------------------------------------------------------------------

def test_flags_on_the_slit_mesh_with_a_converged_state():
    setup = NC.miehe_shear_1_setup()
    asm = GpuAssembler(setup.mesh, setup.layout)
    drv = ActiveSetDriver(setup, asm)
    drv.run(n_steps=3)
    mesh, lay = setup.mesh, setup.layout
    asm.ctx.state_set_host(drv.solution, drv.old_solution, drv.old_old_solution)
    phi = nodal_phi(mesh, lay, drv.solution)
    assert 0.8 < phi.min() < np.median(phi) < 1.0  # the crack has not started: a smooth dip at the slit tip
    counts = [check_flags(asm.ctx, mesh, phi, phi_threshold=t) for t in (0.8, float(np.median(phi)), 1.5)]
    assert counts[0] == 0 and counts[-1] == mesh.n_cells and 0 < counts[1] < mesh.n_cells
    level = (np.arange(mesh.n_cells) % 2).astype(np.uint8)
    check_flags(asm.ctx, mesh, phi, phi_threshold=float(np.median(phi)), max_level=1, cell_level=level)


@pytest.mark.parametrize("blocked", [True, False])
def test_flags_on_a_3d_box_as_one_and_as_eight_contexts(blocked):
    n, p = (24, 24, 24), P.factor_ranks(8, 3)
    g = M.box_mesh(3, n, lo=-1.5, hi=1.5)
    rng = np.random.default_rng(11)
    gphi = rng.uniform(0.0, 1.0, g.n_nodes)
    gu = rng.standard_normal((g.n_nodes, 3))
    glay = M.DofLayout(g.n_nodes, 3, blocked)
    gsol = glay.pack(gu, gphi)
    ref = Context(g, blocked)
    ref.state_set_host(gsol, gsol, gsol)
    thr = 0.02  # about 15 % of the cells have such a vertex
    total = check_flags(ref, g, gphi, phi_threshold=thr)
    assert 0 < total < g.n_cells
    own_mask = (np.arange(g.n_cells) % 3 != 1).astype(np.uint8)
    check_flags(ref, g, gphi, phi_threshold=thr, cell_owned=own_mask)
    first, n_first = ref.refine_flags(phi_threshold=thr)
    for _ in range(3):
        again, n_again = ref.refine_flags(phi_threshold=thr)
        assert again.tobytes() == first.tobytes() and n_again == n_first
    # eight ranks: owned nodes only, ghost values through the halo import; a cell belongs to the rank of its vertex 0
    lps = [P.build_local_problem(3, n, p, r, lo=-1.5, hi=1.5) for r in range(8)]
    ctxs, owned = [], []
    for r, lp in enumerate(lps):
        no = lp.n_owned
        olay = M.DofLayout(no, 3, blocked)
        sol_owned = olay.pack(gu[lp.global_ids[:no]], gphi[lp.global_ids[:no]])
        ctx = Context(lp.mesh, blocked, n_owned_nodes=no)
        ctx.state_set_host(sol_owned, sol_owned, sol_owned)
        ctx.halo_register(lp.send_ptr, lp.send_nodes, lp.recv_ptr, lp.recv_nodes)
        ctxs.append(ctx)
        owned.append((P.owner_of_nodes(n, p, lp.global_ids[lp.mesh.cells[:, 0]]) == r).astype(np.uint8))
    _exchange(ctxs, lps, 3)
    assert sum(int(m.sum()) for m in owned) == g.n_cells
    n_sum = 0
    for lp, ctx, mask in zip(lps, ctxs, owned):
        n_sum += check_flags(ctx, lp.mesh, gphi[lp.global_ids], phi_threshold=thr, cell_owned=mask)
    assert n_sum == total


@pytest.mark.parametrize("blocked", [True, False])
def test_flags_on_the_refined_block_through_the_overlay_and_the_general_family(blocked):
    c = refined_block_case((12, 12, 12), blocked)
    ctx = make_context(c)
    assert ctx.kernel_path == 3
    ctx.state_set_host(c.sol, c.old, c.oldold)
    phi = nodal_phi(c.mesh, c.layout, c.sol)
    level = np.zeros(c.mesh.n_cells, np.uint8)
    level[np.abs(c.mesh.cell_diameters() - c.mesh.min_cell_diameter()) < 1e-12] = 1
    assert 0 < level.sum() < c.mesh.n_cells
    for path in (3, 0):
        if path == 0:
            ctx.force_path(0)
            ctx.state_set_host(c.sol, c.old, c.oldold)
        n_all = check_flags(ctx, c.mesh, phi, phi_threshold=0.9)
        n_lim = check_flags(ctx, c.mesh, phi, phi_threshold=0.9, max_level=1, cell_level=level)
        assert 0 < n_lim < n_all < c.mesh.n_cells


@pytest.mark.parametrize("dim", [2, 3])
def test_flag_edge_cases(dim):
    m = M.box_mesh(dim, 4, 0.0, 4.0)
    lay = M.DofLayout(m.n_nodes, dim, blocked=True)
    phi = np.ones(m.n_nodes)
    phi[0] = 0.5
    phi[m.n_nodes // 2] = 0.8   # equal to the threshold: not flagged
    phi[m.n_nodes - 1] = np.nan  # never flags
    sol = lay.pack(np.zeros((m.n_nodes, dim)), phi)
    ctx = Context(m, True)
    ctx.state_set_host(sol, sol, sol)
    assert check_flags(ctx, m, phi, phi_threshold=0.8) == 1
    assert check_flags(ctx, m, phi, phi_threshold=float("nan")) == 0  # criterion off
    lo, hi = [-np.inf] * dim, [np.inf] * dim
    lo[1] = 3.5  # the "y >= 1.75" kind of rule: one closed side, the others open
    assert check_flags(ctx, m, phi, box_lo=lo, box_hi=hi) == 4 ** (dim - 1)
    assert check_flags(ctx, m, phi, phi_threshold=0.8, box_lo=lo, box_hi=hi) == 4 ** (dim - 1) + 1
    lo2, hi2 = [1.0] * dim, [1.0] * dim  # a single lattice point, closed box: the 2^dim cells around it
    assert check_flags(ctx, m, phi, box_lo=lo2, box_hi=hi2) == 2 ** dim
    level = np.zeros(m.n_cells, np.uint8)
    level[0] = 2
    assert check_flags(ctx, m, phi, phi_threshold=0.8, max_level=2, cell_level=level) == 0
    assert check_flags(ctx, m, phi, phi_threshold=0.8, max_level=1, cell_level=level) == 1
    assert check_flags(ctx, m, phi, phi_threshold=2.0, cell_owned=np.zeros(m.n_cells, np.uint8)) == 0  # empty mask
    with pytest.raises(PfmError) as e:
        ctx.refine_flags(phi_threshold=0.8, max_level=1)  # a level limit without levels
    assert e.value.status == 1


# ---- minimum diameter ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["box2d", "box3d", "slit", "threepoint", "refined_block"])
def test_min_cell_diameter(name):
    mesh = {"box2d": lambda: M.box_mesh(2, (12, 8), lo=-1.5, hi=1.5),
            "box3d": lambda: M.box_mesh(3, (6, 5, 4), lo=(-1.5, 0.0, 1.0), hi=(1.5, 0.7, 2.3)),
            "slit": lambda: M.slit_mesh(3),
            "threepoint": lambda: cases.kat_threepoint().mesh,
            "refined_block": lambda: refined_block_case((12, 12, 12), True).mesh}[name]()
    ctx = Context(mesh, True)
    assert ctx.min_cell_diameter() == A.min_cell_diameter_numpy(mesh) == mesh.min_cell_diameter()
    rng = np.random.default_rng(3)
    for k in range(4):
        mask = (rng.random(mesh.n_cells) < (0.5 if k < 3 else 2.0 / mesh.n_cells)).astype(np.uint8)
        assert ctx.min_cell_diameter(mask) == A.min_cell_diameter_numpy(mesh, mask)
    d = mesh.cell_diameters()
    only_largest = (d == d.max()).astype(np.uint8)
    assert ctx.min_cell_diameter(only_largest) == d.max()
    assert ctx.min_cell_diameter(np.zeros(mesh.n_cells, np.uint8)) == np.inf


# ---- transfer --------------------------------------------------------------------------------------------------------

def device_transfer(src_ctx, dst_ctx, parent, child, vectors, n_dst):
    import torch

    src = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in vectors]
    dst = [torch.full((n_dst,), float("nan"), dtype=torch.float64, device="cuda") for _ in vectors]
    torch.cuda.synchronize()
    try:
        src_ctx.transfer_state(dst_ctx, parent, child, [t.data_ptr() for t in src], [t.data_ptr() for t in dst])
    finally:
        torch.cuda.synchronize()
        out = [t.cpu().numpy() for t in dst]
    return out


def random_vectors(mesh, layout, rng, n=3):
    ch = M.hanging_constraints(mesh, layout)
    return [ch.distribute(rng.standard_normal(layout.n_dofs)) for _ in range(n)]


def transfer_meshes(dim):
    """base, a mesh with hanging nodes, the mesh with one more set of cells refined, the whole box refined"""
    base = M.box_mesh(dim, 6 if dim == 3 else 10, 0.0, 1.0)
    rng = np.random.default_rng(17 + dim)
    m1 = rng.random(base.n_cells) < 0.25
    m2 = m1 | (rng.random(base.n_cells) < 0.25)
    assert m1.any() and (m2 & ~m1).any()
    return base, m1, m2, np.ones(base.n_cells, bool)


@pytest.mark.parametrize("blocked", [True, False])
@pytest.mark.parametrize("dim", [2, 3])
def test_transfer_is_bitwise_numpy(dim, blocked):
    base, m1, m2, full = transfer_meshes(dim)
    rng = np.random.default_rng(23)
    t1 = A.two_level_mesh(base, m1)
    assert t1.mesh.hn_nodes.size > 0
    for old_mask, new_mask in ((m1, m1), (m1, m2), (None, m1), (None, full), (m2, full)):
        ts = t1 if old_mask is m1 else A.two_level_mesh(base, np.zeros(base.n_cells, bool) if old_mask is None else old_mask)
        td = A.two_level_mesh(base, new_mask, old_mask)
        lay_s, lay_d = M.DofLayout(ts.mesh.n_nodes, dim, blocked), M.DofLayout(td.mesh.n_nodes, dim, blocked)
        vecs = random_vectors(ts.mesh, lay_s, rng)
        vecs[2][::5] = -0.0
        want = A.transfer_numpy(ts.mesh, td.mesh, blocked, td.parent_cell, td.child, vecs)
        src_ctx, dst_ctx = Context(ts.mesh, blocked), Context(td.mesh, blocked)
        got = device_transfer(src_ctx, dst_ctx, td.parent_cell, td.child, vecs, lay_d.n_dofs)
        for g, w in zip(got, want):
            assert not np.isnan(g).any()
            assert g.tobytes() == w.tobytes()
        if old_mask is new_mask:  # the same mesh: a copy
            for g, v in zip(got, vecs):
                assert g.tobytes() == v.tobytes()
        again = device_transfer(src_ctx, dst_ctx, td.parent_cell, td.child, vecs, lay_d.n_dofs)
        for g, a in zip(got, again):
            assert g.tobytes() == a.tobytes()
        # the transferred vectors are distributed at the new mesh's hanging nodes
        ch = M.hanging_constraints(td.mesh, lay_d)
        assert np.abs(ch.distribute(got[0]) - got[0]).max() < 1e-14
        src_ctx.close()
        dst_ctx.close()


@pytest.mark.parametrize("dim", [2, 3])
def test_transfer_refuses_a_broken_relation(dim):
    base, m1, m2, _ = transfer_meshes(dim)
    ts, td = A.two_level_mesh(base, m1), A.two_level_mesh(base, m2, m1)
    blocked = dim == 3
    lay_s, lay_d = M.DofLayout(ts.mesh.n_nodes, dim, blocked), M.DofLayout(td.mesh.n_nodes, dim, blocked)
    vecs = random_vectors(ts.mesh, lay_s, np.random.default_rng(1), n=2)
    src_ctx, dst_ctx = Context(ts.mesh, blocked), Context(td.mesh, blocked)
    kid = int(np.nonzero(td.child != 255)[0][0])
    broken = []
    p = td.parent_cell.copy()
    p[-1] = (p[-1] + 1) % ts.mesh.n_cells  # wrong parent
    broken.append((p, td.child))
    c = td.child.copy()
    c[kid] ^= 1  # wrong child number
    broken.append((td.parent_cell, c))
    c = td.child.copy()
    c[kid] = 1 << dim  # not a child number
    broken.append((td.parent_cell, c))
    for bad_index in (-1, ts.mesh.n_cells, 2 ** 31 - 1):  # index out of range
        p = td.parent_cell.copy()
        p[0] = bad_index
        broken.append((p, td.child))
    for p, c in broken:
        assert not A.relation_matches(ts.mesh, td.mesh, p, c)
        with pytest.raises(PfmError) as e:
            device_transfer(src_ctx, dst_ctx, p, c, vecs, lay_d.n_dofs)
        assert e.value.status == 1
    # d_dst still holds its NaN fill
    import torch

    src = [torch.from_numpy(v).cuda() for v in vecs]
    dst = [torch.full((lay_d.n_dofs,), float("nan"), dtype=torch.float64, device="cuda") for _ in vecs]
    torch.cuda.synchronize()
    with pytest.raises(PfmError):
        src_ctx.transfer_state(dst_ctx, broken[0][0], broken[0][1], [t.data_ptr() for t in src], [t.data_ptr() for t in dst])
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in dst)
    # and the intact relation still goes through afterwards
    got = device_transfer(src_ctx, dst_ctx, td.parent_cell, td.child, vecs, lay_d.n_dofs)
    want = A.transfer_numpy(ts.mesh, td.mesh, blocked, td.parent_cell, td.child, vecs)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


def test_transfer_refuses_partitioned_and_mismatched_contexts():
    n, p = (8, 7, 6), P.factor_ranks(4, 3)
    lp = P.build_local_problem(3, n, p, 0, lo=-1.5, hi=1.5)
    assert lp.n_owned < lp.mesh.n_nodes
    part = Context(lp.mesh, True, n_owned_nodes=lp.n_owned)
    whole = Context(lp.mesh, True)
    other_layout = Context(lp.mesh, False)
    flat = Context(M.box_mesh(2, 4), True)
    nc = lp.mesh.n_cells
    ident = (np.arange(nc, dtype=np.int32), np.full(nc, 255, np.uint8))
    vecs = [np.zeros(lp.mesh.n_nodes * 4)]
    for a, b in ((part, whole), (whole, part), (whole, other_layout)):
        with pytest.raises(PfmError) as e:
            device_transfer(a, b, ident[0], ident[1], vecs, lp.mesh.n_nodes * 4)
        assert e.value.status == 5  # PFM_ERR_UNSUPPORTED
    with pytest.raises(PfmError) as e:
        device_transfer(flat, whole, ident[0], ident[1], vecs, lp.mesh.n_nodes * 4)
    assert e.value.status == 5
    got = device_transfer(whole, whole, ident[0], ident[1], vecs, lp.mesh.n_nodes * 4)  # a context onto itself: a copy
    assert got[0].tobytes() == vecs[0].tobytes()


# ---- end to end ------------------------------------------------------------------------------------------------------

def test_miehe_shear_1_adaptive_on_gpu():
    """The reference's predictor-corrector run: a GpuAssembler (context) per mesh, flags and transfer through the C ABI."""
    drv = AC.adaptive_miehe_shear_1(GpuAssembler, A.DeviceAdaptor())
    AC.check_adaptive_miehe_shear_1(drv.run())
