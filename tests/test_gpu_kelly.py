"""RefinementStrategy::mix on the device (include/pfm_newton.h, pfm_adapt.hip) against the numpy statement of
cracks_amd/adapt.py: the Kelly indicator at the project's parity bar |x - x_ref|_inf < 1e-12 max(1, |x_ref|_inf) on every
kernel path, both layouts, with masks and on partitions; the selection and the counts exactly; the flags, count and threshold
of pfm_refine_flags_mix equal (on inputs where, checked first, rounding cannot decide a flag); the refusals; and one
refine_mesh() of the harness through both adaptors."""
import numpy as np
import pytest

import adapt_cases as AC
import cases
from cracks_amd import adapt as A
from cracks_amd import mesh as M
from cracks_amd import partition as P
from cracks_amd.assembler import Context
from cracks_amd.capi import PfmError
from cracks_amd.newton import GpuAssembler
from gpu_util import linf_scaled, make_context
from test_gpu_overlay3d import refined_block_case
from test_gpu_postproc import _exchange

pytestmark = pytest.mark.gpu

BAR = 1e-12
BAD_ARG, UNSUPPORTED = 1, 5


def random_state(mesh, layout, seed):
    """a dof vector with N(0,1) values, distributed at the hanging nodes; phi in (0, 1)"""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((mesh.n_nodes, mesh.dim))
    phi = rng.uniform(0.0, 1.0, mesh.n_nodes)
    return M.hanging_constraints(mesh, layout).distribute(layout.pack(u, phi))


def device_eta(ctx, n_cells, component_mask=None, cell_owned=None):
    import torch

    eta = torch.full((max(n_cells, 1),), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.kelly_indicator(eta.data_ptr(), component_mask, cell_owned)
    ctx.sync_status()
    return eta[:n_cells].cpu().numpy()


def check_kelly(ctx, mesh, layout, sol, component_mask=None, cell_owned=None, neighbours=None):
    got = device_eta(ctx, mesh.n_cells, component_mask, cell_owned)
    want = A.kelly_numpy(mesh, A.nodal_values(mesh, layout, sol), component_mask, cell_owned, neighbours)
    err = linf_scaled(got, want)
    print(f"kelly: {mesh.n_cells} cells, mask {component_mask}, max eta {want.max():.6e}, scaled error {err:.3e}")
    assert not np.isnan(got).any() and want.max() > 0.0  # (the comparison is not one of zeros)
    assert err < BAR
    again = device_eta(ctx, mesh.n_cells, component_mask, cell_owned)
    assert again.tobytes() == got.tobytes()
    return got


def half_refined(dim, n=4):
    base = M.box_mesh(dim, n, 0.0, float(n))
    cx = base.coords[base.cells].mean(axis=1)[:, 0]
    return M.refine_cells(base, cx < 0.5 * n)


MESHES = {
    "box2d": lambda: M.box_mesh(2, (12, 8), lo=-1.5, hi=1.5),
    "box3d": lambda: M.box_mesh(3, (6, 5, 4), lo=(-1.5, 0.0, 1.0), hi=(1.5, 0.7, 2.3)),
    "refined_block": lambda: refined_block_case((12, 12, 12), True).mesh,
    "slit": lambda: M.slit_mesh(3),
    "threepoint": lambda: cases.kat_threepoint().mesh,
    "sneddon2d_amr": M.sneddon_2d_prerefined_mesh,
}


# ---- the indicator ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("blocked", [True, False], ids=["blocked", "interleaved"])
@pytest.mark.parametrize("name", list(MESHES))
def test_kelly_against_numpy(name, blocked):
    mesh = MESHES[name]()
    dim = mesh.dim
    lay = M.DofLayout(mesh.n_nodes, dim, blocked)
    sol = random_state(mesh, lay, 7)
    fn = A.face_neighbours_numpy(mesh)
    if name in ("refined_block", "sneddon2d_amr"):
        assert (fn.rel == A.REL_COARSE).any() and (fn.rel == A.REL_FINE).any()
    ctx = Context(mesh, blocked)
    if name == "refined_block":
        assert ctx.kernel_path == 3
    bytes_before = ctx.device_bytes
    ctx.state_set_host(sol, sol, sol)
    rng = np.random.default_rng(3)
    own = (rng.random(mesh.n_cells) < 0.6).astype(np.uint8)
    for path in (None, 0):
        if path == 0:
            ctx.force_path(0)  # the general family
            ctx.state_set_host(sol, sol, sol)
        eta = check_kelly(ctx, mesh, lay, sol, neighbours=fn)
        masked = check_kelly(ctx, mesh, lay, sol, cell_owned=own, neighbours=fn)
        assert masked.tobytes() == np.where(own != 0, eta, 0.0).tobytes()
        check_kelly(ctx, mesh, lay, sol, component_mask=(1 << (dim + 1)) - 1, neighbours=fn)  # with phi
        check_kelly(ctx, mesh, lay, sol, component_mask=1 << dim, neighbours=fn)               # phi alone
        check_kelly(ctx, mesh, lay, sol, component_mask=0b10, cell_owned=own, neighbours=fn)
    # the table is cached in the context and counted
    nf = 2 * dim
    assert ctx.device_bytes - bytes_before >= 5 * nf * mesh.n_cells
    ctx.close()


@pytest.mark.parametrize("dim", [2, 3])
def test_kelly_closed_forms_on_the_device(dim):
    """the kink on a refinement interface and a linear field across hanging faces (tests/test_kelly_numpy.py)"""
    m = half_refined(dim)
    lay = M.DofLayout(m.n_nodes, dim, True)
    ctx = Context(m, True)
    u = np.zeros((m.n_nodes, dim))
    u[:, 0] = np.abs(m.coords[:, 0] - 2.0)
    sol = lay.pack(u, np.ones(m.n_nodes))
    ctx.state_set_host(sol, sol, sol)
    eta = device_eta(ctx, m.n_cells)
    d = m.cell_diameters()
    coarse = d > 1.5 * d.min()
    cx = m.coords[m.cells].mean(axis=1)[:, 0]
    at_c, at_f = coarse & (np.abs(cx - 2.0) < 0.6), ~coarse & (np.abs(cx - 2.0) < 0.3)
    value = lambda h: np.sqrt(np.sqrt(dim) * h ** dim / 6.0)
    assert np.abs(eta[at_c] - value(1.0)).max() < BAR and np.abs(eta[at_f] - value(0.5)).max() < BAR
    assert np.abs(eta[~(at_c | at_f)]).max() < BAR
    a = np.random.default_rng(0).normal(size=(dim, dim))
    sol = lay.pack(m.coords @ a + 1.0, np.ones(m.n_nodes))
    ctx.state_set_host(sol, sol, sol)
    assert device_eta(ctx, m.n_cells).max() < BAR


@pytest.mark.parametrize("which,world", [("sneddon2d_amr", 4), ("half3d", 3), ("half2d", 2)])
def test_kelly_on_partitions(which, world):
    g = {"sneddon2d_amr": M.sneddon_2d_prerefined_mesh, "half3d": lambda: half_refined(3, 6),
         "half2d": lambda: half_refined(2, 8)}[which]()
    dim, nf = g.dim, 2 * g.dim
    assert g.hn_nodes.size > 0
    blocked = dim == 3
    glay = M.DofLayout(g.n_nodes, dim, blocked)
    gsol = random_state(g, glay, 13)
    gnodal = A.nodal_values(g, glay, gsol)
    ref = Context(g, blocked)
    ref.state_set_host(gsol, gsol, gsol)
    want = check_kelly(ref, g, glay, gsol)
    lps = P.partition_general(g, world, ghost_layer="dealii")
    # the caller's contract, which the reference's ghost layer meets: every face neighbour of an owned cell is local
    fn = A.face_neighbours_numpy(g)
    for lp in lps:
        local = np.zeros(g.n_cells, bool)
        local[lp.global_cells] = True
        owned = lp.global_cells[lp.cell_owned != 0]
        for f in range(nf):
            rel, nbr = fn.rel[owned, f], fn.nbr[owned, f]
            direct = (rel == A.REL_SAME) | (rel == A.REL_FINE)
            assert local[nbr[direct]].all()
            fine = fn.sub[nbr[rel == A.REL_COARSE]]
            assert (fine >= 0).all() and local[fine // nf].all()
    ctxs = []
    for lp in lps:
        no = lp.n_owned
        olay = M.DofLayout(no, dim, blocked)
        sol = olay.pack(gnodal[lp.global_ids[:no], :dim], gnodal[lp.global_ids[:no], dim])
        ctx = Context(lp.mesh, blocked, n_owned_nodes=no)
        ctx.state_set_host(sol, sol, sol)
        ctx.halo_register(lp.send_ptr, lp.send_nodes, lp.recv_ptr, lp.recv_nodes)
        ctxs.append(ctx)
    _exchange(ctxs, lps, dim)
    seen = np.zeros(g.n_cells, int)
    for lp, ctx in zip(lps, ctxs):
        got = device_eta(ctx, lp.mesh.n_cells, cell_owned=lp.cell_owned)
        own = lp.cell_owned != 0
        seen[lp.global_cells[own]] += 1
        err = linf_scaled(got[own], want[lp.global_cells[own]])
        print(f"rank with {own.sum()} owned of {lp.mesh.n_cells} cells: scaled error {err:.3e}")
        assert err < BAR and (got[~own] == 0.0).all()
        # ... and the local numpy statement says the same about the local mesh
        loc = A.kelly_numpy(lp.mesh, gnodal[lp.global_ids], cell_owned=lp.cell_owned)
        assert linf_scaled(got, loc) < BAR
    assert (seen == 1).all()


# ---- selection -------------------------------------------------------------------------------------------------------

def tied_values(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n)
    x[::7] = x[3]      # exact ties
    x[1::11] = 0.0
    x[2::13] = -0.0
    x[5::17] = np.nan
    x[6 % n] = np.inf
    x[8 % n] = -np.inf
    return x


def check_select(ctx, x, ks, mask=None):
    import torch

    d = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    for k in ks:
        t, above, equal = ctx.indicator_select(d.data_ptr(), k, mask)
        wt, wa, we = A.indicator_select_numpy(x, k, mask)
        assert np.float64(t).tobytes() == np.float64(wt).tobytes() or (np.isnan(t) and np.isnan(wt)), (k, t, wt)
        assert (above, equal) == (wa, we), (k, above, equal, wa, we)
        assert ctx.indicator_count(d.data_ptr(), t, mask) == (wa, we)
    for t in (0.0, -0.0, 0.5, float("inf"), float("-inf"), float("nan"), float(x[3])):
        assert ctx.indicator_count(d.data_ptr(), t, mask) == A.indicator_count_numpy(x, t, mask), t


@pytest.mark.parametrize("dim", [2, 3])
def test_select_and_count_are_exact(dim):
    m = M.box_mesh(dim, 40 if dim == 2 else 12)
    ctx = Context(m, True)
    n = m.n_cells
    x = tied_values(n, 5)
    n_num = int((~np.isnan(x)).sum())
    check_select(ctx, x, (1, 2, 10, n // 7, n // 7 + 1, n // 2, n_num - 1, n_num, n_num + 1, n))
    mask = (np.arange(n) % 3 != 1).astype(np.uint8)
    n_mask = int(mask.sum())
    check_select(ctx, x, (1, 5, n_mask // 2, n_mask), mask)
    check_select(ctx, np.zeros(n), (1, n))
    check_select(ctx, np.full(n, np.nan), (1, n))
    check_select(ctx, -np.abs(x), (1, 3, n))
    import torch

    d = torch.from_numpy(x).cuda()
    for bad_k, bad_mask in ((0, None), (-1, None), (n + 1, None), (n_mask + 1, mask)):
        with pytest.raises(PfmError) as e:
            ctx.indicator_select(d.data_ptr(), bad_k, bad_mask)
        assert e.value.status == BAD_ARG
    with pytest.raises(PfmError) as e:
        ctx.indicator_select(0, 1)
    assert e.value.status == BAD_ARG
    check_select(ctx, x, (3,))  # and the context still selects


def test_select_among_ten_million():
    m = M.box_mesh(3, 216)
    n = m.n_cells
    assert n >= 10 ** 7
    ctx = Context(m, True)
    x = tied_values(n, 9)
    n_num = int((~np.isnan(x)).sum())
    check_select(ctx, x, (1, int(0.3 * n), n_num, n))
    mask = (np.arange(n) % 5 != 0).astype(np.uint8)
    check_select(ctx, x, (int(0.3 * mask.sum()),), mask)


# ---- mix -------------------------------------------------------------------------------------------------------------

def assert_rounding_cannot_decide(eta, k):
    s = np.sort(eta)[::-1]
    assert k < s.size and (s[k - 1] - s[k]) > 1e-9 * s[0], (s[k - 1], s[k], s[0])


def check_mix(ctx, mesh, layout, sol, top_fraction, **crit):
    nodal = A.nodal_values(mesh, layout, sol)
    want, n_want, t_want = A.refine_flags_mix_numpy(mesh, nodal, top_fraction, **crit)
    flags, n, t = ctx.refine_flags_mix(top_fraction, **crit)
    print(f"mix: {mesh.n_cells} cells, fraction {top_fraction}: flagged {n}/{n_want}, threshold {t!r}/{t_want!r}")
    assert flags.dtype == np.uint8 and np.array_equal(flags, want) and n == n_want
    return flags, n, t, t_want


@pytest.mark.parametrize("blocked", [True, False], ids=["blocked", "interleaved"])
@pytest.mark.parametrize("dim", [2, 3])
def test_mix_on_a_half_refined_box(dim, blocked):
    m = half_refined(dim)
    lay = M.DofLayout(m.n_nodes, dim, blocked)
    rng = np.random.default_rng(1)
    u = rng.normal(size=(m.n_nodes, dim))
    sol = M.hanging_constraints(m, lay).distribute(lay.pack(u, np.ones(m.n_nodes)))
    nodal = A.nodal_values(m, lay, sol)
    eta = A.kelly_numpy(m, nodal)
    k = int(0.3 * m.n_cells)
    assert_rounding_cannot_decide(eta, k)
    ctx = Context(m, blocked)
    ctx.state_set_host(sol, sol, sol)
    flags, n, t, t_want = check_mix(ctx, m, lay, sol, 0.3)
    assert n == k and abs(t - t_want) <= BAR * max(1.0, abs(t_want))
    # the threshold is the k-th largest of the device's own indicator, exactly
    got = device_eta(ctx, m.n_cells)
    assert t == np.sort(got)[::-1][k - 1]
    # with a phase-field criterion and the level limit: phi < 0.5 around the most indicated cell
    phi = np.ones(m.n_nodes)
    phi[m.cells[np.argmax(eta)]] = 0.1
    sol2 = M.hanging_constraints(m, lay).distribute(lay.pack(u, phi))
    nodal2 = A.nodal_values(m, lay, sol2)
    by_phi = A.refine_flags_numpy(m, nodal2[:, dim], 0.5)[0].astype(bool)
    assert by_phi.any()
    assert_rounding_cannot_decide(np.where(by_phi, 0.0, A.kelly_numpy(m, nodal2)), k)
    ctx.state_set_host(sol2, sol2, sol2)
    level = (m.cell_diameters() < 1.5 * m.cell_diameters().min()).astype(np.uint8)
    f1, n1, _, _ = check_mix(ctx, m, lay, sol2, 0.3, phi_threshold=0.5)
    f2, n2, _, _ = check_mix(ctx, m, lay, sol2, 0.3, phi_threshold=0.5, max_level=1, cell_level=level)
    assert (f1[by_phi] == 1).all() and np.array_equal(f2, f1 * (level != 1)) and 0 < n2 < n1
    own = (np.arange(m.n_cells) % 4 != 0).astype(np.uint8)
    assert_rounding_cannot_decide(np.where(by_phi | (own == 0), 0.0, A.kelly_numpy(m, nodal2)), k)
    f3, _, _, _ = check_mix(ctx, m, lay, sol2, 0.3, phi_threshold=0.5, cell_owned=own)
    assert (f3[own == 0] == 0).all()
    # k = 0: nothing beyond phi
    f4, n4, t4, _ = check_mix(ctx, m, lay, sol2, 0.5 / m.n_cells, phi_threshold=0.5)
    assert np.array_equal(f4.astype(bool), by_phi) and t4 == np.inf
    # all indicators zero: nothing flags, whatever the fraction
    still = lay.pack(np.zeros((m.n_nodes, dim)), np.ones(m.n_nodes))
    ctx.state_set_host(still, still, still)
    for frac in (0.3, 1.0):
        _, n5, t5, _ = check_mix(ctx, m, lay, still, frac)
        assert n5 == 0 and t5 == np.inf
    # top_fraction = 1 with zeros among the indicators (cells that are not owned): the zero threshold becomes the smallest
    # positive indicator
    ctx.state_set_host(sol, sol, sol)
    f6, n6, t6, _ = check_mix(ctx, m, lay, sol, 1.0, cell_owned=own)
    assert n6 == int(own.sum()) and t6 == got[own != 0].min() and (f6 == own).all()
    f7, n7, _, _ = check_mix(ctx, m, lay, sol, 1.0)
    assert n7 == m.n_cells
    # refusals leave the context in working order
    for kw in (dict(top_fraction=-0.1), dict(top_fraction=1.5), dict(top_fraction=float("nan")), dict(component_mask=0),
               dict(component_mask=1 << (dim + 1)), dict(max_level=1)):
        with pytest.raises(PfmError) as e:
            ctx.refine_flags_mix(**kw)
        assert e.value.status == BAD_ARG
    import torch

    buf = torch.zeros(m.n_cells, dtype=torch.float64, device="cuda")
    for bad in (0, 1 << (dim + 1), 0xffffffff):
        with pytest.raises(PfmError) as e:
            ctx.kelly_indicator(buf.data_ptr(), bad)
        assert e.value.status == BAD_ARG
    with pytest.raises(PfmError) as e:
        ctx.kelly_indicator(0)
    assert e.value.status == BAD_ARG
    with pytest.raises(PfmError) as e:
        ctx.indicator_select(buf.data_ptr(), m.n_cells + 1)
    assert e.value.status == BAD_ARG
    check_mix(ctx, m, lay, sol, 0.3)
    c = cases.perturbed(cases.kat_sneddon_3d(4) if dim == 3 else cases.kat_miehe_shear_1())
    actx = make_context(c)
    buf = torch.zeros(c.mesh.n_cells, dtype=torch.float64, device="cuda")
    with pytest.raises(PfmError):
        actx.kelly_indicator(buf.data_ptr(), 0)
    with pytest.raises(PfmError):
        actx.indicator_select(buf.data_ptr(), 0)
    values, res, _ = actx.assemble_host(c.sol, c.old, c.oldold, residual_only=False)
    fresh = make_context(c)
    values2, res2, _ = fresh.assemble_host(c.sol, c.old, c.oldold, residual_only=False)
    assert linf_scaled(res, res2) < BAR and all(linf_scaled(a, b) < BAR for a, b in zip(values, values2))


def test_mix_refuses_a_partitioned_context():
    g = half_refined(2, 8)
    lp = P.partition_general(g, 2, ghost_layer="dealii")[0]
    assert lp.n_owned < lp.mesh.n_nodes
    ctx = Context(lp.mesh, True, n_owned_nodes=lp.n_owned)
    sol = np.zeros(lp.n_owned * 3)
    ctx.state_set_host(sol, sol, sol)
    import ctypes as C

    from cracks_amd import capi

    crit = ctx._criteria(float("nan"), None, None, -1)
    flags = np.full(lp.mesh.n_cells, 7, np.uint8)
    n, t = C.c_int64(-3), C.c_double(-2.0)
    rc = ctx.lib.pfm_refine_flags_mix(ctx._h, C.byref(crit), 0.3, 3, None, None, capi.np_ptr(flags, np.uint8), C.byref(n), C.byref(t))
    assert rc == UNSUPPORTED and (flags == 7).all() and n.value == -3 and t.value == -2.0
    with pytest.raises(PfmError) as e:
        ctx.refine_flags_mix(0.3)
    assert e.value.status == UNSUPPORTED


# ---- the converged state of the adaptive Miehe run, and the harness ------------------------------------------------------

def converged_miehe(n_steps):
    drv = AC.adaptive_miehe_shear_1(GpuAssembler, A.DeviceAdaptor())
    drv.run(n_steps=n_steps)
    return drv


def test_mix_on_the_converged_adaptive_miehe_state():
    drv = converged_miehe(7)  # past the first mesh change: the state lives on a mesh with hanging nodes
    d = drv.drv
    mesh, lay = d.s.mesh, d.s.layout
    assert mesh.hn_nodes.size > 0
    nodal = A.nodal_values(mesh, lay, d.solution)
    level = drv.tl.cell_level
    by_phi = A.refine_flags_numpy(mesh, nodal[:, 2], AC.PHI_THRESHOLD)[0].astype(bool)
    eta = np.where(by_phi, 0.0, A.kelly_numpy(mesh, nodal))
    ctx = drv.asm.ctx
    ctx.set_params(d._params())
    ctx.state_set_host(d.solution, d.old_solution, d.old_old_solution)
    check_kelly(ctx, mesh, lay, d.solution)
    for frac in (0.3, 0.1):
        assert_rounding_cannot_decide(eta, int(frac * mesh.n_cells))
        flags, n, t, t_want = check_mix(ctx, mesh, lay, d.solution, frac, phi_threshold=AC.PHI_THRESHOLD, max_level=1, cell_level=level)
        assert 0 < n < mesh.n_cells and abs(t - t_want) <= BAR * max(1.0, abs(t_want))


def test_refine_mesh_with_the_mix_strategy_through_both_adaptors():
    dev = converged_miehe(3)
    host = AC.adaptive_miehe_shear_1(GpuAssembler, A.NumpyAdaptor())
    d = dev.drv
    for name in ("solution", "old_solution", "old_old_solution"):
        setattr(host.drv, name, getattr(d, name).copy())
    for name in ("time", "timestep", "old_timestep", "old_old_timestep", "timestep_number", "use_old_timestep_pf"):
        setattr(host.drv, name, getattr(d, name))
    nodal = A.nodal_values(d.s.mesh, d.s.layout, d.solution)
    k = int(0.3 * d.s.mesh.n_cells)
    assert_rounding_cannot_decide(A.kelly_numpy(d.s.mesh, nodal), k)
    results = []
    for drv in (dev, host):
        drv.strategy, drv.top_fraction = "mix", 0.3
        changed, n = drv.refine_mesh()
        assert changed and n == k  # phi has not dropped below the threshold yet: the Kelly cells alone
        results.append((n, drv.mask.copy(), drv.tl.mesh, [drv.drv.solution, drv.drv.old_solution, drv.drv.old_old_solution]))
    (n_a, mask_a, mesh_a, vec_a), (n_b, mask_b, mesh_b, vec_b) = results
    assert n_a == n_b and np.array_equal(mask_a, mask_b) and mask_a.sum() == k
    assert np.array_equal(mesh_a.cells, mesh_b.cells) and mesh_a.coords.tobytes() == mesh_b.coords.tobytes()
    assert np.array_equal(mesh_a.hn_nodes, mesh_b.hn_nodes)
    for a, b in zip(vec_a, vec_b):
        assert a.tobytes() == b.tobytes()
    with pytest.raises(ValueError):
        A.AdaptiveDriver(M.slit_mesh(3), AC.miehe_shear_1_setup_of, GpuAssembler, A.NumpyAdaptor(), 0.8, strategy="kelly")
