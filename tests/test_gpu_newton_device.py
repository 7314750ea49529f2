"""The Newton-loop device sweeps of include/pfm_newton.h (pfm_diag_mass_device, pfm_active_set_device, pfm_residual_norms,
pfm_functionals[_material]) where tests/test_newton_sweeps.py does not reach: on partitions (owner computes, the blocked
offset n_owned * dim + P, ghost flag bytes, the refusal for hanging nodes), past one grid of k_residual_norms, at the edges
of the active-set criterion against newton.py's unfused numpy statement, on 3-D hanging nodes and the interleaved layout,
with per-cell Lame coefficients, in the device-resident step (active set on the device, then the next assembly), and with
bad arguments.  Every rank is a context on one device."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp

import bench
import cases
import oracle_api as O
from cracks_amd import capi
from cracks_amd import mesh as M
from cracks_amd import partition as P
from cracks_amd import statistics as S
from cracks_amd.assembler import Assembler, Context, node_flags_from_dof_flags
from cracks_amd.capi import PfmError
from gpu_util import blocks_to_global, linf_scaled
from test_gpu_overlay3d import refined_block_case
from test_gpu_postproc import _exchange
from test_newton_sweeps import criterion_edges, numpy_active_set

pytestmark = pytest.mark.gpu

BAD_ARG, UNSUPPORTED = 1, 5
GRID = 2048 * 256  # NORM_BLOCKS_MAX blocks of 256 threads: k_residual_norms strides above this many owned nodes


def dev(a, dtype=None):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    return t if dtype is None else t.to(dtype)


def padded(a):
    """a float64 device copy of ``a`` at the start of an allocation twice as long whose tail is NaN"""
    import torch

    a = np.ascontiguousarray(a, np.float64)
    t = torch.full((max(2 * a.size, 64),), float("nan"), dtype=torch.float64, device="cuda")
    t[:a.size] = torch.from_numpy(a).to("cuda")
    return t


def new_ctx(mesh, blocked, n_owned=None, prm=None, flags=None, **kw):
    import torch

    ctx = Context(mesh, blocked, n_owned_nodes=n_owned, **kw)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_params(prm if prm is not None else bench.sneddon_params(mesh.min_cell_diameter() if mesh.n_cells else 1.0, mesh.dim))
    ctx.set_constraints(np.zeros(mesh.n_nodes, np.uint8) if flags is None else flags)
    return ctx


def numpy_norms(z):
    z = np.asarray(z, np.float64)
    sq = math.fsum((z * z).tolist())
    return math.sqrt(sq), float(np.abs(z).max()) if z.size else 0.0, sq


def zero_flagged(lay, v, flags, hanging=None):
    """constraints_update.set_zero + the hanging lines, from node flag bytes (bit c: dof (node, c))"""
    z = v.copy()
    n = np.arange(lay.n_nodes)
    for c in range(lay.nc):
        z[lay.dof(n, c)[((flags >> c) & 1).astype(bool)]] = 0.0
        if hanging is not None:
            z[lay.dof(hanging, c)] = 0.0
    return z


# ---------------------------------------------------------------------------------------------------------- partitions
def node_state(g, seed=11):
    """Random per-node inputs of all four sweeps, a function of the global node id (what every rank restricts)."""
    rng = np.random.default_rng(seed)
    N, dim = g.n_nodes, g.dim
    mass = O.diag_mass(g, M.DofLayout(N, dim, True))[dim * N:]
    on_bnd = np.zeros(N, bool)
    for nodes in g.boundary_nodes.values():
        on_bnd[nodes] = True
    flags = np.where(on_bnd, (1 << dim) - 1, 0).astype(np.uint8)
    flags |= ((rng.random(N) < 0.3).astype(np.uint8) << dim).astype(np.uint8)
    return dict(mass=mass, flags=flags,
                res_u=rng.standard_normal((N, dim)), res_phi=rng.standard_normal(N) * mass,
                u=rng.uniform(-1e-3, 1e-3, (N, dim)), phi=rng.uniform(0.0, 1.0, N), phi_old=rng.uniform(0.0, 1.0, N),
                cyc=rng.integers(0, 7, N).astype(np.int32))


def run_sweeps(ctx, lay_own, st, ids, c=10.0, active_set=True):
    """diag mass, norms and active set of one context over the owned nodes ``ids`` (global ids) of ``st``; functionals
    are run by the caller once the ghosts are in"""
    import torch

    dim, no = lay_own.dim, lay_own.n_nodes
    out = {}
    m = padded(np.zeros(no))
    ctx.diag_mass_device(m.data_ptr())
    torch.cuda.synchronize()
    mh = m.cpu().numpy()
    assert np.isnan(mh[no:]).all()  # nothing written past n_owned
    out["mass"] = mh[:no]
    r = padded(lay_own.pack(st["res_u"][ids], st["res_phi"][ids]))
    out["norms"] = ctx.residual_norms(r.data_ptr())
    assert ctx.residual_norms(r.data_ptr()) == out["norms"]
    if active_set:
        sol = padded(lay_own.pack(st["u"][ids], st["phi"][ids]))
        old = padded(lay_own.pack(0 * st["u"][ids], st["phi_old"][ids]))
        cyc = dev(np.concatenate([st["cyc"][ids], np.full(no + 16, -7, np.int32)]))
        mass = dev(np.concatenate([st["mass"][ids], [np.nan]]))
        flags_before = ctx.get_constraints()
        try:
            out["counts"] = ctx.active_set_device(r.data_ptr(), mass.data_ptr(), c, sol.data_ptr(), old.data_ptr(), cyc.data_ptr())
            out["status"] = 0
        except PfmError as e:
            out["status"] = e.status
        torch.cuda.synchronize()
        s, k = sol.cpu().numpy(), cyc.cpu().numpy()
        assert np.isnan(s[lay_own.n_dofs:]).all() and (k[no:] == -7).all()
        out["sol"], out["cyc"], out["flags"], out["flags_before"] = s[:lay_own.n_dofs], k[:no], ctx.get_constraints(), flags_before
    return out


def check_partition(g, lps, blocked, cell_owned, c=10.0):
    dim, N = g.dim, g.n_nodes
    st = node_state(g)
    glay = M.DofLayout(N, dim, blocked)
    if g.hn_nodes.size:  # a conforming state: a hanging node's value is its parents' (what every rank computes from)
        v = M.hanging_constraints(g, glay).distribute(glay.pack(st["u"], st["phi"]))
        st["u"] = np.stack([v[glay.dof(np.arange(N), k)] for k in range(dim)], axis=1)
        st["phi"] = v[glay.dof(np.arange(N), dim)]
    prm = bench.sneddon_params(g.min_cell_diameter(), dim)
    hanging_mesh = g.hn_nodes.size > 0
    ref_ctx = new_ctx(g, blocked, prm=prm, flags=st["flags"])
    ref = run_sweeps(ref_ctx, glay, st, np.arange(N), c)
    # the single context itself against the oracle and numpy
    dm = O.diag_mass(g, glay)[glay.dof(np.arange(N), dim)]
    assert np.abs(ref["mass"] - dm).max() <= 1e-13 * np.abs(dm).max()
    z = zero_flagged(glay, glay.pack(st["res_u"], st["res_phi"]), st["flags"], g.hn_nodes)
    l2, linf, sq = numpy_norms(z)
    assert ref["norms"][1] == linf and abs(ref["norms"][2] - sq) <= 1e-13 * sq
    gsol = glay.pack(st["u"], st["phi"])
    if not hanging_mesh:  # and its active set against numpy's statement
        ph = glay.dof(np.arange(N), dim)
        act, sol_phi, cyc_ref, counts_ref = numpy_active_set(np.ones(N, np.uint8), np.zeros(N, np.uint8), st["res_phi"], st["mass"],
                                                             c, st["phi"], st["phi_old"], st["cyc"], (st["flags"] >> dim) & 1)
        assert ref["counts"] == counts_ref and np.array_equal(ref["cyc"], cyc_ref)
        assert np.array_equal((ref["flags"] >> dim) & 1, act) and ref["sol"][ph].tobytes() == sol_phi.tobytes()
    ref_ctx.state_set_host(gsol, gsol, gsol)
    want_f = O.functionals(g, glay, prm, gsol)

    ctxs, outs = [], []
    for r, lp in enumerate(lps):
        no, gid = lp.n_owned, lp.global_ids
        own = M.DofLayout(no, dim, blocked)
        ctx = new_ctx(lp.mesh, blocked, no, prm, st["flags"][gid])
        outs.append(run_sweeps(ctx, own, st, gid[:no], c))
        sol = own.pack(st["u"][gid[:no]], st["phi"][gid[:no]])
        ctx.state_set_host(sol, sol, sol)
        ctx.halo_register(lp.send_ptr, lp.send_nodes, lp.recv_ptr, lp.recv_nodes)
        ctxs.append(ctx)
    _exchange(ctxs, lps, dim)
    f = np.zeros(3)
    sq, linf = 0.0, 0.0
    counts = np.zeros(3, np.int64)
    refused = 0
    for r, (lp, ctx, o) in enumerate(zip(lps, ctxs, outs)):
        no, gid = lp.n_owned, lp.global_ids
        own = M.DofLayout(no, dim, blocked)
        go = gid[:no]
        assert np.abs(o["mass"] - dm[go]).max(initial=0.0) <= 1e-13 * np.abs(dm).max()
        sq += o["norms"][2]
        linf = max(linf, o["norms"][1])
        f += ctx.functionals(cell_owned[r])
        if o["status"] == UNSUPPORTED:  # hanging nodes on a partitioned mesh: refused, nothing touched
            assert lp.mesh.hn_nodes.size > 0
            refused += 1
            assert np.array_equal(o["cyc"], st["cyc"][go])
            assert o["sol"].tobytes() == own.pack(st["u"][go], st["phi"][go]).tobytes()
            assert o["flags"].tobytes() == o["flags_before"].tobytes()
            continue
        assert o["status"] == 0 and lp.mesh.hn_nodes.size == 0
        counts += np.asarray(o["counts"])
        assert o["flags"][no:].tobytes() == st["flags"][gid[no:]].tobytes()  # ghost bytes: untouched
        assert np.array_equal(o["flags"][:no], ref["flags"][go])
        assert np.array_equal(o["cyc"], ref["cyc"][go])
        want_sol = own.pack(np.stack([ref["sol"][glay.dof(go, k)] for k in range(dim)], axis=1), ref["sol"][glay.dof(go, dim)])
        assert o["sol"].tobytes() == want_sol.tobytes()
    assert abs(sq - ref["norms"][2]) <= 1e-13 * ref["norms"][2] and linf == ref["norms"][1]
    for got, want in zip(f, want_f):
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (f, want_f)
    if hanging_mesh:
        assert refused > 0
    else:
        assert refused == 0 and tuple(counts[:2]) == ref["counts"][:2] and min(counts[2], 1) == ref["counts"][2]
        assert ref["counts"][0] > 0 and ref["counts"][2] == 1


def box_cell_owned(n, p, lps):
    # a cell is owned by the rank that owns its vertex 0 (every rank holds the cells around its owned nodes)
    return [(P.owner_of_nodes(n, p, lp.global_ids[lp.mesh.cells[:, 0]]) == r).astype(np.uint8) for r, lp in enumerate(lps)]


@pytest.mark.parametrize("blocked", [True, False], ids=["blocked", "interleaved"])
@pytest.mark.parametrize("dim,n,p", [(2, (13, 9), (2, 1)), (2, (13, 9), (2, 2)), (2, (11, 12), (3, 2)),
                                     (3, (6, 5, 7), (2, 1, 1)), (3, (6, 5, 7), (2, 2, 1)), (3, (5, 6, 7), (1, 2, 3))])
def test_box_partition_sweeps(dim, n, p, blocked):
    g = M.box_mesh(dim, n)
    lps = [P.build_local_problem(dim, n, p, r) for r in range(int(np.prod(p)))]
    assert sum(lp.n_owned for lp in lps) == g.n_nodes
    check_partition(g, lps, blocked, box_cell_owned(n, p, lps))


@pytest.mark.parametrize("blocked", [True, False], ids=["blocked", "interleaved"])
@pytest.mark.parametrize("which", ["box2d", "box3d", "sneddon2d_amr"])
def test_general_partition_sweeps(which, blocked):
    g = {"box2d": lambda: M.box_mesh(2, (10, 7)), "box3d": lambda: M.box_mesh(3, (5, 4, 6)),
         "sneddon2d_amr": M.sneddon_2d_prerefined_mesh}[which]()
    lps = P.partition_general(g, 3 if which != "sneddon2d_amr" else 4)
    check_partition(g, lps, blocked, [lp.cell_owned for lp in lps])


@pytest.mark.parametrize("dim", [2, 3])
def test_rank_that_owns_no_node(dim):
    """zeros and PFM_OK from every sweep, nothing written; also a rank with nodes but no cells"""
    import torch

    g = M.box_mesh(dim, (3,) * dim)
    ctx = new_ctx(g, True, 0, flags=np.full(g.n_nodes, 0xA5, np.uint8))
    sentinel = padded(np.zeros(0))
    ctx.diag_mass_device(sentinel.data_ptr())
    assert ctx.residual_norms(sentinel.data_ptr()) == (0.0, 0.0, 0.0)
    assert ctx.lib.pfm_residual_norms(ctx._h, None, (C.c_double * 3)()) == 0  # NULL is fine with nothing owned
    cyc = dev(np.full(8, -7, np.int32))
    assert ctx.active_set_device(*(sentinel.data_ptr(),) * 2, 10.0, *(sentinel.data_ptr(),) * 2, cyc.data_ptr()) == (0, 0, 0)
    assert ctx.functionals(np.zeros(g.n_cells, np.uint8)) == (0.0, 0.0, 0.0)
    torch.cuda.synchronize()
    assert np.isnan(sentinel.cpu().numpy()).all() and (cyc.cpu().numpy() == -7).all()
    assert (ctx.get_constraints() == 0xA5).all()

    empty = M.Mesh(dim=dim, coords=g.coords.copy(), cells=np.zeros((0, 1 << dim), np.int32), boundary_nodes={})
    ctx = new_ctx(empty, True)
    m = padded(np.full(empty.n_nodes, 3.0))
    ctx.diag_mass_device(m.data_ptr())
    assert ctx.functionals() == (0.0, 0.0, 0.0)
    torch.cuda.synchronize()
    mh = m.cpu().numpy()
    assert (mh[:empty.n_nodes] == 0.0).all() and np.isnan(mh[empty.n_nodes:]).all()


# --------------------------------------------------------------------------------------------- reductions past one grid
@functools.lru_cache(maxsize=None)
def _point_cloud(dim, n_nodes):
    """nodes without cells: the norms only read n_owned, the flags and the vector"""
    rng = np.random.default_rng(dim)
    return M.Mesh(dim=dim, coords=rng.random((n_nodes, dim)), cells=np.zeros((0, 1 << dim), np.int32), boundary_nodes={})


@pytest.mark.parametrize("blocked", [True, False], ids=["blocked", "interleaved"])
@pytest.mark.parametrize("dim", [2, 3])
def test_residual_norms_past_one_grid(dim, blocked):
    import torch

    big = 3 * GRID + 257
    g = _point_cloud(dim, big + 5)
    rng = np.random.default_rng(17 + dim)
    flags = (rng.random((g.n_nodes, dim + 1)) < 0.2).astype(np.uint8) @ (1 << np.arange(dim + 1)).astype(np.uint8)
    flags = flags.astype(np.uint8)
    for no in (1, 255, 256, 257, GRID - 1, GRID, GRID + 1, 2 * GRID + 1, 3 * GRID - 1, big):
        lay = M.DofLayout(no, dim, blocked)
        v = rng.standard_normal(lay.n_dofs) * 10.0 ** rng.integers(-3, 4, lay.n_dofs)
        v[lay.dof(no - 1, dim)] = 1e3 * (1 + rng.random())  # the last owned dof holds the l_inf norm
        flags[no - 1] = 0
        ctx = new_ctx(g, blocked, no, flags=flags)
        t = padded(v)
        got = ctx.residual_norms(t.data_ptr())
        l2, linf, sq = numpy_norms(zero_flagged(lay, v, flags[:no]))
        assert got[1] == linf, no
        assert abs(got[2] - sq) <= 1e-13 * sq and abs(got[0] - l2) <= 1e-13 * l2, (no, got, l2)
        assert ctx.residual_norms(t.data_ptr()) == got
        ctx.close()
        del t
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------ criterion edges
@pytest.mark.parametrize("c", [3.7, 10.0, 0.0])
@pytest.mark.parametrize("dim,blocked", [(2, True), (2, False), (3, True), (3, False)])
def test_criterion_edges_match_unfused_numpy(dim, blocked, c):
    """Exact ties where fma(c, gap, r / m) decides differently, +-0, NaN, +-Inf, c = 0, cycle counters 4 / 5 / 6 from both
    sides, dofs that leave the set: the device makes numpy's decisions, and a second call from the result changes
    nothing."""
    import torch

    res_e, mass_e, sol_e, old_e, cyc_e, was_e, flips = criterion_edges(c if c else 10.0)
    g = M.box_mesh(dim, 20 if dim == 2 else 7)
    N = g.n_nodes
    rng = np.random.default_rng(5)
    at = rng.permutation(N)[:res_e.size]
    mass = 2.0 ** rng.integers(-8, 2, N).astype(np.float64)
    res_phi, sol_phi, old_phi = rng.standard_normal(N) * mass, rng.random(N), rng.random(N)
    cyc, was = rng.integers(0, 7, N).astype(np.int32), (rng.random(N) < 0.4).astype(np.uint8)
    for a, e in ((mass, mass_e), (res_phi, res_e), (sol_phi, sol_e), (old_phi, old_e), (cyc, cyc_e), (was, was_e)):
        a[at] = e
    ubits = rng.integers(0, 1 << dim, N).astype(np.uint8)
    lay = M.DofLayout(N, dim, blocked)
    u_sol, u_res = rng.standard_normal((N, dim)), rng.standard_normal((N, dim))
    ctx = new_ctx(g, blocked, flags=(ubits | (was << dim)).astype(np.uint8))
    sol0 = lay.pack(u_sol, sol_phi)
    d_sol, d_cyc = padded(sol0), dev(cyc)
    d_res, d_mass, d_old = padded(lay.pack(u_res, res_phi)), padded(mass), padded(lay.pack(0 * u_sol, old_phi))
    got = ctx.active_set_device(d_res.data_ptr(), d_mass.data_ptr(), c, d_sol.data_ptr(), d_old.data_ptr(), d_cyc.data_ptr())
    act, sol_ref, cyc_ref, counts = numpy_active_set(np.ones(N, np.uint8), np.zeros(N, np.uint8), res_phi, mass, c, sol_phi,
                                                     old_phi, cyc, was)
    if c:
        assert np.any(flips & ~act[at])  # a fused criterion would decide otherwise here
    assert got == counts
    flags = ctx.get_constraints()
    assert np.array_equal((flags >> dim) & 1, act) and np.array_equal(flags & ((1 << dim) - 1), ubits)
    s = d_sol.cpu().numpy()
    assert s[:lay.n_dofs].tobytes() == lay.pack(u_sol, sol_ref).tobytes() and np.isnan(s[lay.n_dofs:]).all()
    assert np.array_equal(d_cyc.cpu().numpy(), cyc_ref)
    # the resulting set as the previous one, the same inputs: no change, no counter moves
    d_sol, d_cyc = padded(sol0), dev(cyc)
    assert ctx.active_set_device(d_res.data_ptr(), d_mass.data_ptr(), c, d_sol.data_ptr(), d_old.data_ptr(),
                                 d_cyc.data_ptr()) == counts[:2] + (0,)
    torch.cuda.synchronize()
    assert np.array_equal(d_cyc.cpu().numpy(), cyc) and np.array_equal(ctx.get_constraints(), flags)


# ------------------------------------------------------------------------------ hanging nodes, layouts, the material
def box_case(dim, n, blocked, seed=3):
    mesh = M.box_mesh(dim, n)
    lay = M.DofLayout(mesh.n_nodes, dim, blocked)
    prm = O.PfmParams.from_buffer_copy(bytes((cases.kat_sneddon_3d(4) if dim == 3 else cases.kat_sneddon_2d()).params))
    h = mesh.min_cell_diameter()
    prm.alpha_eps = 2.0 * h
    sol = lay.pack(np.zeros((mesh.n_nodes, dim)), M.initial_values_sneddon(mesh, h))
    cu = M.update_constraints(mesh, lay, M.sneddon_dirichlet_dofs(mesh, lay))
    ch = M.hanging_constraints(mesh, lay)
    return cases.perturbed(cases.Case(f"box{dim}d", mesh, lay, prm, sol, sol.copy(), sol.copy(), cu, ch), seed=seed)


SWEEP_CASES = {"hetero_3d": lambda: cases.perturbed(cases.kat_hetero_3d()),
               "box3d_interleaved": lambda: box_case(3, 6, False), "box2d_interleaved": lambda: box_case(2, 9, False),
               "refined_block_blocked": lambda: refined_block_case(4, True),
               "refined_block_interleaved": lambda: refined_block_case(4, False)}


@pytest.mark.parametrize("name", sorted(SWEEP_CASES))
def test_sweeps_on_hanging_nodes_and_layouts(name):
    import torch

    from test_newton_sweeps import _active_set_inputs

    case = SWEEP_CASES[name]()
    lay, dim, nn = case.layout, case.mesh.dim, case.mesh.n_nodes
    ctx = new_ctx(case.mesh, lay.blocked, prm=case.params, flags=node_flags_from_dof_flags(lay, case.cu.flag, case.ch.flag),
                  cell_lambda=case.cell_lambda, cell_mu=case.cell_mu)
    phi_dof = lay.dof(np.arange(nn), dim)
    m = padded(np.zeros(nn))
    ctx.diag_mass_device(m.data_ptr())
    ref = O.diag_mass(case.mesh, lay)[phi_dof]
    assert np.abs(m.cpu().numpy()[:nn] - ref).max() <= 1e-13 * np.abs(ref).max()
    # norms of an arbitrary vector: Dirichlet and hanging lines zeroed by the call
    rng = np.random.default_rng(9)
    r = rng.standard_normal(lay.n_dofs) * 10.0 ** rng.integers(-3, 4, lay.n_dofs)
    d = padded(r)
    got = ctx.residual_norms(d.data_ptr())
    z = case.cu.set_zero(r)
    z[case.ch.flag.astype(bool)] = 0.0
    l2, linf, sq = numpy_norms(z)
    assert got[1] == linf and abs(got[2] - sq) <= 1e-13 * sq and abs(got[0] - l2) <= 1e-13 * l2
    # active set + distribution of the hanging nodes against the oracle
    is_phi, hanging, res, mass, sol, old, cyc, active = _active_set_inputs(case)
    cu_flag = case.cu.flag.copy()
    cu_flag[phi_dof] = active[phi_dof]
    ctx.set_constraints(node_flags_from_dof_flags(lay, cu_flag, case.ch.flag))
    d_res, d_mass, d_sol, d_old = padded(res), padded(mass[phi_dof]), padded(sol), padded(old)
    d_cyc = dev(cyc[phi_dof])
    got = ctx.active_set_device(d_res.data_ptr(), d_mass.data_ptr(), 10.0, d_sol.data_ptr(), d_old.data_ptr(), d_cyc.data_ptr())
    want = O.active_set(is_phi, hanging, res, mass, 10.0, sol, old, cyc, active)
    sol = case.ch.distribute(sol)
    assert got == want and want[0] > 0
    assert np.array_equal(d_cyc.cpu().numpy(), cyc[phi_dof])
    s = d_sol.cpu().numpy()
    assert np.abs(s[:lay.n_dofs] - sol).max() <= 1e-15 and np.isnan(s[lay.n_dofs:]).all()
    flags = ctx.get_constraints()
    assert np.array_equal((flags >> dim) & 1, active[phi_dof])
    if case.ch.flag.any():
        assert not np.any(active[case.ch.flag.astype(bool)])
    torch.cuda.synchronize()


def _hetero_unshifted(case):
    nu = 0.2
    emod = case.cell_mu * 2.0 * (1 + nu) - 1.0  # compute_energy reads func_emodulus without the +1 of cracks.cc:2209-2210
    mu = emod / (2.0 * (1 + nu))
    return (2 * nu * mu) / (1.0 - 2 * nu), mu


@pytest.mark.parametrize("which", ["hetero_3d", "box3d", "box2d"])
def test_functionals_material(which):
    if which == "hetero_3d":
        case = cases.perturbed(cases.kat_hetero_3d())
        lam, mu = _hetero_unshifted(case)
        assert not np.allclose(mu, case.cell_mu)
    else:
        case = box_case(3 if which == "box3d" else 2, 5 if which == "box3d" else 8, True)
        rng = np.random.default_rng(4)
        lam, mu = rng.uniform(0.1, 3.0, case.mesh.n_cells), rng.uniform(0.1, 3.0, case.mesh.n_cells)
    lay = case.layout
    ctx = new_ctx(case.mesh, lay.blocked, prm=case.params, cell_lambda=case.cell_lambda, cell_mu=case.cell_mu)
    ctx.state_set_host(case.sol, case.old, case.oldold)
    mask = (np.arange(case.mesh.n_cells) % 3 != 0).astype(np.uint8)
    for m in (None, mask):
        got = ctx.functionals(m, lam, mu)
        want = O.functionals(case.mesh, lay, case.params, case.sol, lam, mu, m)
        for g_, w in zip(got, want):
            assert abs(g_ - w) <= 1e-12 * max(1.0, abs(w)), (got, want)
        assert got[0] != ctx.functionals(m)[0]  # the override is used
        # both NULL: pfm_functionals, bit for bit
        out = (C.c_double * 3)()
        mp = None if m is None else capi.np_ptr(m, np.uint8)
        assert ctx.lib.pfm_functionals_material(ctx._h, mp, None, None, out) == 0
        assert tuple(out) == ctx.functionals(m)
        # exactly one NULL: refused, out untouched
        la = np.ascontiguousarray(lam)
        for a, b in ((capi.np_ptr(la, np.float64), None), (None, capi.np_ptr(la, np.float64))):
            out = (C.c_double * 3)(-1.0, -2.0, -3.0)
            assert ctx.lib.pfm_functionals_material(ctx._h, mp, a, b, out) == BAD_ARG
            assert tuple(out) == (-1.0, -2.0, -3.0)


def test_functionals_and_norms_interleaved_with_postproc():
    """cod_lines / face_load share d_partial and d_cell_owned with pfm_functionals: interleaved calls, the same bits"""
    case = box_case(2, 12, True)
    ctx = new_ctx(case.mesh, True, prm=case.params, flags=node_flags_from_dof_flags(case.layout, case.cu.flag))
    ctx.state_set_host(case.sol, case.old, case.oldold)
    n = case.mesh.n_cells
    mask_a = (np.arange(n) % 3 != 0).astype(np.uint8)
    mask_b = (np.arange(n) % 2 == 0).astype(np.uint8)
    r = padded(np.random.default_rng(1).standard_normal(case.layout.n_dofs))
    want = (ctx.functionals(mask_a), ctx.functionals(), ctx.residual_norms(r.data_ptr()))
    cells, faces = M.boundary_faces(case.mesh, 3)
    lines = S.cod_lines()
    for _ in range(2):
        ctx.cod_lines(lines, mask_b)
        assert ctx.functionals(mask_a) == want[0]
        ctx.face_load(cells, faces)
        assert ctx.functionals() == want[1]
        assert ctx.residual_norms(r.data_ptr()) == want[2]
        ctx.sneddon_phi_error_sq(mask_b)
        assert ctx.functionals(mask_a) == want[0]
        ctx.cod_lines(lines)
        assert ctx.functionals() == want[1]


# -------------------------------------------------------------------------------------------- the device-resident step
STEP_CASES = {"box3d": lambda: box_case(3, 6, True), "box2d": lambda: box_case(2, 12, True),
              "sneddon_2d": lambda: cases.perturbed(cases.kat_sneddon_2d()),
              "hetero_3d": lambda: cases.perturbed(cases.kat_hetero_3d())}


@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_device_resident_step(name):
    """set_constraints(Dirichlet) -> diag mass -> residual -> active set fed the device residual_total -> solution onto the
    device -> full + residual assembly -> norms, against a second context given the same set through pfm_set_constraints"""
    import torch

    case = STEP_CASES[name]()
    lay, dim, nn, c = case.layout, case.mesh.dim, case.mesh.n_nodes, 10.0
    uniform = name.startswith("box")
    flags0 = node_flags_from_dof_flags(lay, case.cu.flag, case.ch.flag)
    a = Assembler(case.mesh, lay.blocked, cell_lambda=case.cell_lambda, cell_mu=case.cell_mu)
    if uniform:
        assert a.ctx.kernel_path == 1
    a.set_params(case.params)
    a.set_constraints(flags0)
    a.set_vectors(case.sol, case.old, case.oldold)
    mass = torch.zeros(nn, dtype=torch.float64, device=a.dev)
    a.ctx.diag_mass_device(mass.data_ptr())
    a.assemble_nl_residual()
    res_tot = a.system_total_residual.cpu().numpy()
    mass_h = mass.cpu().numpy()
    cyc = torch.zeros(nn, dtype=torch.int32, device=a.dev)
    counts = a.ctx.active_set_device(a.system_total_residual.data_ptr(), mass.data_ptr(), c, a.solution.data_ptr(),
                                     a.old_solution.data_ptr(), cyc.data_ptr())
    a.assemble_system(False, solution_only=True)
    values_a = [v.cpu().numpy() for v in a.system_pde_matrix]
    res_full_a = a.system_pde_residual.cpu().numpy()
    a.assemble_nl_residual(solution_only=True)
    res_a = a.system_pde_residual.cpu().numpy()
    norms = a.ctx.residual_norms(a.system_pde_residual.data_ptr())
    sol_a = a.solution.cpu().numpy()

    # the same set in numpy
    phi = lay.dof(np.arange(nn), dim)
    hang = case.ch.flag[phi].astype(np.uint8)
    was = (flags0 >> dim) & 1
    act, sol_phi, cyc_ref, counts_ref = numpy_active_set(np.ones(nn, np.uint8), hang, res_tot[phi], mass_h, c,
                                                         case.sol[phi], case.old[phi], np.zeros(nn, np.int32), was)
    assert counts == counts_ref and counts[0] > 0 and np.array_equal(cyc.cpu().numpy(), cyc_ref)
    sol_b = case.sol.copy()
    sol_b[phi] = sol_phi
    sol_b = case.ch.distribute(sol_b)
    assert np.abs(sol_a - sol_b).max() <= (0.0 if uniform else 1e-15)
    flags_b = (flags0 & ~np.uint8(1 << dim)) | (act.astype(np.uint8) << dim)
    assert np.array_equal(a.ctx.get_constraints(), flags_b)
    b = Assembler(case.mesh, lay.blocked, cell_lambda=case.cell_lambda, cell_mu=case.cell_mu)
    b.set_params(case.params)
    b.set_constraints(flags_b)
    b.set_vectors(sol_a if uniform else sol_b, case.old, case.oldold)
    b.assemble_system(False)
    values_b = [v.cpu().numpy() for v in b.system_pde_matrix]
    res_full_b = b.system_pde_residual.cpu().numpy()
    b.assemble_nl_residual()
    res_b = b.system_pde_residual.cpu().numpy()
    for va, vb in zip(values_a, values_b):
        assert va.tobytes() == vb.tobytes() if uniform else linf_scaled(va, vb) < 1e-12
    for ra, rb in ((res_full_a, res_full_b), (res_a, res_b)):
        assert ra.tobytes() == rb.tobytes() if uniform else linf_scaled(ra, rb) < 1e-12
    # both against the oracle with the new lines
    cu = M.update_constraints(case.mesh, lay, list(np.nonzero(case.cu.flag)[0]) + list(phi[act]))
    rp, ci = M.dof_sparsity(case.mesh, lay)
    r = O.assemble(case.mesh, lay, case.params, sol_b, case.old, case.oldold, cu, case.ch, False, rp, ci,
                   case.cell_lambda, case.cell_mu)
    assert r.err == 0
    A = blocks_to_global(a.ctx, lay, values_a)
    A.sort_indices()
    A_ref = sp.csr_matrix((r.values, ci, rp), shape=A.shape)
    A_ref.sort_indices()
    assert linf_scaled(A.data, A_ref.data) < 1e-12
    assert linf_scaled(res_full_a, r.residual_pde) < 1e-12 and linf_scaled(res_a, r.residual_pde) < 1e-12
    z = cu.set_zero(res_a)
    z[case.ch.flag.astype(bool)] = 0.0
    assert abs(norms[0] - np.linalg.norm(z)) <= 1e-13 * np.linalg.norm(z) and norms[1] == np.abs(z).max()


# ------------------------------------------------------------------------------------------------------- bad arguments
def test_bad_arguments_leave_the_outputs_untouched():
    import torch

    g = M.box_mesh(2, (4, 3))
    N = g.n_nodes
    raw = Context(g, True)  # no pfm_set_params yet
    lib, h = raw.lib, raw._h
    out = (C.c_double * 3)(-1.0, -2.0, -3.0)
    assert lib.pfm_functionals(h, None, out) == BAD_ARG and tuple(out) == (-1.0, -2.0, -3.0)
    ctx = new_ctx(g, True, flags=np.full(N, 4, np.uint8))
    lib, h = ctx.lib, ctx._h
    v = padded(np.ones(3 * N))
    m = padded(np.ones(N))
    cyc = dev(np.zeros(N, np.int32))
    p = [v.data_ptr(), m.data_ptr(), v.data_ptr(), v.data_ptr(), cyc.data_ptr()]
    assert lib.pfm_diag_mass_device(h, None) == BAD_ARG and lib.pfm_diag_mass_device(None, C.c_void_p(m.data_ptr())) == BAD_ARG
    for k in range(6):
        args = [C.c_void_p(x) for x in p] + [(C.c_int64 * 3)(-1, -1, -1)]
        counts = args[-1]
        if k < 5:
            args[k] = None
        else:
            args[-1] = None
        rc = lib.pfm_active_set_device(h, args[0], args[1], C.c_double(10.0), args[2], args[3], args[4], args[5])
        assert rc == BAD_ARG and tuple(counts) == (-1, -1, -1)
    out = (C.c_double * 3)(-1.0, -2.0, -3.0)
    assert lib.pfm_residual_norms(h, None, out) == BAD_ARG and tuple(out) == (-1.0, -2.0, -3.0)
    assert lib.pfm_residual_norms(h, C.c_void_p(v.data_ptr()), None) == BAD_ARG
    assert lib.pfm_functionals(h, None, None) == BAD_ARG
    assert lib.pfm_get_constraints(h, None) == BAD_ARG
    torch.cuda.synchronize()
    assert (v.cpu().numpy()[:3 * N] == 1.0).all() and (m.cpu().numpy()[:N] == 1.0).all()
    assert (cyc.cpu().numpy() == 0).all() and (ctx.get_constraints() == 4).all()


# --------------------------------------------------------------------------------------------------------- bench size
def _bench_mesh_checks(g, no, gid, state, prm, blocked=True):
    import torch

    dim, N = g.dim, g.n_nodes
    u, phi, po, poo, flags = state
    ctx = new_ctx(g, blocked, no, prm, flags)
    own = M.DofLayout(no, dim, blocked)
    # diag mass: the closed form of a uniform box, h^dim halved once per axis on which the node lies on the boundary
    n_axis = [int(k) for k in g.box_shape]
    m = torch.zeros(no + 8, dtype=torch.float64, device="cuda").fill_(float("nan"))
    ctx.diag_mass_device(m.data_ptr())
    mh = m.cpu().numpy()
    assert np.isnan(mh[no:]).all()
    hs = [20.0 / k for k in n_axis]
    rem = gid[:no].copy()
    want = np.full(no, float(np.prod(hs)))
    for d in range(dim):
        i = rem % (n_axis[d] + 1)
        rem //= n_axis[d] + 1
        want[(i == 0) | (i == n_axis[d])] *= 0.5
    # the bound: the node coordinates (|x| <= 10) carry a rounding that the differences of neighbours (h) inherit
    assert np.abs(mh[:no] - want).max() <= 16 * np.finfo(float).eps * (10.0 / min(hs)) * want.max()
    # norms of the state vector as a residual stand-in, numpy in float64
    rng = np.random.default_rng(216)
    res = own.pack(rng.standard_normal((no, dim)), rng.standard_normal(no) * want)
    d_res = torch.from_numpy(res).to("cuda")
    got = ctx.residual_norms(d_res.data_ptr())
    z = zero_flagged(own, res, flags[:no])
    sq = float(np.sum(z * z))
    assert got[1] == float(np.abs(z).max()) and abs(got[2] - sq) <= 1e-12 * sq
    assert ctx.residual_norms(d_res.data_ptr()) == got
    # active set against the numpy predicate
    sol = own.pack(u[:no], phi[:no])
    old = own.pack(0 * u[:no], po[:no])
    d_sol, d_old = torch.from_numpy(sol).to("cuda"), torch.from_numpy(old).to("cuda")
    cyc = rng.integers(0, 7, no).astype(np.int32)
    d_cyc = torch.from_numpy(cyc).to("cuda")
    d_mass = torch.from_numpy(want).to("cuda")
    del z
    got = ctx.active_set_device(d_res.data_ptr(), d_mass.data_ptr(), 10.0, d_sol.data_ptr(), d_old.data_ptr(), d_cyc.data_ptr())
    ph = own.dof(np.arange(no), dim)
    act, sol_ref, cyc_ref, counts = numpy_active_set(np.ones(no, np.uint8), np.zeros(no, np.uint8), res[ph], want, 10.0,
                                                     sol[ph], old[ph], cyc, (flags[:no] >> dim) & 1)
    assert got == counts and counts[0] > 0
    assert np.array_equal(d_cyc.cpu().numpy(), cyc_ref)
    assert d_sol.cpu().numpy()[ph].tobytes() == sol_ref.tobytes()
    del d_res, d_sol, d_old, d_cyc, d_mass
    # functionals on a few thousand sparse cells, the highest indices included; mask + complement = unmasked
    ctx.state_set_host(own.pack(u[:no], phi[:no]), own.pack(0 * u[:no], po[:no]), own.pack(0 * u[:no], poo[:no]))
    nc = g.n_cells
    sel = np.unique(np.concatenate([rng.choice(nc, 3000, replace=False), np.arange(nc - 40, nc), np.arange(40)]))
    mask = np.zeros(nc, np.uint8)
    mask[sel] = 1
    got = ctx.functionals(mask)
    sub = M.Mesh(dim=dim, coords=g.coords, cells=np.ascontiguousarray(g.cells[sel]), boundary_nodes={})
    glay = M.DofLayout(N, dim, True)
    want_f = O.functionals(sub, glay, prm, glay.pack(u, phi))
    for a_, b_ in zip(got, want_f):
        assert abs(a_ - b_) <= 1e-12 * max(1.0, abs(b_)), (got, want_f)
    full, comp = ctx.functionals(), ctx.functionals(1 - mask)
    for k in range(3):
        assert abs(got[k] + comp[k] - full[k]) <= 1e-12 * max(1.0, abs(full[k]))
    ctx.close()


@pytest.mark.timeout(1500)
def test_bench_meshes():
    """216^3 (bench.py's workload, 10.2 M owned nodes, 20 grid strides of the norms) and config 2's 1000^2"""
    import torch

    n = 216
    g = M.box_mesh(3, n)
    h = (20.0 / n) * np.sqrt(3)
    st = bench.synthetic_state(g, np.arange(g.n_nodes), h, 3)
    _bench_mesh_checks(g, g.n_nodes, np.arange(g.n_nodes), st, bench.sneddon_params(h, 3))
    del g, st
    torch.cuda.empty_cache()
    n2 = 1000
    lp = P.build_local_problem(2, (n2, n2), P.factor_ranks(1, 2), 0)
    h = (20.0 / n2) * np.sqrt(2)
    st = bench.synthetic_state(lp.mesh, lp.global_ids, h, 2)
    _bench_mesh_checks(lp.mesh, lp.n_owned, lp.global_ids, st, bench.sneddon_params(h, 2))
