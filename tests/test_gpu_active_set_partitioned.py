"""The active-set update of a partitioned mesh with hanging nodes (include/pfm_newton.h: pfm_active_set_owned_device,
pfm_halo_pack_flags_all / _unpack_, pfm_distribute_hanging_device, pfm_active_set_exchange) against ONE context over the
whole mesh through pfm_active_set_device: every rank is a context on one device, the messages travel as in-process copies
(newton.active_set_partitioned).  The ghost values and ghost flag bytes are observed by the next assembly, which runs on
every rank without a further state call.  On one rank pfm_active_set_exchange(comm = NULL) equals pfm_active_set_device
bit for bit."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import active_set_cases as A
import bench
import oracle_api as O
from cracks_amd import mesh as M
from cracks_amd import newton as NW
from cracks_amd import partition as P
from gpu_util import TOL, linf_scaled
from test_gpu_newton_device import dev, new_ctx, padded
from test_gpu_postproc import _exchange

pytestmark = pytest.mark.gpu

BAD_ARG = 1
SENTINEL = 0xEE


def dof_vectors(lay, st, ids):
    """residual_total, solution, old solution of the nodes ``ids`` (global) in the layout ``lay`` over them"""
    return (lay.pack(st["res_u"][ids], st["res_phi"][ids]), lay.pack(st["u"][ids], st["phi"][ids]),
            lay.pack(0 * st["u"][ids], st["phi_old"][ids]))


class Rank:
    """a context over the nodes ``ids`` with the state of ``st`` scattered and the inputs of the update on the device"""

    def __init__(self, mesh, blocked, n_owned, ids, st, prm):
        self.no, self.lay = n_owned, M.DofLayout(n_owned, mesh.dim, blocked)
        own = ids[:n_owned]
        self.ctx = new_ctx(mesh, blocked, n_owned, prm, st["flags"][ids])
        res, sol, old = dof_vectors(self.lay, st, own)
        self.sol0 = sol
        if n_owned:
            self.ctx.state_set_host(sol, old, old)
        self.res, self.sol, self.old = padded(res), padded(sol), padded(old)
        self.mass = dev(np.concatenate([st["mass"][own], [np.nan]]))
        self.cyc = dev(np.concatenate([st["cyc"][own], np.full(n_owned + 16, -7, np.int32)]))

    def args(self):
        return (self.res.data_ptr(), self.mass.data_ptr(), A.C_CONST, self.sol.data_ptr(), self.old.data_ptr(), self.cyc.data_ptr())

    def read(self):
        """(solution, cycle counters) with the paddings checked"""
        import torch

        torch.cuda.synchronize()
        s, k = self.sol.cpu().numpy(), self.cyc.cpu().numpy()
        assert np.isnan(s[self.lay.n_dofs:]).all() and (k[self.no:] == -7).all()
        for t in (self.res, self.old):
            assert np.isnan(t.cpu().numpy()[self.lay.n_dofs:]).all()
        return s[:self.lay.n_dofs], k[:self.no]

    def assemble(self):
        """residual-only call, then the full one, on the node state and flags the context holds: (values, res_pde of
        the residual call, res_pde of the full call)"""
        import torch

        n = self.lay.n_dofs
        pde, tot = padded(np.zeros(n)), padded(np.zeros(n))
        self.ctx.assemble_device(True, [], pde.data_ptr(), tot.data_ptr())
        self.ctx.sync_status()
        r1 = pde.cpu().numpy()[:n].copy()
        vals = [torch.zeros(max(self.ctx.pattern_size(b)[1], 1), dtype=torch.float64, device="cuda") for b in range(self.ctx.n_blocks)]
        self.ctx.assemble_device(False, [v.data_ptr() for v in vals], pde.data_ptr(), tot.data_ptr())
        self.ctx.sync_status()
        return [v.cpu().numpy()[:self.ctx.pattern_size(b)[1]] for b, v in enumerate(vals)], r1, pde.cpu().numpy()[:n]


def block_shape(blocked, dim, b):
    """components per node of the rows and of the columns of block b"""
    if not blocked:
        return dim + 1, dim + 1
    return (dim if b in (0, 1) else 1), (dim if b in (0, 2) else 1)


def global_block(ctx, values, b, blocked, dim, gi, N):
    """block b of a context's matrix as a CSR over the global nodes, and the global rows it holds"""
    ncr, ncc = block_shape(blocked, dim, b)
    rp, ci = ctx.pattern(b)
    lrow = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    grow = gi[lrow // ncr] * ncr + lrow % ncr
    gcol = gi[ci // ncc] * ncc + ci % ncc
    m = sp.csr_matrix((values[b], (grow, gcol)), shape=(N * ncr, N * ncc))
    return m, np.unique(grow)


def other_rank_parent_changed(lps, st, ref):
    """local hanging nodes with a parent that another rank owns and whose phi the update changed, over all ranks"""
    changed = ref["phi_before_distribute"] != st["phi"]
    n = 0
    for lp in lps:
        m = lp.mesh
        for k in range(m.hn_nodes.size):
            par = m.hn_parents[m.hn_ptr[k]:m.hn_ptr[k + 1]]
            n += int(np.any((par >= lp.n_owned) & changed[lp.global_ids[par]]))
    return n


CASES = [("sneddon2d_amr", 2, True, "closure"), ("sneddon2d_amr", 3, False, "closure"), ("sneddon2d_amr", 4, True, "closure"),
         ("sneddon2d_amr", 4, False, "dealii+shipped"), ("hang3d", 2, True, "closure"), ("hang3d", 3, False, "closure"),
         ("hetero3d", 4, True, "closure")]


@pytest.mark.parametrize("name,world,blocked,ghost_layer", CASES,
                         ids=[f"{n}-w{w}-{'blocked' if b else 'interleaved'}-{g}" for n, w, b, g in CASES])
def test_partitioned_update_equals_the_single_context(name, world, blocked, ghost_layer):
    g, st = A.mesh_of(name), A.node_state(name)
    lps = A.partition_of(name, world, ghost_layer)
    dim, N, bit = g.dim, g.n_nodes, 1 << g.dim
    glay = M.DofLayout(N, dim, blocked)
    prm = bench.sneddon_params(g.min_cell_diameter(), dim)
    both = A.split_hanging_counts(lps)
    assert both[0] > 0 and both[1] > 0
    stmt = A.global_statement(g, st)
    ghost_bits = sum(int(np.sum(((st["flags"][lp.global_ids[lp.n_owned:]] & bit) != 0) != stmt["active"][lp.global_ids[lp.n_owned:]]))
                     for lp in lps)
    assert ghost_bits > 0 and other_rank_parent_changed(lps, st, stmt) > 0

    # the reference: one context over the whole mesh
    ref = Rank(g, blocked, N, np.arange(N), st, prm)
    ref_counts = ref.ctx.active_set_device(*ref.args())
    ref_sol, ref_cyc = ref.read()
    ref_flags = ref.ctx.get_constraints()
    assert ref_counts == stmt["counts"] and np.array_equal((ref_flags & bit) != 0, stmt["active"])
    ref.ctx.state_set_solution_device(ref.sol.data_ptr())
    ref_vals, ref_res, ref_res_full = ref.assemble()
    # ... whose residual is the oracle's for these lines
    flagged = np.concatenate([glay.dof(np.nonzero((ref_flags >> c) & 1)[0], c) for c in range(dim + 1)])
    _, _, old = dof_vectors(glay, st, np.arange(N))
    r = O.assemble(g, glay, prm, ref_sol, old, old, M.update_constraints(g, glay, flagged), M.hanging_constraints(g, glay), True)
    assert r.err == 0 and linf_scaled(ref_res, r.residual_pde) < TOL and linf_scaled(ref_res_full, r.residual_pde) < TOL
    ref_mats = [global_block(ref.ctx, ref_vals, b, blocked, dim, np.arange(N), N)[0] for b in range(ref.ctx.n_blocks)]

    ranks = [Rank(lp.mesh, blocked, lp.n_owned, lp.global_ids, st, prm) for lp in lps]
    for lp, rk in zip(lps, ranks):
        rk.ctx.halo_register(lp.send_ptr, lp.send_nodes, lp.recv_ptr, lp.recv_nodes)
    _exchange([rk.ctx for rk in ranks], lps, dim)  # the ghost import of the assembly before the update
    counts = NW.active_set_partitioned([rk.ctx for rk in ranks], lps, *[[rk.args()[k] for rk in ranks] for k in (0, 1)], A.C_CONST,
                                       *[[rk.args()[k] for rk in ranks] for k in (3, 4, 5)])
    total = np.sum(np.asarray(counts), axis=0)
    assert tuple(total[:2]) == ref_counts[:2] and min(total[2], 1) == ref_counts[2]
    for lp, rk in zip(lps, ranks):
        no, gi = lp.n_owned, lp.global_ids
        go = gi[:no]
        sol, cyc = rk.read()
        want = rk.lay.pack(np.stack([ref_sol[glay.dof(go, k)] for k in range(dim)], axis=1), ref_sol[glay.dof(go, dim)])
        assert sol.tobytes() == want.tobytes()
        assert np.array_equal(cyc, ref_cyc[go])
        f = rk.ctx.get_constraints()
        assert np.array_equal(f[:no], ref_flags[go])
        assert np.array_equal(f[no:] & bit, ref_flags[gi[no:]] & bit)
        assert np.array_equal(f[no:] & (bit - 1), st["flags"][gi[no:]] & (bit - 1))
        # the next assembly, residual and Jacobian, with no further state call: owned rows at the parity bar
        vals, res, res_full = rk.assemble()
        for c in range(dim + 1):
            for got in (res, res_full):
                assert linf_scaled(got[rk.lay.dof(np.arange(no), c)], ref_res[glay.dof(go, c)]) < TOL
        for b in range(rk.ctx.n_blocks):
            m, rows = global_block(rk.ctx, vals, b, blocked, dim, gi, N)
            got, want = m[rows], ref_mats[b][rows]
            got.sort_indices()
            want.sort_indices()
            assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
            assert linf_scaled(got.data, want.data) < TOL


@pytest.mark.parametrize("blocked", [True, False], ids=["blocked", "interleaved"])
@pytest.mark.parametrize("name", ["sneddon2d_amr", "hang3d"])
def test_one_rank_equals_active_set_device_bit_for_bit(name, blocked):
    g, st = A.mesh_of(name), A.node_state(name)
    N, dim = g.n_nodes, g.dim
    prm = bench.sneddon_params(g.min_cell_diameter(), dim)
    ids = np.arange(N)
    a, b, c = (Rank(g, blocked, N, ids, st, prm) for _ in range(3))
    want_counts = a.ctx.active_set_device(*a.args())
    want_sol, want_cyc = a.read()
    assert want_counts[0] > 0 and want_counts[2] == 1
    hang_dofs = np.concatenate([a.lay.dof(g.hn_nodes, k) for k in range(dim + 1)])
    assert np.any(want_sol[hang_dofs] != a.sol0[hang_dofs])  # the distribution moved hanging values
    assert b.ctx.active_set_exchange(0, None, *b.args()) == want_counts
    sol, cyc = b.read()
    assert sol.tobytes() == want_sol.tobytes() and np.array_equal(cyc, want_cyc)
    assert np.array_equal(b.ctx.get_constraints(), a.ctx.get_constraints())
    b.ctx.distribute_hanging_device(b.sol.data_ptr())  # idempotent
    assert b.read()[0].tobytes() == want_sol.tobytes()
    _, res_b, _ = b.assemble()
    # d_solution = NULL: the node arrays only
    assert c.ctx.active_set_owned_device(*c.args()) == want_counts
    owned_only = c.read()[0].copy()
    assert owned_only[hang_dofs].tobytes() == c.sol0[hang_dofs].tobytes()  # the owned sweep leaves the hanging values
    c.ctx.state_set_solution_device(c.sol.data_ptr())
    c.ctx.distribute_hanging_device(0)
    assert c.read()[0].tobytes() == owned_only.tobytes()
    _, res_c, _ = c.assemble()
    assert linf_scaled(res_c, res_b) < TOL
    # (what the comparison can see: without the distribution the residual is another one)
    c.ctx.state_set_solution_device(c.sol.data_ptr())
    assert linf_scaled(c.assemble()[1], res_b) > 1e3 * TOL


def test_flag_messages_stay_inside_their_buffers():
    """pack: the flag bytes of the send nodes, peer k at byte send_ptr[k]; unpack: bit dim of the ghosts only; sentinel
    bytes behind both buffers and NaN behind the value message survive"""
    import torch

    name, world = "sneddon2d_amr", 3
    g, st, lps = A.mesh_of(name), A.node_state(name), A.partition_of(name, world)
    dim, bit = g.dim, 1 << g.dim
    prm = bench.sneddon_params(g.min_cell_diameter(), dim)
    for lp in lps:
        rk = Rank(lp.mesh, True, lp.n_owned, lp.global_ids, st, prm)
        rk.ctx.halo_register(lp.send_ptr, lp.send_nodes, lp.recv_ptr, lp.recv_nodes)
        ns, nr, no = int(lp.send_ptr[-1]), int(lp.recv_ptr[-1]), lp.n_owned
        assert ns > 0 and nr > 0
        buf = torch.full((ns + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        val = torch.full(((dim + 3) * ns + 64,), float("nan"), dtype=torch.float64, device="cuda")
        rk.ctx.halo_pack_flags_all(buf.data_ptr())
        rk.ctx.halo_pack_all(val.data_ptr())
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        f0 = st["flags"][lp.global_ids]
        assert np.array_equal(h[:ns], f0[lp.send_nodes]) and (h[ns:] == SENTINEL).all()
        assert np.isnan(val.cpu().numpy()[(dim + 3) * ns:]).all()
        msg = np.random.default_rng(3).integers(0, 256, nr + 64).astype(np.uint8)
        rk.ctx.halo_unpack_flags_all(dev(msg).data_ptr())
        torch.cuda.synchronize()
        f = rk.ctx.get_constraints()
        want = f0.copy()
        want[lp.recv_nodes] = (f0[lp.recv_nodes] & ~np.uint8(bit)) | (msg[:nr] & np.uint8(bit))
        assert np.array_equal(f, want) and np.array_equal(f[:no], f0[:no])
        assert np.any(f[no:] != f0[no:])
        rk.read()  # nothing else moved


def test_rank_without_owned_nodes_and_contexts_without_hanging_nodes_or_peers():
    import torch

    g = A.mesh_of("hang3d")
    st = A.node_state("hang3d")
    prm = bench.sneddon_params(g.min_cell_diameter(), 3)
    rk = Rank(g, True, 0, np.arange(g.n_nodes), st, prm)  # every node a ghost, hanging ones included
    assert rk.ctx.active_set_owned_device(*rk.args()) == (0, 0, 0)
    assert rk.ctx.active_set_exchange(0, None, *rk.args()) == (0, 0, 0)
    rk.ctx.distribute_hanging_device(rk.sol.data_ptr())
    rk.read()
    assert np.array_equal(rk.ctx.get_constraints(), st["flags"])
    # no hanging nodes, no peers: PFM_OK with nothing to do
    box = M.box_mesh(2, (4, 3))
    ctx = new_ctx(box, True, flags=np.full(box.n_nodes, 4, np.uint8))
    v = padded(np.ones(3 * box.n_nodes))
    ctx.distribute_hanging_device(v.data_ptr())
    ctx.distribute_hanging_device(0)
    ctx.halo_exchange_flags(0, [])
    assert ctx.lib.pfm_halo_pack_flags_all(ctx._h, None) == 0 and ctx.lib.pfm_halo_unpack_flags_all(ctx._h, None) == 0
    torch.cuda.synchronize()
    assert (v.cpu().numpy()[:3 * box.n_nodes] == 1.0).all() and (ctx.get_constraints() == 4).all()


def test_bad_arguments_leave_the_state_untouched():
    import torch

    name = "sneddon2d_amr"
    g, st, lps = A.mesh_of(name), A.node_state(name), A.partition_of(name, 2)
    lp = lps[0]
    prm = bench.sneddon_params(g.min_cell_diameter(), g.dim)
    rk = Rank(lp.mesh, True, lp.n_owned, lp.global_ids, st, prm)
    rk.ctx.halo_register(lp.send_ptr, lp.send_nodes, lp.recv_ptr, lp.recv_nodes)
    lib, h = rk.ctx.lib, rk.ctx._h
    p = [C.c_void_p(x) if k != 2 else C.c_double(x) for k, x in enumerate(rk.args())]
    peers = np.asarray(lp.peers, np.int32)
    pr = C.c_void_p(peers.ctypes.data)
    for k in [0, 1, 3, 4, 5, 6]:  # each pointer NULL in turn, then the counts
        counts = (C.c_int64 * 3)(-1, -1, -1)
        a = list(p) + [counts]
        a[k] = None
        assert lib.pfm_active_set_owned_device(h, *a) == BAD_ARG
        assert lib.pfm_active_set_exchange(h, None, None, *a) == BAD_ARG
        assert tuple(counts) == (-1, -1, -1)
    counts = (C.c_int64 * 3)(-1, -1, -1)
    assert lib.pfm_active_set_owned_device(None, *p, counts) == BAD_ARG
    assert lib.pfm_active_set_exchange(None, None, None, *p, counts) == BAD_ARG
    # peers without a communicator or without their ranks
    assert lib.pfm_active_set_exchange(h, None, pr, *p, counts) == BAD_ARG
    assert lib.pfm_halo_exchange_flags(h, None, pr) == BAD_ARG and lib.pfm_halo_exchange_flags(None, None, None) == BAD_ARG
    assert tuple(counts) == (-1, -1, -1)
    assert lib.pfm_halo_pack_flags_all(h, None) == BAD_ARG and lib.pfm_halo_unpack_flags_all(h, None) == BAD_ARG
    assert lib.pfm_halo_pack_flags_all(None, C.c_void_p(rk.sol.data_ptr())) == BAD_ARG
    assert lib.pfm_halo_unpack_flags_all(None, C.c_void_p(rk.sol.data_ptr())) == BAD_ARG
    assert lib.pfm_distribute_hanging_device(None, C.c_void_p(rk.sol.data_ptr())) == BAD_ARG
    torch.cuda.synchronize()
    sol, cyc = rk.read()
    assert sol.tobytes() == rk.sol0.tobytes() and np.array_equal(cyc, st["cyc"][lp.global_ids[:lp.n_owned]])
    assert np.array_equal(rk.ctx.get_constraints(), st["flags"][lp.global_ids])
