"""Every z-chunk length of the marching kernels of the cartesian family: k_cart_uu3, k_cart_phi4, the 3-D residual kernels
(k_cart_residual3x / 3d / 3) and k_cart_residual2m.

A workgroup of these kernels marches through one chunk of node planes (2-D: node rows): it recomputes a start-up cell
layer, carries partial sums from plane to plane and keeps a ring of nodal planes in LDS; the residual kernels also move
planes from global memory to LDS two steps ahead.  The length is picked at launch (choose_zchunk) from the tile count, the
plane count and the CU count -- 31 planes for the Jacobian kernels and 22 for the residual at 216^3, other lengths on a
rank's sub-box -- while oracle-sized boxes only ever get the shortest ones.  pfm_ctx_force_zchunk sets the length per
context, so here every length of a kernel's range runs on a box of a few thousand cells:

1. the read-back (pfm_ctx_zchunk) is the forced length: the sweep really changes the launch;
2. with the outputs prefilled with NaN, every value of every block and both residuals equal the run at the model's own
   length on the same context, bit for bit -- a skipped or doubled chunk shows as NaN or as other bits.  The row-owner
   kernels form each row's sums in a fixed order whatever chunk the row falls in, so no tolerance is needed;
3. the run at the model's length matches the oracle (1e-12 max(1, |x_ref|_inf)), once per variant.
"""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from cracks_amd.assembler import Context
from cracks_amd.capi import PfmError
from gpu_util import blocks_to_global, exchange_ghosts, linf_scaled, make_context, reference_parity, residual_parity
from test_gpu_cart import box_case, dead_zone, heterogeneous, oracle

pytestmark = pytest.mark.gpu
TOL = 1e-12
UU3, PHI4, RES3, RES2 = Context.ZC_UU3, Context.ZC_PHI4, Context.ZC_RES3, Context.ZC_RES2
RANGE = {UU3: (8, 48), PHI4: (6, 48), RES3: (4, 24), RES2: (4, 64)}  # what the model may pick (zchunk_of, pfm_cart.hip)
ENV = {UU3: "PFM_UU_ZC", PHI4: "PFM_PHI_ZC", RES3: "PFM_RES_ZC", RES2: "PFM_RES2_ZC"}
NAME = {UU3: "k_cart_uu3", PHI4: "k_cart_phi4", RES3: "3-D residual", RES2: "k_cart_residual2m"}
# (16, 9, 60): partial tiles of k_cart_uu3 (8 x 4 nodes), k_cart_phi4 (7 x 7) and the residual (15 x 15), 61 planes (prime:
# every length leaves a short last chunk); (5, 4, 61): 62 planes, 31 divides them as it divides the 217 planes of 216^3
BOXES3 = [(16, 9, 60), (5, 4, 61)]
# (70, 130): 71 nodes in x, a partial wave of k_cart_residual2m (62 nodes), 131 rows (prime); (61, 127): one full wave,
# 128 = 2 x 64 rows
BOXES2 = [(70, 130), (61, 127)]


def _same_bits(a, b):
    import torch

    return a.shape == b.shape and torch.equal(a.view(torch.int64), b.view(torch.int64))


def _diff(a, b):
    import torch

    return f"{int((a.view(torch.int64) != b.view(torch.int64)).sum())} entries differ, {int(torch.isnan(a).sum())} NaN"


class Outputs:
    """Device buffers of one context's assemblies: a full one writes the value blocks and res_pde, a residual-only one
    res_pde and res_tot.  run() prefills them with NaN, assembles and returns copies (on the device)."""

    def __init__(self, ctx, residual_only, sol=None):
        import torch

        z = lambda k: torch.empty(k, dtype=torch.float64, device="cuda")
        self.ctx, self.residual_only = ctx, residual_only
        self.vals = [] if residual_only else [z(ctx.pattern_size(b)[1]) for b in range(ctx.n_blocks)]
        self.res = [z(ctx.n_owned_dofs), z(ctx.n_owned_dofs)]
        self.outs = self.res if residual_only else self.vals + self.res[:1]
        # sol: the line-search entry point (pfm_assemble_nl_residual_device) reads this device solution itself
        self.sol = None if sol is None else torch.from_numpy(np.ascontiguousarray(sol)).cuda()

    def run(self, fill=True):
        if fill:
            for o in self.outs:
                o.fill_(float("nan"))
        if self.sol is not None:
            self.ctx.assemble_nl_residual_device(self.sol.data_ptr(), self.res[0].data_ptr(), self.res[1].data_ptr())
        else:
            self.ctx.assemble_device(self.residual_only, [v.data_ptr() for v in self.vals], self.res[0].data_ptr(),
                                     self.res[1].data_ptr())
        self.ctx.sync_status()
        return [o.clone() for o in self.outs]


def check_bits(got, ref, tag):
    for k, (a, b) in enumerate(zip(got, ref)):
        assert _same_bits(a, b), f"{tag}: output {k} differs from the run at the model's length ({_diff(a, b)})"


def planes_of(ctx, kernel):
    """the plane count of the context's box along the kernel's march: a forced length is clamped to it"""
    ctx.force_zchunk(kernel, 1 << 20)
    p = ctx.zchunk(kernel)
    ctx.force_zchunk(kernel, 0)
    return p


def sweep(ctx, kernel, runs, refs, tag, lengths=None):
    """every length of the kernel's range bounded by the plane count (or `lengths`): the read-back first, then every output
    of every run bitwise against refs; the default restored afterwards"""
    planes = planes_of(ctx, kernel)
    lo, hi = (min(x, planes) for x in RANGE[kernel])
    for L in (range(lo, hi + 1) if lengths is None else lengths):
        ctx.force_zchunk(kernel, L)
        assert ctx.zchunk(kernel) == L, f"{tag}: {NAME[kernel]} forced to {L} of {planes} planes"
        for r, ref in zip(runs, refs):
            check_bits(r.run(), ref, f"{tag}, {NAME[kernel]} at {L} of {planes} planes")
    ctx.force_zchunk(kernel, 0)


def full_against_oracle(c, ctx, outs):
    r, rp, ci = oracle(c, False)
    A_ref = sp.csr_matrix((r.values, ci, rp), shape=(c.layout.n_dofs,) * 2)
    A = blocks_to_global(ctx, c.layout, [v.cpu().numpy() for v in outs[:-1]])
    A.sort_indices()
    assert (A.indptr == A_ref.indptr).all() and (A.indices == A_ref.indices).all()
    assert linf_scaled(A.data, A_ref.data) < TOL
    assert linf_scaled(outs[-1].cpu().numpy(), r.residual_pde) < TOL
    reference_parity(c.layout, c.sol, A, A_ref, [(outs[-1].cpu().numpy(), r.residual_pde, "pde")], tag=f"zchunks {c.name}")


def residual_against_oracle(c, outs):
    r, _, _ = oracle(c, True)
    assert linf_scaled(outs[0].cpu().numpy(), r.residual_pde) < TOL
    assert linf_scaled(outs[1].cpu().numpy(), r.residual_total) < TOL
    residual_parity(c, outs[0].cpu().numpy(), outs[1].cpu().numpy(), r.residual_pde, r.residual_total, tag="zchunks")


def case3(n, kind, blocked):
    """stag: the pair k_cart_uu3 + k_cart_phi4 writes the residual rows; mono: the monolithic scheme (old phase fields in
    k_cart_phi4's ring, the quadrature residual kernel next to the Jacobian); het: per-cell Lame coefficients (the residual
    kernel too); dead: Dirichlet lines, an active set and a dead zone with kappa = 0 (placeholder diagonals)"""
    c = box_case(3, n, -10.0, 10.0, blocked, monolithic=kind == "mono")
    if kind == "dead":
        dead_zone(c)
    if kind == "het":
        heterogeneous(c, seed=7)
    return c


def _context(c):
    ctx = make_context(c)
    assert ctx.kernel_path == 1
    ctx.state_set_host(c.sol, c.old, c.oldold)
    return ctx


# ---- the hook itself --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n", [(3, (16, 9, 60)), (3, (6, 6, 6)), (2, (70, 130)), (2, (5, 3))])
def test_force_and_read_back_the_chunk_lengths(dim, n):
    ctx = make_context(box_case(dim, n, -10.0, 10.0, True))
    assert ctx.kernel_path == 1
    kernels = (UU3, PHI4, RES3) if dim == 3 else (RES2,)
    planes = n[-1] + 1
    model = {k: ctx.zchunk(k) for k in kernels}
    for k in kernels:
        env = int(os.environ.get(ENV[k]) or 0)
        if env > 0:  # the tuning variable stands in for the model
            assert model[k] == min(env, planes)
        else:
            assert min(RANGE[k][0], planes) <= model[k] <= min(RANGE[k][1], planes)
        for L in (1, 2, 5, planes - 1, planes, planes + 1, 1000):
            ctx.force_zchunk(k, L)
            assert ctx.zchunk(k) == min(L, planes)
            assert all(ctx.zchunk(o) == model[o] for o in kernels if o != k), "one kernel's length only"
        ctx.force_zchunk(k, 0)
        assert ctx.zchunk(k) == model[k], "0 restores the default"
    for k in {UU3, PHI4, RES3, RES2} - set(kernels):  # the kernels of the other dimension
        ctx.force_zchunk(k, 8)
        with pytest.raises(PfmError) as e:
            ctx.zchunk(k)
        assert e.value.status == 5  # PFM_ERR_UNSUPPORTED
        ctx.force_zchunk(k, 0)
    for bad in ((-1, 8), (4, 8), (kernels[0], -1)):
        with pytest.raises(PfmError) as e:
            ctx.force_zchunk(*bad)
        assert e.value.status == 1  # PFM_ERR_BAD_ARG
    for bad in (-1, 4):
        with pytest.raises(PfmError) as e:
            ctx.zchunk(bad)
        assert e.value.status == 1
    assert ctx.lib.pfm_ctx_zchunk(ctx._h, kernels[0], None) == 1
    ctx.close()


# ---- 3-D Jacobian: k_cart_uu3 and k_cart_phi4 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("blocked", [True, False])  # k_cart_uu3 with NC = 3 and NC = 4
@pytest.mark.parametrize("kind", ["stag", "mono", "het", "dead"])
@pytest.mark.parametrize("n", BOXES3)
def test_jacobian_kernels_at_every_chunk_length(n, kind, blocked):
    """k_cart_uu3 over 8..48 planes with k_cart_phi4 at its default, then k_cart_phi4 over 6..48 with k_cart_uu3 at its
    default; the residual of the same call (from the matrix rows, or the residual kernel's at its default)"""
    c = case3(n, kind, blocked)
    ctx = _context(c)
    full = Outputs(ctx, False)
    W = full.run()
    assert not any(bool(w.isnan().any()) for w in W), "the default run leaves no entry unwritten"
    full_against_oracle(c, ctx, W)
    tag = f"{n} {kind} {'blocked' if blocked else 'interleaved'}"
    sweep(ctx, UU3, [full], [W], tag)
    sweep(ctx, PHI4, [full], [W], tag)
    check_bits(full.run(), W, f"{tag}: defaults restored")
    ctx.close()


# ---- 3-D residual kernels ------------------------------------------------------------------------------------------------------
RES3_VARIANTS = [  # (kind, blocked, environment, line-search entry point): the kernel that runs
    ("stag", True, {}, True),                                      # k_cart_residual3x (blocked solution read in place)
    ("stag", True, {"PFM_RES_NO_WIDE_TRANSFERS": "1"}, True),      # k_cart_residual3d (dword transfers)
    ("stag", True, {"PFM_RES_NO_TRANSFERS": "1"}, True),           # k_cart_residual3 <true> (planes through registers)
    ("stag", False, {}, False),                                    # k_cart_residual3d, interleaved layout
    ("mono", True, {}, False),                                     # k_cart_residual3 <false>
    ("het", True, {}, True),                                       # k_cart_residual3x <HET>
]


@pytest.mark.parametrize("kind,blocked,env,nl", RES3_VARIANTS)
@pytest.mark.parametrize("n", BOXES3)
def test_residual_kernels_at_every_chunk_length(n, kind, blocked, env, nl, monkeypatch):
    for k, v in env.items():  # read per launch
        monkeypatch.setenv(k, v)
    c = case3(n, kind, blocked)
    ctx = _context(c)
    res = Outputs(ctx, True, sol=c.sol if nl else None)
    R = res.run()
    assert not any(bool(r.isnan().any()) for r in R)
    residual_against_oracle(c, R)
    sweep(ctx, RES3, [res], [R], f"{n} {kind} {'blocked' if blocked else 'interleaved'} {env}")
    ctx.close()


# ---- 2-D residual: k_cart_residual2m (a 2-D Jacobian call writes its residual from k_cart2d_cells) -----------------------------
@pytest.mark.parametrize("blocked", [True, False])
@pytest.mark.parametrize("monolithic", [False, True])  # k_cart_residual2m <true> / <false>
@pytest.mark.parametrize("n", BOXES2)
def test_residual2m_at_every_chunk_length(n, monolithic, blocked):
    c = box_case(2, n, -10.0, 10.0, blocked, monolithic=monolithic)
    ctx = _context(c)
    plain, nl = Outputs(ctx, True), Outputs(ctx, True, sol=c.sol)
    R = plain.run()
    assert not any(bool(r.isnan().any()) for r in R)
    residual_against_oracle(c, R)
    check_bits(nl.run(), R, "line-search entry point")
    sweep(ctx, RES2, [plain, nl], [R, R], f"{n} {'mono' if monolithic else 'stag'} {'blocked' if blocked else 'interleaved'}")
    ctx.close()


# ---- partitioned ranks: chunk origins offset by o0[2] > 0, ghost planes above and below ------------------------------------------
def _handful(planes, kernel):
    """min, max and +-1 around a divisor of the plane count, within the kernel's range"""
    lo, hi = (min(x, planes) for x in RANGE[kernel])
    divs = [d for d in range(max(lo, 2), min(hi, planes - 1) + 1) if planes % d == 0] or [max(lo, (planes + 1) // 2)]
    d = divs[-1]
    return sorted({x for x in (lo, hi, d - 1, d, d + 1) if lo <= x <= hi})


@pytest.mark.parametrize("kind", ["stag", "mono"])
@pytest.mark.parametrize("p,n", [((1, 1, 2), (9, 8, 60)), ((2, 2, 2), (17, 9, 40))])
def test_partition_pieces_at_chunk_lengths(p, n, kind):
    """per rank: the whole assembly (full and residual-only) at a handful of lengths of every kernel, bitwise against the
    rank's default run; and phase 1 + phase 2 of the overlapped assembly at those lengths of the residual kernel, bitwise
    equal to the whole assembly -- phase 2 launches the boundary tiles of the residual kernel from a list keyed by its
    length, which pfm_ctx_force_zchunk drops and the next phase rebuilds"""
    from test_gpu_overlap_phases import box_ranks, global_case

    c = global_case(3, n, kind, True)
    ranks = box_ranks(c, n, p)
    recv = exchange_ghosts([r.lp for r in ranks], [r.ctx for r in ranks], 3)
    for rank, buf in zip(ranks, recv):
        ctx = rank.ctx
        if buf.numel():
            ctx.halo_unpack_all(buf.data_ptr())
        full, res = Outputs(ctx, False), Outputs(ctx, True)
        W, R = full.run(), res.run()
        assert not any(bool(w.isnan().any()) for w in W + R)
        tag = f"{p} {kind} rank {rank.index}"
        for k in (UU3, PHI4, RES3):
            sweep(ctx, k, [full, res], [W, R], tag, _handful(planes_of(ctx, k), k))
        for L in _handful(planes_of(ctx, RES3), RES3):
            ctx.force_zchunk(RES3, L)
            assert ctx.zchunk(RES3) == L
            for o, ref in ((full, W), (res, R)):
                ctx.force_phase(1)
                o.run()
                ctx.force_phase(2)
                got = o.run(fill=False)
                ctx.force_phase(0)
                check_bits(got, ref, f"{tag}: phase 1 + phase 2, residual kernel at {L} planes, "
                                     f"{'residual only' if o.residual_only else 'full'}")
        ctx.force_zchunk(RES3, 0)
        check_bits(full.run(), W, f"{tag}: defaults restored")
        check_bits(res.run(), R, f"{tag}: defaults restored (residual only)")


# ---- 3-D overlay: the level lattices have plane counts of their own ------------------------------------------------------------
def test_overlay_level_lattices_at_the_shortest_and_longest_chunks():
    from test_gpu_overlay3d import refined_block_case

    c = refined_block_case((12, 10, 12), True)
    ctx = make_context(c)
    assert ctx.kernel_path == 3
    ctx.state_set_host(c.sol, c.old, c.oldold)
    full, res = Outputs(ctx, False), Outputs(ctx, True)
    W, R = full.run(), res.run()
    assert not any(bool(w.isnan().any()) for w in W + R)
    for k in (UU3, PHI4, RES3):
        for L in (RANGE[k][0], RANGE[k][1], 1000):  # 1000: clamped to each lattice's plane count
            ctx.force_zchunk(k, L)
            check_bits(full.run(), W, f"overlay, {NAME[k]} at {L} planes")
            check_bits(res.run(), R, f"overlay, {NAME[k]} at {L} planes (residual only)")
        ctx.force_zchunk(k, 0)
    ctx.close()
