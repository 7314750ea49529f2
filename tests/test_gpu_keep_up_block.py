"""The kept (u,phi) block (pfm_values_keep_up_block): with the caller's promise that nothing but the library writes
d_values[1], an assembly into that pointer leaves the structurally zero block alone -- no store of k_cart_phi4,
k_cart_split3_jac or k_cart2d_cells, no fill, no memset -- and every other output keeps its bits.

Shapes (cells; k_cart_phi4 tiles are 7 x 7 nodes): (22, 22, 4) interior, face and partial tiles; (22, 22, 9) with forced
z-chunks of 2 and 3 planes and the default, several consecutive fast planes in a chunk and chunk seams; (8, 4, 2) only
generic copy-outs; a 2-D box of 24^2; the refined block of tests/test_gpu_overlay3d.py for the level lattices.  Each with
Dirichlet faces flagged and without flags.  Bar against the CPU oracle: gpu_util.TOL; "bits": int64 views, array_equal."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

from cracks_amd import capi
from cracks_amd import mesh as M
from cracks_amd.assembler import Context, node_flags_from_dof_flags
from gpu_util import TOL, blocks_to_global, linf_scaled, make_context, oracle, reference_parity
from test_gpu_cart import box_case
from test_gpu_overlay3d import refined_block_case
from test_gpu_pattern import _permuted_patterns

pytestmark = pytest.mark.gpu

SENT = 7.0
PHI4 = Context.ZC_PHI4
# name -> (dim, maker, z-chunk of k_cart_phi4 (None: not forced), kernel path)
SHAPES = {
    "22x22x4": (3, lambda: box_case(3, (22, 22, 4), -10.0, 10.0, True), None, 1),
    "22x22x9_zc2": (3, lambda: box_case(3, (22, 22, 9), -10.0, 10.0, True), 2, 1),
    "22x22x9_zc3": (3, lambda: box_case(3, (22, 22, 9), -10.0, 10.0, True), 3, 1),
    "22x22x9": (3, lambda: box_case(3, (22, 22, 9), -10.0, 10.0, True), 0, 1),
    "8x4x2": (3, lambda: box_case(3, (8, 4, 2), -10.0, 10.0, True), None, 1),
    "2d_24x24": (2, lambda: box_case(2, (24, 24), -10.0, 10.0, True), None, 1),
    "overlay": (3, lambda: refined_block_case((12, 12, 12), True), None, 3),
}
BOXES_3D = ["22x22x4", "22x22x9_zc2", "22x22x9_zc3", "22x22x9", "8x4x2"]
FLAGGED = pytest.mark.parametrize("flagged", [True, False], ids=["dirichlet_faces", "no_flags"])


@functools.lru_cache(maxsize=None)
def _case(shape, flagged):
    """The case and its oracle Jacobian and residual, computed once and shared (nobody changes them)."""
    c = SHAPES[shape][1]()
    if not flagged:
        c.cu = M.update_constraints(c.mesh, c.layout, [])
    r, rp, ci = oracle(c, False)
    return c, sp.csr_matrix((r.values, ci, rp), shape=(c.layout.n_dofs,) * 2), r.residual_pde


def _context(shape, flagged, bound=False):
    c, A_ref, res_ref = _case(shape, flagged)
    dim, _, zc, path = SHAPES[shape]
    ctx = make_context(c)
    assert ctx.kernel_path == path and ctx.n_blocks == 4
    if zc is not None:
        ctx.force_zchunk(PHI4, zc)
    if bound:
        for b, (rp, ci, _) in enumerate(_permuted_patterns(ctx, dim, True, seed=11)):
            ctx.pattern_bind(b, rp, ci)
    ctx.state_set_host(c.sol, c.old, c.oldold)
    return ctx, c, A_ref, res_ref


class Outputs:
    """The four value blocks and the residual of one context on the device."""

    def __init__(self, ctx):
        import torch

        self.ctx = ctx
        self.vals = [torch.empty(ctx.pattern_size(b)[1], dtype=torch.float64, device="cuda") for b in range(4)]
        self.res = torch.empty(ctx.n_owned_dofs, dtype=torch.float64, device="cuda")

    @property
    def up(self):
        return self.vals[1].data_ptr()

    def fill(self, value, blocks=(0, 1, 2, 3)):
        for b in blocks:
            self.vals[b].fill_(value)
        self.res.fill_(value)
        return self

    def assemble(self):
        import torch

        torch.cuda.synchronize()  # the fills ran on torch's stream
        self.ctx.assemble_device(False, [v.data_ptr() for v in self.vals], self.res.data_ptr(), 0)
        self.ctx.sync_status()
        return [_bits(v) for v in self.vals], _bits(self.res)


def _bits(t):
    return t.cpu().numpy().view(np.int64)


def _same(a, b, what, blocks=(0, 1, 2, 3)):
    for k in blocks:
        bad = np.nonzero(a[0][k] != b[0][k])[0]
        assert bad.size == 0, f"{what}: block {k}: {bad.size} of {a[0][k].size} entries differ, first at {bad[:8]}"
    assert np.array_equal(a[1], b[1]), f"{what}: residual"


def _all(bits, value, what):
    want = np.float64(value).view(np.int64)
    bad = np.nonzero(bits != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {bits.size} entries are not {value!r}, first at {bad[:8]}: {bits[bad[:4]].view(np.float64)}"


def _oracle_bar(ctx, c, out, A_ref, res_ref, tag):
    vals, res = [b.view(np.float64) for b in out[0]], out[1].view(np.float64)
    assert not any(np.isnan(v).any() for v in vals) and not np.isnan(res).any(), f"{tag}: an output was not written"
    A = blocks_to_global(ctx, c.layout, [v.copy() for v in vals])
    A.sort_indices()
    assert (A.indptr == A_ref.indptr).all() and (A.indices == A_ref.indices).all()
    e_mat, e_res = linf_scaled(A.data, A_ref.data), linf_scaled(res, res_ref)
    print(f"{tag}: |dA|_inf = {e_mat:.2e}, |dR|_inf = {e_res:.2e}")
    assert e_mat < TOL and e_res < TOL
    reference_parity(c.layout, c.sol, A, A_ref, [(res, res_ref, "pde")], tag=tag)


def _unkept_then_kept(shape, flagged, bound):
    """The reference run without a promise (held to the oracle bar), then the promise on a NaN-filled block 1."""
    ctx, c, A_ref, res_ref = _context(shape, flagged, bound)
    o = Outputs(ctx)
    assert ctx.values_up_block_kept() == 0
    ref = o.fill(np.nan).assemble()
    _oracle_bar(ctx, c, ref, A_ref, res_ref, f"{shape} unkept")
    _all(ref[0][1], 0.0, "unkept block 1")
    o.fill(np.nan)
    ctx.values_keep_up_block(o.up)
    assert ctx.values_up_block_kept() == o.up
    _all(_bits(o.vals[1]), 0.0, "block 1 right after the promise")
    return ctx, o, ref


# ---------------------------------------------------------------- 1
@FLAGGED
@pytest.mark.parametrize("bound", [False, True], ids=["canonical", "bound_pattern"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kept_equals_unkept(shape, bound, flagged):
    ctx, o, ref = _unkept_then_kept(shape, flagged, bound)
    for k in range(2):
        got = o.fill(np.nan, blocks=(0, 2, 3)).assemble()
        _all(got[0][1], 0.0, f"kept block 1, assembly {k}")
        _same(got, ref, f"{shape} kept against unkept, assembly {k}", blocks=(0, 2, 3))
    ctx.close()


# ---------------------------------------------------------------- 2
@FLAGGED
@pytest.mark.parametrize("shape,bound", [(s, b) for s in BOXES_3D for b in (False, True)] + [("2d_24x24", False)],
                         ids=lambda v: v if isinstance(v, str) else ("bound_pattern" if v else "canonical"))
def test_the_stores_are_gone(shape, bound, flagged, monkeypatch):
    ctx, o, ref = _unkept_then_kept(shape, flagged, bound)
    o.fill(np.nan, blocks=(0, 2, 3)).vals[1].fill_(SENT)
    got = o.assemble()
    _all(got[0][1], SENT, "sentinel in a kept block")
    _same(got, ref, f"{shape} kept, sentinel in block 1", blocks=(0, 2, 3))
    monkeypatch.setenv("PFM_NO_KEEP_UP_BLOCK", "1")  # per call
    got = o.assemble()
    monkeypatch.delenv("PFM_NO_KEEP_UP_BLOCK")
    _same(got, ref, f"{shape} PFM_NO_KEEP_UP_BLOCK=1")
    assert ctx.values_up_block_kept() == o.up
    ctx.close()


def _split_params(c):
    p = type(c.params).from_buffer_copy(bytes(c.params))
    p.decompose_stress_matrix, p.decompose_stress_rhs, p.timestep_number = 1.0, 1.0, 1
    return p


@FLAGGED
def test_the_stores_are_gone_under_split_route_5(flagged, monkeypatch):
    c, _, _ = _case("22x22x4", flagged)
    ctx = Context(c.mesh, True)
    ctx.set_split_model(capi.SPLIT_VOLDEV)
    ctx.set_split_route(capi.SPLIT_ROUTE_LATTICE_JACOBIAN)
    ctx.set_params(_split_params(c))
    ctx.set_constraints(node_flags_from_dof_flags(c.layout, c.cu.flag, c.ch.flag))
    ctx.state_set_host(c.sol, c.old, c.oldold)
    assert ctx.split_route_plan()[:3] == (5, 1, 1)
    o = Outputs(ctx)
    ref = o.fill(np.nan).assemble()
    assert not any(np.isnan(b.view(np.float64)).any() for b in ref[0])
    _all(ref[0][1], 0.0, "unkept block 1")
    ctx.values_keep_up_block(o.up)
    o.fill(np.nan, blocks=(0, 2, 3)).vals[1].fill_(SENT)
    got = o.assemble()
    _all(got[0][1], SENT, "sentinel in a kept block, route 5")
    _same(got, ref, "route 5 kept", blocks=(0, 2, 3))
    monkeypatch.setenv("PFM_NO_KEEP_UP_BLOCK", "1")
    got = o.assemble()
    monkeypatch.delenv("PFM_NO_KEEP_UP_BLOCK")
    _same(got, ref, "route 5, PFM_NO_KEEP_UP_BLOCK=1")
    ctx.close()


# ---------------------------------------------------------------- 3
@FLAGGED
@pytest.mark.parametrize("shape", ["22x22x4", "2d_24x24", "overlay"])
def test_withdrawn_and_foreign_pointers(shape, flagged):
    ctx, a, ref = _unkept_then_kept(shape, flagged, False)
    # a foreign array while the promise on A stands: written in full
    b = Outputs(ctx)
    got = b.fill(np.nan).assemble()
    _same(got, ref, "foreign array B")
    assert ctx.values_up_block_kept() == a.up
    if SHAPES[shape][3] == 1:  # (the row-owner kernels of a box; an overlay's general family may add its zeros)
        a.fill(np.nan, blocks=(0, 2, 3)).vals[1].fill_(SENT)
        got = a.assemble()
        _all(got[0][1], SENT, "sentinel in A after an assembly into B")
        _same(got, ref, "A after B", blocks=(0, 2, 3))
    # withdrawn: as without a promise
    ctx.values_release_up_block()
    assert ctx.values_up_block_kept() == 0
    got = a.fill(np.nan).assemble()
    _same(got, ref, "withdrawn")
    ctx.close()


# ---------------------------------------------------------------- 4
@FLAGGED
def test_living_context(flagged):
    """One context with the promise held throughout against a twin without, through the same sequence."""
    c, _, _ = _case("22x22x4", flagged)
    pair = []
    for _ in range(2):
        ctx = Context(c.mesh, True)
        ctx.set_split_model(capi.SPLIT_VOLDEV)
        ctx.set_params(c.params)
        ctx.set_constraints(node_flags_from_dof_flags(c.layout, c.cu.flag, c.ch.flag))
        ctx.state_set_host(c.sol, c.old, c.oldold)
        pair.append((ctx, Outputs(ctx)))
    (kept, ok), (twin, ot) = pair
    kept.values_keep_up_block(ok.up)
    other = np.zeros(c.mesh.n_nodes, np.uint8)
    other[::3] = 0x8  # an active set on every third node
    other[1::7] |= 0x3
    pats = _permuted_patterns(kept, 3, True, seed=5)

    def bind(x):
        for b, (rp, ci, _) in enumerate(pats):
            x.pattern_bind(b, rp, ci)

    steps = [("default", lambda x: None), ("force_path(0)", lambda x: x.force_path(0)), ("force_path(2)", lambda x: x.force_path(2)),
             ("force_path(1)", lambda x: x.force_path(1)),
             ("model 3, route 0", lambda x: x.set_params(_split_params(c))),
             ("model 3, route 5", lambda x: x.set_split_route(5)), ("model 3, route 21", lambda x: x.set_split_route(21)),
             ("unsplit, other flags", lambda x: (x.set_params(c.params), x.set_constraints(other))),
             ("pattern_bind", bind), ("force_phase(1)", lambda x: x.force_phase(1)), ("force_phase(2)", lambda x: x.force_phase(2)),
             ("force_phase(0)", lambda x: x.force_phase(0))]
    for name, step in steps:
        step(kept), step(twin)
        if name != "force_phase(2)":  # (the second half goes into the arrays of the first)
            ok.fill(np.nan, blocks=(0, 2, 3)), ot.fill(np.nan)
        got, want = ok.assemble(), ot.assemble()
        _all(got[0][1], 0.0, f"{name}: kept block 1")
        _same(got, want, name, blocks=(0, 2, 3))
        assert kept.values_up_block_kept() == ok.up, name
    assert not any(np.isnan(b.view(np.float64)).any() for b in want[0])
    kept.close(), twin.close()


# ---------------------------------------------------------------- 5
def test_arguments_and_lifetime():
    import torch

    c, _, _ = _case("8x4x2", True)
    il = Context(c.mesh, False)
    x = torch.zeros(8, dtype=torch.float64, device="cuda")
    for call in (lambda: il.values_keep_up_block(x.data_ptr()), il.values_release_up_block):
        with pytest.raises(capi.PfmError) as e:
            call()
        assert e.value.status == 1  # PFM_ERR_BAD_ARG: the interleaved layout has no such block
    assert il.values_up_block_kept() == 0
    il.close()
    ctx = make_context(c)
    o = Outputs(ctx).fill(SENT)
    ctx.values_keep_up_block(o.up)
    _all(_bits(o.vals[1]), 0.0, "keep")
    o.vals[1].fill_(SENT)
    torch.cuda.synchronize()
    ctx.values_keep_up_block(o.up)  # the same pointer again: cleared again
    _all(_bits(o.vals[1]), 0.0, "keep again")
    assert ctx.values_up_block_kept() == o.up
    ctx.values_release_up_block()
    ctx.values_release_up_block()
    assert ctx.values_up_block_kept() == 0
    ctx.values_keep_up_block(o.up)
    ctx.close()  # with a promise held


# ---------------------------------------------------------------- 6
def test_the_assembler_keeps_the_block_of_its_own_matrix():
    from cracks_amd.assembler import Assembler

    c, A_ref, res_ref = _case("22x22x4", True)
    a = Assembler(c.mesh, blocked=True)
    a.set_params(c.params)
    a.set_constraints(node_flags_from_dof_flags(c.layout, c.cu.flag, c.ch.flag))
    a.set_vectors(c.sol, c.old, c.oldold)
    assert a.ctx.values_up_block_kept() == 0
    a.assemble_system(False)
    a.synchronize()
    assert a.ctx.values_up_block_kept() == a.system_pde_matrix[1].data_ptr() != 0
    a.system_pde_matrix = None
    assert a.ctx.values_up_block_kept() == 0 and a.system_pde_matrix == []
    for _ in range(2):
        a.assemble_system(False)
        a.synchronize()
        assert a.ctx.values_up_block_kept() == a.system_pde_matrix[1].data_ptr() != 0
        out = ([_bits(m) for m in a.system_pde_matrix], _bits(a.system_pde_residual))
        _all(out[0][1], 0.0, "block 1 of the assembler's matrix")
        _oracle_bar(a.ctx, c, out, A_ref, res_ref, "assembler")
    # a caller who allocates the matrix itself has the tensors in hand before the first assembly: no promise
    b = Assembler(c.mesh, blocked=True)
    b.allocate_matrix()
    assert b.ctx.values_up_block_kept() == 0
    # ... and a promise the caller gave the context for an array of its own is neither replaced nor withdrawn by the assembler
    own = Outputs(b.ctx)
    b.ctx.values_keep_up_block(own.up)
    b.system_pde_matrix = None
    assert b.ctx.values_up_block_kept() == own.up
    b.set_params(c.params)
    b.set_constraints(node_flags_from_dof_flags(c.layout, c.cu.flag, c.ch.flag))
    b.set_vectors(c.sol, c.old, c.oldold)
    b.assemble_system(False)
    b.synchronize()
    assert b.ctx.values_up_block_kept() == own.up
    _all(_bits(b.system_pde_matrix[1]), 0.0, "block 1 of a matrix without a promise")
    b.system_pde_matrix = None
    assert b.ctx.values_up_block_kept() == own.up
    a.ctx.close(), b.ctx.close()


# ---------------------------------------------------------------- 7
@FLAGGED
def test_host_pointer_call(flagged):
    ctx, c, A_ref, res_ref = _context("22x22x4", flagged)
    ref = Outputs(ctx).fill(np.nan).assemble()
    for k in range(2):  # (the staging block is cleared when it is allocated, and kept)
        values = [np.full(ctx.pattern_size(b)[1], np.nan) for b in range(4)]
        res = np.full(ctx.n_owned_dofs, np.nan)
        ctx.assemble_host(c.sol, c.old, c.oldold, False, out=(values, res, None))
        got = ([v.view(np.int64) for v in values], res.view(np.int64))
        _all(got[0][1], 0.0, f"h_values[1], call {k}")
        _same(got, ref, f"host-pointer call {k} against the device path")
    assert ctx.values_up_block_kept() == 0  # the library's own staging is no promise of the caller's
    ctx.close()
