"""The kept (u,u) block (pfm_values_keep_uu_block): with the caller's promise that nothing but the library writes
d_values[0], the pair of a 3-D box leaves that block alone while old_solution, old_old_solution, the displacement bits of
the constraints and the parameters are what they were when it was written.  Results are the same whether the block was
just written or kept: the four value blocks keep the bits of an assembly without the promise; the displacement rows of the
residual come from the quadrature kernel in every assembly under the promise (the rows of PFM_RES_KERNEL=1, bit for bit).

The box is the one of tests/test_gpu_uu3_stream.py, 18 x 10 x 7 nodes: several tiles, regular and face copy-outs, u = 0 on
the boundary and one flagged node inside the regular tile.  Bar against the CPU oracle: gpu_util.TOL.  "bits": int64
views, array_equal.  "NaN probe": the kept array is overwritten with NaN behind the library's back (which breaks the
promise on purpose); an assembly that keeps the block leaves every NaN, one that writes it leaves none.
"""
import copy
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from cracks_amd import capi
from cracks_amd import mesh as M
from cracks_amd.assembler import Context, node_flags_from_dof_flags
from gpu_util import TOL, linf_scaled, make_context, oracle
from test_gpu_cart import box_case
from test_gpu_keep_up_block import _all, _bits, _oracle_bar, _same
from test_gpu_overlay3d import refined_block_case
from test_gpu_uu3_stream import FLAGGED, NX, NY, make_case

pytestmark = pytest.mark.gpu
UU3 = Context.ZC_UU3
INTERIOR = 11 + NX * (6 + NY * 3)  # node (11, 6, 3): no boundary node, not the flagged one


def _with(c, **kw):
    d = copy.copy(c)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@functools.lru_cache(maxsize=None)
def _base():
    return make_case("flagged")


def _solution(k):
    """three different `solution` vectors (the case's own, then two perturbations of every dof)"""
    c = _base()
    if k == 0:
        return c.sol
    rng = np.random.default_rng(100 + k)
    return c.sol + 0.05 * rng.standard_normal(c.sol.size)


def _reference(c):
    """the oracle's Jacobian and residual of a case (callers cache what they share)"""
    r, rp, ci = oracle(c, False)
    return sp.csr_matrix((r.values, ci, rp), shape=(c.layout.n_dofs,) * 2), r.residual_pde


@functools.lru_cache(maxsize=None)
def _reference_of_solution(k):
    return _reference(_with(_base(), sol=_solution(k)))


class Run:
    """One context with explicit device arrays: the four value blocks, the residual and the three state vectors."""

    def __init__(self, c, promise, ctx=None):
        import torch

        self.torch, self.c = torch, c
        self.ctx = ctx if ctx is not None else make_context(c)
        self.vals = [torch.empty(max(self.ctx.pattern_size(b)[1], 1), dtype=torch.float64, device="cuda")[:self.ctx.pattern_size(b)[1]]
                     for b in range(self.ctx.n_blocks)]
        self.res = torch.empty(self.ctx.n_owned_dofs, dtype=torch.float64, device="cuda")
        self.vec = [torch.zeros(self.ctx.n_owned_dofs, dtype=torch.float64, device="cuda") for _ in range(3)]
        if promise:
            self.ctx.values_keep_uu_block(self.uu)
            assert self.ctx.values_uu_block_kept() == self.uu
        self.state(c.sol, c.old, c.oldold)

    @property
    def uu(self):
        return self.vals[0].data_ptr()

    def state(self, sol=None, old=None, oldold=None):
        """pfm_state_set with device vectors; None: the vector as it was"""
        for t, a in zip(self.vec, (sol, old, oldold)):
            if a is not None:
                t.copy_(self.torch.from_numpy(np.ascontiguousarray(a, np.float64)))
        self.torch.cuda.synchronize()
        self.ctx.state_set_device(*[t.data_ptr() for t in self.vec])
        return self

    def assemble(self, vals=None):
        self.torch.cuda.synchronize()  # fills and copies ran on torch's stream
        vals = self.vals if vals is None else vals
        self.ctx.assemble_device(False, [v.data_ptr() for v in vals], self.res.data_ptr(), 0)
        self.ctx.sync_status()
        return [_bits(v) for v in vals], _bits(self.res)

    def poison(self):
        self.vals[0].fill_(float("nan"))
        return self

    def close(self):
        self.ctx.close()


def _nan_count(out):
    return int(np.isnan(out[0][0].view(np.float64)).sum())


def _kept(out, what):
    n = out[0][0].size
    assert _nan_count(out) == n, f"{what}: the block was written ({n - _nan_count(out)} of {n} entries)"


def _written(out, what):
    assert _nan_count(out) == 0, f"{what}: {_nan_count(out)} entries of the block were not written"


def _twins(c):
    """a context under the promise and one without, through the same calls"""
    return Run(c, True), Run(c, False)


CHILD = """
import sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import test_gpu_keep_uu_block as T
run = T.Run(T._base(), False)
out = {{}}
for k in range(3):
    out[f"res{{k}}"] = run.state(sol=T._solution(k)).assemble()[1]
np.savez(sys.argv[1], **out)
"""


# ---------------------------------------------------------------- 1
def test_three_assemblies_against_the_ignored_promise(tmp_path, monkeypatch):
    """Three `solution` vectors, then the first again.  Under the promise: assembly 0 writes the block, 1 to 3 keep it.
    The twin holds the same promise and runs with PFM_NO_KEEP_UU_BLOCK=1 (the parent's form)."""
    c = _base()
    kept, plain = Run(c, True), Run(c, True)
    n_u = 3 * c.mesh.n_nodes
    script, path = tmp_path / "run.py", tmp_path / "out.npz"
    here = os.path.dirname(os.path.abspath(__file__))
    script.write_text(CHILD.format(root=os.path.dirname(here), tests=here))
    subprocess.run([sys.executable, str(script), str(path)], check=True, env=dict(os.environ, PFM_RES_KERNEL="1"), timeout=300)
    quadrature = np.load(path)
    first = None
    for step, k in enumerate((0, 1, 2, 0)):
        sol = _solution(k)
        got = kept.state(sol=sol).assemble()
        monkeypatch.setenv("PFM_NO_KEEP_UU_BLOCK", "1")  # per call
        want = plain.state(sol=sol).assemble()
        monkeypatch.delenv("PFM_NO_KEEP_UU_BLOCK")
        for b in range(4):
            assert np.array_equal(got[0][b], want[0][b]), f"assembly {step}: block {b} differs from the form without the promise"
        A_ref, res_ref = _reference_of_solution(k)
        _oracle_bar(kept.ctx, _with(c, sol=sol), got, A_ref, res_ref, f"assembly {step} under the promise")
        r, q = got[1].view(np.float64), quadrature[f"res{k}"].view(np.float64)
        print(f"assembly {step}: |R_u - R_u(row identity)|_inf scaled = {linf_scaled(r[:n_u], want[1].view(np.float64)[:n_u]):.2e}")
        assert np.array_equal(got[1][:n_u], quadrature[f"res{k}"][:n_u]), f"assembly {step}: u rows are not those of PFM_RES_KERNEL=1"
        assert np.array_equal(got[1][n_u:], want[1][n_u:]), f"assembly {step}: phase-field rows differ from the form without the promise"
        assert not np.isnan(r).any() and not np.isnan(q).any()
        if step == 0:
            first = got
    _same(got, first, "the first solution again")
    kept.close(), plain.close()


# ---------------------------------------------------------------- 2
def test_the_skip_happens_and_is_exact():
    c = _base()
    run = Run(c, True)
    _written(run.poison().assemble(), "first assembly")
    _kept(run.poison().state(sol=_solution(1)).assemble(), "another solution only")
    _kept(run.state(sol=_solution(2)).assemble(), "a third solution")
    cur = _with(c, sol=_solution(2), old=c.old.copy(), oldold=c.oldold.copy())
    phi = c.layout.dof(np.array([INTERIOR]), 3)[0]
    for name, value in (("old", 0.37), ("oldold", 0.61), ("old", 0.0), ("old", -0.0)):
        vec = getattr(cur, name)
        minus_zero = value == 0.0 and np.signbit(value)
        assert minus_zero or vec[phi] != value
        vec[phi] = value
        out = run.poison().state(**{name: vec}).assemble()
        _written(out, f"{name}[{INTERIOR}] = {value!r}")
        A_ref, res_ref = _reference(cur)
        _oracle_bar(run.ctx, cur, out, A_ref, res_ref, f"{name}[{INTERIOR}] = {value!r}")
        _kept(run.poison().state(**{name: vec}).assemble(), f"the same {name} again")
    run.close()


# ---------------------------------------------------------------- 3
def test_constraint_changes():
    c = _base()
    run = Run(c, True)
    flags = node_flags_from_dof_flags(c.layout, c.cu.flag, c.ch.flag)
    _written(run.poison().assemble(), "first assembly")
    active = flags.copy()
    active[::3] ^= 0x8  # an active-set update: the phase-field bit of every third node
    run.ctx.set_constraints(active)
    _kept(run.poison().assemble(), "flags changed in the phase-field bit only")
    run.ctx.set_constraints(flags)
    _kept(run.assemble(), "... and back")
    extra = int(c.layout.dof(np.array([INTERIOR]), 1)[0])
    cu = M.update_constraints(c.mesh, c.layout, np.union1d(np.nonzero(c.cu.flag)[0], [extra]))
    c2 = _with(c, cu=cu)
    flags2 = node_flags_from_dof_flags(c.layout, cu.flag, c.ch.flag)
    assert np.count_nonzero(flags2 != flags) == 1 and (flags2[INTERIOR] ^ flags[INTERIOR]) == 0x2
    run.ctx.set_constraints(flags2)
    out = run.poison().assemble()
    _written(out, "one displacement bit changed")
    A_ref, res_ref = _reference(c2)
    _oracle_bar(run.ctx, c2, out, A_ref, res_ref, "one displacement bit changed")
    run.close()


# ---------------------------------------------------------------- 4
def _params(c, **kw):
    p = type(c.params).from_buffer_copy(bytes(c.params))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_parameter_and_setup_changes():
    c = _base()
    kept, twin = _twins(c)
    _written(kept.poison().assemble(), "first assembly")
    kept.ctx.set_params(_params(c))
    _kept(kept.poison().assemble(), "pfm_set_params with identical bytes")
    pats = [kept.ctx.pattern(b) for b in range(4)]

    def bind(x):
        for b, (rp, ci) in enumerate(pats):
            x.pattern_bind(b, rp, ci)

    steps = [("timestep", lambda x: x.set_params(_params(c, timestep=0.5 * c.params.timestep))),
             ("lambda_", lambda x: x.set_params(_params(c, timestep=0.5 * c.params.timestep, lambda_=1.25 * c.params.lambda_))),
             ("pfm_pattern_bind", bind), ("pfm_set_split_route", lambda x: x.set_split_route(capi.SPLIT_ROUTE_LATTICE)),
             ("pfm_ctx_force_path", lambda x: x.force_path(1))]
    last = None
    for name, step in steps:
        step(kept.ctx), step(twin.ctx)
        out = kept.poison().assemble()
        _written(out, name)
        want = twin.assemble()
        _same((out[0], want[1]), want, name)  # (the four blocks; the u rows of the residual are another form's)
        if last is not None and name in ("timestep", "lambda_"):
            assert not np.array_equal(out[0][0], last[0][0]), f"{name} does not change the block: the case proves nothing"
        last = out
        _kept(kept.poison().assemble(), f"{name}: the next assembly")
    for planes in (2, 3):
        kept.ctx.force_zchunk(UU3, planes), twin.ctx.force_zchunk(UU3, planes)
        for k in (1, 2):  # written or kept, whichever the library chooses: the values are those of the twin
            sol = _solution(k)
            out, want = kept.state(sol=sol).assemble(), twin.state(sol=sol).assemble()
            _same((out[0], want[1]), want, f"chunks of {planes} planes, solution {k}")
    kept.close(), twin.close()


# ---------------------------------------------------------------- 5
def test_patches_on_a_kept_block():
    """kappa = 0 and phi_old = phi_oldold = 0 on the node planes x = 0 and x = 1: the element matrices of the cell layer at
    the flagged face x = 0 vanish in (u,u), their constrained diagonals get the placeholder of k_cart_phi4, which follows
    `solution` and is ADDED behind the join -- on a kept block to the value under the patch, not to the last sum."""
    c0 = _base()
    lay = c0.layout
    layer = np.nonzero(c0.mesh.coords[:, 0] < c0.mesh.coords[:, 0].min() + 1.5 * (20.0 / 17))[0]
    assert layer.size == 2 * 10 * 7
    old, oldold = c0.old.copy(), c0.oldold.copy()
    old[lay.dof(layer, 3)] = 0.0
    oldold[lay.dof(layer, 3)] = 0.0
    c = _with(c0, old=old, oldold=oldold, params=_params(c0, constant_k=0.0))
    kept, twin = _twins(c)
    outs = []
    for step, k in enumerate((0, 1, 2)):
        sol = _solution(k)
        out = kept.state(sol=sol).assemble()
        want = twin.state(sol=sol).assemble()
        bad = np.nonzero(out[0][0] != want[0][0])[0]
        assert bad.size == 0, f"assembly {step}: {bad.size} (u,u) entries differ from the block just written, first at {bad[:8]}"
        _same((out[0], want[1]), want, f"assembly {step}")
        ck = _with(c, sol=sol)
        A_ref, res_ref = _reference(ck)
        _oracle_bar(kept.ctx, ck, out, A_ref, res_ref, f"patches, assembly {step}")
        outs.append(out)
    changed = np.nonzero(outs[0][0][0] != outs[1][0][0])[0]
    print(f"(u,u) entries that follow the solution (patched diagonals): {changed.size}")
    assert changed.size > 0, "no patched diagonal: the case proves nothing"
    # NaN probe: the block is kept -- but for the patched entries, which are put back and patched again
    out = kept.poison().state(sol=_solution(0)).assemble()
    there = ~np.isnan(out[0][0].view(np.float64))
    flagged_u = int(np.count_nonzero(c.cu.flag[: 3 * c.mesh.n_nodes]))
    assert changed.size <= there.sum() <= flagged_u, f"{there.sum()} entries written, {changed.size} patched, {flagged_u} flagged dofs"
    assert np.array_equal(out[0][0][there], outs[0][0][0][there])
    kept.close(), twin.close()


# ---------------------------------------------------------------- 6
def test_scope_pointers():
    import torch

    c = _base()
    run = Run(c, True)
    _written(run.poison().assemble(), "first assembly")
    other = [torch.full_like(v, float("nan")) for v in run.vals]
    out = run.assemble(other)
    _written(out, "another d_values[0]")
    assert run.ctx.values_uu_block_kept() == run.uu
    _kept(run.poison().assemble(), "the kept array after an assembly into another one")
    run.ctx.values_release_uu_block()
    assert run.ctx.values_uu_block_kept() == 0
    _written(run.poison().assemble(), "withdrawn")
    _written(run.poison().assemble(), "withdrawn, again")
    run.ctx.values_keep_uu_block(run.uu)
    run.ctx.close()  # with a promise held
    il = Context(c.mesh, False)
    for call in (lambda: il.values_keep_uu_block(run.uu), il.values_release_uu_block):
        with pytest.raises(capi.PfmError) as e:
            call()
        assert e.value.status == 1  # PFM_ERR_BAD_ARG
    assert il.values_uu_block_kept() == 0
    il.close()


def _peers(ctx):
    ctx.halo_register([0, 1], [0], [0, 0], [])  # one peer that takes node 0 and sends nothing


SCOPE = {
    "monolithic": (lambda: box_case(3, (17, 9, 6), -10.0, 10.0, True, monolithic=True), 1, None),
    "peers": (_base, 1, _peers),
    "overlay": (lambda: refined_block_case((12, 12, 12), True), 3, None),
    "2d_24x24": (lambda: box_case(2, (24, 24), -10.0, 10.0, True), 1, None),
}


@pytest.mark.parametrize("name", list(SCOPE))
def test_scope_accepted_and_ignored(name):
    maker, path, setup = SCOPE[name]
    c = maker()
    ctx = make_context(c)
    assert ctx.kernel_path == path and ctx.n_blocks == 4
    if setup:
        setup(ctx)
    run = Run(c, True, ctx)
    assert ctx.values_uu_block_kept() == run.uu
    first = run.poison().assemble()
    _written(first, f"{name}: first assembly")
    for k in range(2):
        out = run.poison().assemble()
        _written(out, f"{name}: assembly {k + 1} of the same state")
        if name != "overlay":  # (the general family of an overlay adds with atomics)
            _same(out, first, f"{name}: assembly {k + 1}")
    run.close()


# ---------------------------------------------------------------- 7
def test_the_assembler_gives_both_promises_for_its_own_matrix():
    from cracks_amd.assembler import Assembler

    c = _base()
    A_ref, res_ref = _reference_of_solution(0)
    a = Assembler(c.mesh, blocked=True)
    a.set_params(c.params)
    a.set_constraints(node_flags_from_dof_flags(c.layout, c.cu.flag, c.ch.flag))
    a.set_vectors(c.sol, c.old, c.oldold)
    assert a.ctx.values_uu_block_kept() == 0 and a.ctx.values_up_block_kept() == 0
    for k in range(2):
        a.assemble_system(False)
        a.synchronize()
        assert a.ctx.values_uu_block_kept() == a.system_pde_matrix[0].data_ptr() != 0
        assert a.ctx.values_up_block_kept() == a.system_pde_matrix[1].data_ptr() != 0
        out = ([_bits(m) for m in a.system_pde_matrix], _bits(a.system_pde_residual))
        _oracle_bar(a.ctx, c, out, A_ref, res_ref, f"assembler, assembly {k}")
    a.system_pde_matrix[0].fill_(float("nan"))
    a.assemble_system(False)
    a.synchronize()
    assert bool(a.system_pde_matrix[0].isnan().all()), "the assembler's own matrix is not kept"
    a.system_pde_matrix = None
    assert a.ctx.values_uu_block_kept() == 0 and a.ctx.values_up_block_kept() == 0
    b = Assembler(c.mesh, blocked=True)
    b.allocate_matrix()
    assert b.ctx.values_uu_block_kept() == 0 and b.ctx.values_up_block_kept() == 0
    a.ctx.close(), b.ctx.close()
