"""The two-stage reductions of the device-side entries (csrc/pfm_reduce.h) at the sizes the parity tests never reach:

  * more than 256 block partials, so that threads of the second stage fold two of them (a 2-D box of 257 x 256 cells =
    257 blocks, a 3-D box of 41 x 40 x 41 cells = 263 blocks; 260 node blocks for the norms);
  * the tail of a wave and of a block (1, 63, 65 and 257 cells);
  * nothing to reduce (a mask of zeros, an empty face list).

Every entry is called twice and must repeat bitwise.  References and bounds are those of the entries' parity tests
(tests/test_gpu_postproc.py, tests/test_newton_sweeps.py, tests/test_gpu_adapt.py), with one exception.  On the 3-D box
the oracle's own sum is the less accurate one: oracle_api.functionals adds its 1.8e6 terms one after the other, and its
crack energy differs from math.fsum over its results on the 263 blocks of 256 cells by 6.27e-12 (relative; 8.9e-13 with
the mask, 1.8e-13 on the 2-D box; np.sum of the block results agrees with fsum to 8e-16).  The device result differs from
the oracle by 6.27e-12 there, before and after the reductions moved to pfm_reduce.h, i.e. it agrees with fsum.  The bound of
that case is ten times the reference's spread."""
import functools

import numpy as np
import pytest

import bench
import oracle_api as O
import postproc_ref as R
from cracks_amd import adapt as A
from cracks_amd import mesh as M
from cracks_amd.assembler import Context

pytestmark = pytest.mark.gpu

TOL = 1e-12        # functionals, phi error, load: |got - want| <= TOL max(1, |want|)
NORM_RTOL = 1e-13  # residual norms
FUNCTIONALS_TOL = {"3d_41x40x41": 6.3e-11}  # ten times the spread of the oracle's own sum (see above); TOL elsewhere

BOXES = {
    "2d_257x256": (2, (257, 256)),
    "3d_41x40x41": (3, (41, 40, 41)),
    "2d_1": (2, (1, 1)),
    "2d_63": (2, (63, 1)),
    "2d_65": (2, (65, 1)),
    "2d_257": (2, (257, 1)),
}


def err(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


class Case:
    def __init__(self, name):
        dim, n = BOXES[name]
        self.dim = dim
        self.mesh = mesh = M.box_mesh(dim, n, lo=-1.5, hi=1.5)
        self.lay = M.DofLayout(mesh.n_nodes, dim, blocked=(name != "2d_257x256"))
        x = mesh.coords
        u = np.stack([1e-3 * np.sin(x[:, c]) * x[:, (c + 1) % dim] for c in range(dim)], axis=1)
        self.phi = 0.5 + 0.5 * np.tanh(4.0 * np.abs(x[:, 1]) - 0.3)
        self.sol = self.lay.pack(u, self.phi)
        rng = np.random.default_rng(11)
        self.mask = (rng.random(mesh.n_cells) < 0.5).astype(np.uint8)
        self.zeros = np.zeros(mesh.n_cells, np.uint8)
        self.node_flags = (rng.integers(0, 1 << (dim + 1), mesh.n_nodes) * (rng.random(mesh.n_nodes) < 0.3)).astype(np.uint8)
        self.prm = bench.sneddon_params(mesh.min_cell_diameter(), dim)
        self.ctx = Context(mesh, self.lay.blocked)
        self.ctx.set_params(self.prm)
        self.ctx.set_constraints(self.node_flags)
        self.ctx.state_set_host(self.sol, self.sol, self.sol)

    def masks(self):
        return (None, self.mask) if self.mesh.n_cells > 1 else (None,)


@functools.lru_cache(maxsize=None)
def case_of(name):
    return Case(name)


def twice(fn):
    """the result of fn(), which a second call must repeat bitwise"""
    first, again = fn(), fn()
    for a, b in zip(first, again) if isinstance(first, tuple) else [(first, again)]:
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (first, again)
    return first


@pytest.mark.parametrize("name", list(BOXES))
def test_functionals(name):
    c = case_of(name)
    for mask in c.masks():
        got = twice(lambda: c.ctx.functionals(mask))
        want = O.functionals(c.mesh, c.lay, c.prm, c.sol, None, None, mask)
        print(name, "functionals", got, want, err(got, want))
        assert err(got, want) <= FUNCTIONALS_TOL.get(name, TOL), (got, want)


@pytest.mark.parametrize("name", list(BOXES))
def test_sneddon_phi_error(name):
    c = case_of(name)
    for mask in c.masks():
        got = twice(lambda: c.ctx.sneddon_phi_error_sq(mask))
        want = R.sneddon_phi_error_sq(c.mesh, c.lay, c.sol, c.prm.alpha_eps, mask)
        print(name, "phi error", got, want, err(got, want))
        assert err(got, want) <= TOL, (got, want)


@pytest.mark.parametrize("name", list(BOXES))
def test_face_load(name):
    """one (cell, face) pair per cell: as many blocks as the cell-wise entries have"""
    c = case_of(name)
    cells = np.arange(c.mesh.n_cells, dtype=np.int32)
    faces = (cells % (2 * c.dim)).astype(np.uint8)
    got = twice(lambda: c.ctx.face_load(cells, faces))
    want = R.face_load(c.mesh, c.lay, c.sol, c.prm.lambda_, c.prm.mu, cells, faces)
    print(name, "face load", got, want, err(got, want))
    assert got.shape == (c.dim,) and err(got, want) <= TOL, (got, want)


@pytest.mark.parametrize("name", list(BOXES))
def test_min_cell_diameter(name):
    c = case_of(name)
    for mask in c.masks():
        got = twice(lambda: c.ctx.min_cell_diameter(mask))
        assert got == A.min_cell_diameter_numpy(c.mesh, mask)


@pytest.mark.parametrize("name", list(BOXES))
def test_refine_flags(name):
    c = case_of(name)
    level = (np.arange(c.mesh.n_cells) % 3).astype(np.uint8)
    lo, hi = [-0.5, -np.inf, -np.inf][:c.dim], [0.7, np.inf, 0.1][:c.dim]
    crits = [dict(phi_threshold=0.8), dict(phi_threshold=2.0), dict(box_lo=lo, box_hi=hi),
             dict(phi_threshold=0.8, box_lo=lo, box_hi=hi, max_level=1, cell_level=level)]
    assert c.ctx.refine_flags(phi_threshold=2.0)[1] == c.mesh.n_cells  # every cell is counted, the tail of the last block included
    n_total = 0
    for mask in c.masks():
        for crit in crits:
            flags, n = twice(lambda: c.ctx.refine_flags(cell_owned=mask, **crit))
            want, n_want = A.refine_flags_numpy(c.mesh, c.phi, cell_owned=mask, **crit)
            assert np.array_equal(flags, want) and n == n_want
            n_total += n
    assert n_total > 0


@pytest.mark.parametrize("name", list(BOXES))
def test_residual_norms(name):
    import torch

    c = case_of(name)
    rng = np.random.default_rng(7)
    n = c.lay.n_dofs
    r = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
    d = torch.from_numpy(r).to("cuda")
    torch.cuda.synchronize()
    l2, linf, sq = twice(lambda: c.ctx.residual_norms(d.data_ptr()))
    z = r.copy()
    nodes = np.arange(c.mesh.n_nodes)
    for comp in range(c.dim + 1):
        z[c.lay.dof(nodes[(c.node_flags >> comp) & 1 != 0], comp)] = 0.0
    assert 0 < np.count_nonzero(z) <= n
    print(name, "norms", l2, np.linalg.norm(z), sq, float(z @ z))
    assert l2 == pytest.approx(np.linalg.norm(z), rel=NORM_RTOL)
    assert linf == np.abs(z).max()
    assert sq == pytest.approx(float(z @ z), rel=NORM_RTOL)


@pytest.mark.parametrize("name", list(BOXES))
def test_nothing_to_reduce(name):
    c = case_of(name)
    assert twice(lambda: c.ctx.functionals(c.zeros)) == (0.0, 0.0, 0.0)
    assert twice(lambda: c.ctx.sneddon_phi_error_sq(c.zeros)) == 0.0
    flags, n = twice(lambda: c.ctx.refine_flags(phi_threshold=2.0, cell_owned=c.zeros))
    assert n == 0 and not flags.any()
    assert twice(lambda: c.ctx.min_cell_diameter(c.zeros)) == np.inf
    none = np.zeros(0, np.int32)
    assert np.array_equal(twice(lambda: c.ctx.face_load(none, none.astype(np.uint8))), np.zeros(c.dim))
