"""The states of the tests of the volumetric-deviatoric split Jacobian on the level lattices of a 3-D overlay
(PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS = 13 / _ALL_LEVELS = 15; tests/test_gpu_split_levels_jacobian.py) that
tests/split_lattice_cases.py does not have already, and a numpy copy of what makes a node a regular row of the overlay.
tests/test_split_levels_ref_cpu.py runs every input condition on the CPU, so a GPU test never fails on its input.

  LC.block_case(blocked)          the refined (8, 8, 8) block (960 cells, hanging nodes, Dirichlet faces, an active set, per-cell
                                  Lame), both layouts: 9^3 coarse and 9^3 fine lattice nodes plus halo
  big_block_case(active)          refined_block_case((12, 10, 12)), interleaved, the monolithic scheme with the penalty term and
                                  use_old_timestep_pf, per-cell Lame: a fine lattice of 13 x 9 x 13 nodes plus halo, so several
                                  8 x 4 tiles of k_cart_split3_jac in x and y on both levels.  active=False: no active set (the
                                  bound-pattern test: rows whose 27 neighbours are all free)
  one_sided_case(sign)            a dilation (+1) / compression (-1) of 1e-2 plus noise on the (8, 8, 8) block
  line_search_case()              the (8, 8, 8) block, blocked, active-set scheme (the state of the device line search)
  weights_case(d_mat, d_rhs)      LC.block_case() with decompose_stress_matrix != decompose_stress_rhs

References: split_jacobian_cases.Ref (split_voldev_ref.element_matrices), computed once per case (split_jacobian_cases.ref)."""
import functools

import numpy as np

import cases
import split_lattice_cases as LC
import split_voldev_cases as SC
from test_gpu_split3d import _copy, _params

BIG = (12, 10, 12)
BIG_SEED = {True: 54, False: 54}  # by `active`; chosen on the CPU among 52..65: share 0.501, margin 6.9e-6 (the displacement is the first draw)


def _block(n, blocked, active=True):
    from test_gpu_overlay3d import refined_block_case

    shape = refined_block_case(n, blocked, active=active)
    lines = lambda lay, rng: np.nonzero(shape.cu.flag.astype(bool) & ~shape.ch.flag.astype(bool))[0]
    return shape, lines


@functools.lru_cache(maxsize=None)
def big_block_case(active=True):
    shape, lines = _block(BIG, False, active)
    prm = _params(1.0, 1.0, outer_solver=1, gamma_penal=1e-2, use_old_timestep_pf=1)
    c = SC.mixed_case(f"levels/refined_block_12x10x12/{'active_set' if active else 'free'}", shape.mesh, False, prm, BIG_SEED[active], lines,
                      cell_lame=True)
    assert np.array_equal(c.cu.flag, shape.cu.flag) and c.ch.flag.any() and c.cell_lambda is not None and not c.layout.blocked
    return c


@functools.lru_cache(maxsize=None)
def one_sided_case(sign):
    shape, lines = _block((8, 8, 8), sign > 0)
    c = SC.mixed_case(f"levels/refined_block/{'tension' if sign > 0 else 'compression'}", shape.mesh, sign > 0,
                      _params(1.0, 1.0, outer_solver=1, gamma_penal=1e-2), 31, lines, cell_lame=True, grad=sign * SC.EXPAND, noise=2e-4)
    assert c.mesh.n_cells == 960 and c.ch.flag.any()
    return c


@functools.lru_cache(maxsize=None)
def line_search_case():
    shape, lines = _block((8, 8, 8), True)
    c = SC.mixed_case("levels/refined_block/line_search", shape.mesh, True, _params(), 70, lines, cell_lame=True)
    return c


@functools.lru_cache(maxsize=None)
def weights_case(d_mat, d_rhs):
    """LC.block_case() with decompose_stress_matrix != decompose_stress_rhs (split_jacobian_cases.WEIGHTS)"""
    c = LC.block_case()
    return cases.Case(f"levels/refined_block/weights/mat{d_mat}/rhs{d_rhs}", c.mesh, c.layout,
                      _copy(c.params, decompose_stress_matrix=d_mat, decompose_stress_rhs=d_rhs), c.sol, c.old, c.oldold, c.cu, c.ch, None,
                      c.cell_lambda, c.cell_mu)


def general_cells(mesh, regular):
    """the cells the general family keeps next to the overlay: those with a hanging vertex or an owned vertex that is no
    regular row (finish_patches3d)"""
    hanging = np.zeros(mesh.n_nodes, bool)
    hanging[np.asarray(mesh.hn_nodes, np.int64)] = True
    cells = np.asarray(mesh.cells, np.int64)
    return hanging[cells].any(axis=1) | (~regular[cells]).any(axis=1)


def rows_owning_a_cell(mesh, regular):
    """the regular rows that are the lowest vertex of a cell: the cells k_cart_split3_jac counts for pfm_ctx_split_route_info
    (a regular row on an upper face of the domain has no cell above it)"""
    cells = np.asarray(mesh.cells, np.int64)
    lowest = cells[np.arange(cells.shape[0]), np.argmin(mesh.coords[cells].sum(axis=2), axis=1)]
    return np.intersect1d(np.nonzero(regular)[0], lowest)


def regular_rows(mesh, n_owned=None):
    """What makes a node a regular row of the 3-D overlay (cracks_amd/csrc/pfm_mesh_plan.h), recomputed in numpy from the
    mesh (axis-parallel cells, one edge length per level along x): owned, not hanging, not a parent of a hanging node, every
    incident cell of one level and without a hanging vertex, and a cell at every one of the eight positions around the node
    that lies inside the box of that level's cells (a node on a face of that box has fewer: the face of a level that reaches
    the boundary of the domain).  Returns a bool array over the nodes.  The library drops a whole level with fewer than 64
    such rows (PFM_OVERLAY3_MIN_ROWS) -- not on the blocks used here: the GPU tests hold the count to overlay_info()[0]."""
    n = mesh.n_nodes
    owned = n if n_owned is None else n_owned
    cells = np.asarray(mesh.cells, np.int64)
    hanging = np.zeros(n, bool)
    hanging[np.asarray(mesh.hn_nodes, np.int64)] = True
    parent = np.zeros(n, bool)
    parent[np.unique(np.asarray(mesh.hn_parents, np.int64))] = True
    x = mesh.coords[cells]  # [cells, 8, 3]
    size = (x.max(axis=1) - x.min(axis=1))[:, 0]
    flat, rep = cells.ravel(), lambda a: np.repeat(a, 8)
    lo, hi = np.full(n, np.inf), np.zeros(n)
    np.minimum.at(lo, flat, rep(size))
    np.maximum.at(hi, flat, rep(size))
    touches_hanging = np.zeros(n, bool)
    np.logical_or.at(touches_hanging, flat, rep(hanging[cells].any(axis=1)))
    count = np.bincount(flat, minlength=n)
    one_level = count > 0
    one_level &= hi - lo <= 1e-9 * np.where(one_level, lo, 1.0)
    want = np.zeros(n, np.int64)
    for s in np.unique(np.round(size, 9)):  # per level: the box of its cells
        of = np.abs(size - s) <= 1e-9 * s
        bx = x[of].reshape(-1, 3)
        blo, bhi = bx.min(axis=0), bx.max(axis=0)
        sel = one_level & (np.abs(np.where(one_level, lo, -1.0) - s) <= 1e-9 * s)
        inside = (mesh.coords[sel] > blo + 1e-9 * s) & (mesh.coords[sel] < bhi - 1e-9 * s)
        want[sel] = np.prod(np.where(inside, 2, 1), axis=1)
    ok = ~hanging & ~parent & one_level & ~touches_hanging & (count == want)
    ok[owned:] = False
    return ok


# every mixed state of the level tests
MIXED = [lambda b=b: LC.block_case(b) for b in (True, False)] + [lambda a=a: big_block_case(a) for a in (True, False)] + [line_search_case]
MIXED += [lambda w=w: weights_case(*w) for w in ((1.0, 0.0), (0.5, 1.0))]  # split_jacobian_cases.WEIGHTS
