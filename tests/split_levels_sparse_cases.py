"""The states of the tests of the sparse volumetric-deviatoric split Jacobian on the level lattices of a 3-D overlay
(PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS_SPARSE = 61, PFM_SPLIT_ROUTE_LATTICE_ALL_LEVELS_SPARSE = 63;
tests/test_gpu_split_levels_sparse_jacobian.py, tests/test_gpu_glue_split_route_levels_sparse.py), and what the route does with a
state, computed from the numpy reference's strains and split_levels_cases.regular_rows alone.
tests/test_split_levels_sparse_ref_cpu.py runs every condition on the CPU, so a GPU test never fails on its input.

corner(shape, kind): the corner state of tests/split_sparse_cases.py on a block-refined mesh -- a dilation of 1e-2 plus noise of
2e-4 (tension everywhere), and on the nodes of a block at the lowest corner of the domain the gradient -2e-2 on top, taken
from that corner: the cells inside the block are compressed by 1e-2, every other cell keeps tr E > 0.  The block reaches from
the corner through the coarse cells into the refined region, so it lies partly in either and crosses the seam with its hanging
nodes, which are interpolated again after the block is added.

  (8, 8, 8)     the refined block of LC.block_case (coarse edge 2.5, refined region [5, 15]^3 from the corner), block <= 9 on every
                axis: 3 fine cells deep into the refined region
  (12, 10, 12)  refined_block_case((12, 10, 12)) (coarse edges 5/3, 2, 5/3; refined region [5, 15] x [6, 14] x [5, 15]), block
                <= (7.6, 9.1, 7.6): several 8 x 4 tiles of k_cart_uu3 per level, most of them without a touched row

kinds: split_sparse_cases.KINDS -- "lame" (blocked, active set, per-cell Lame), "homogeneous" (its twin with the scalars),
"monolithic" (interleaved, monolithic scheme with the penalty term, per-cell Lame)."""
import functools

import numpy as np

import split_levels_cases as VC
import split_sparse_cases as XC
import split_voldev_cases as SC
import split_voldev_ref as V
from test_gpu_split3d import _params

MARGIN = XC.MARGIN  # min |tr E| / |E|_F over the q-points
T3X, T3Y = XC.T3X, XC.T3Y
SEED = 101
SMALL, BIG = (8, 8, 8), VC.BIG
BLOCK = {SMALL: (9.0, 9.0, 9.0), BIG: (7.6, 9.1, 7.6)}  # from the lowest corner of the domain
KINDS = XC.KINDS
CORNER_IDS = [(s, k) for s in (SMALL, BIG) for k in KINDS]
# shape -> (compressed cells, cells, compressed cells whose lowest vertex is a regular row (what the level kernels count),
#           compressed cells of the general family, margin to three digits); the same for every kind
COUNTS = {SMALL: (53, 960, 27, 33, 1.42e-3), BIG: (90, 2448, 64, 33, 3.51e-3)}
# shape -> per level, coarse first: (touched regular rows, regular rows, nodes of the level lattice per axis)
LEVEL_ROWS = {SMALL: ((56, 604, (9, 9, 9)), (8, 125, (9, 9, 9))), BIG: ((117, 1614, (13, 11, 13)), (8, 405, (13, 9, 13)))}
# shape -> chunk length -> per level, coarse first: (flagged tile-chunks, tile-chunks, untouched regular rows inside flagged ones)
TILE_CHUNKS = {SMALL: {1: ((4, 54, 52), (2, 54, 12)), 4: ((1, 18, 52), (1, 18, 12))},
               BIG: {1: ((10, 78, 153), (2, 78, 16)), 4: ((4, 24, 270), (1, 24, 16))}}


@functools.lru_cache(maxsize=None)
def corner(shape, kind="lame"):
    blocked, solver, gamma, lame = KINDS[kind]
    block, lines = VC._block(shape, blocked)
    mesh = block.mesh
    c = SC.mixed_case(f"levels_sparse/corner/{shape}/{kind}", mesh, blocked, _params(1.0, 1.0, outer_solver=solver, gamma_penal=gamma), SEED, lines,
                      cell_lame=lame, grad=SC.EXPAND, noise=2e-4)
    x = mesh.coords - mesh.coords.min(axis=0)
    blk = np.nonzero((x <= np.asarray(BLOCK[shape])).all(axis=1))[0]
    for k in range(3):
        c.sol[c.layout.dof(blk, k)] += x[blk] @ (-2.0 * SC.EXPAND)[k]
    c.sol = c.ch.distribute(c.sol)  # the hanging nodes on the faces of the refined region, from their parents' new values
    assert c.ch.flag.any() and (c.cell_lambda is not None) == lame
    return c


def margin(c):
    return V.trace_conditions(SC.strains(c))[1]


def compressed_cells(c):
    return XC.compressed_cells(c)


def touched_rows(c):
    """bool per node: a regular row that is a vertex of a compressed cell (all eight cells of a regular row are cells of its
    level lattice) -- its four rows are those of route 13 under route 61"""
    return XC.touched_rows(c) & VC.regular_rows(c.mesh)


def counted_cells(c):
    """the compressed cells whose lowest vertex is a regular row: what route 13 and the mark kernel count"""
    cells = np.asarray(c.mesh.cells, np.int64)
    lowest = cells[np.arange(cells.shape[0]), np.argmin(c.mesh.coords[cells].sum(axis=2), axis=1)]
    return int((compressed_cells(c) & VC.regular_rows(c.mesh)[lowest]).sum())


def levels(mesh):
    """per refinement level, coarse first: (regular rows of the level as node numbers, their positions in the level's lattice,
    nodes of the lattice per axis).  The lattice of a level is that of the box of its cells (cracks_amd/csrc/pfm_mesh_plan.h)."""
    reg = VC.regular_rows(mesh)
    cells = np.asarray(mesh.cells, np.int64)
    x = mesh.coords[cells]
    size = x.max(axis=1) - x.min(axis=1)
    out = []
    for s in np.unique(np.round(size[:, 0], 9))[::-1]:
        of = np.abs(size[:, 0] - s) <= 1e-9 * s
        h, lo, hi = size[of][0], x[of].reshape(-1, 3).min(axis=0), x[of].reshape(-1, 3).max(axis=0)
        nodes = np.intersect1d(np.nonzero(reg)[0], np.unique(cells[of]))
        ijk = np.rint((mesh.coords[nodes] - lo) / h).astype(int)
        out.append((nodes, ijk, np.rint((hi - lo) / h).astype(int) + 1))
    return out


def tile_chunks(c, zc):
    """per level, coarse first: (flagged tile-chunks, tile-chunks, untouched regular rows inside the flagged ones, touched
    regular rows, regular rows) of the level's grid of k_cart_uu3 tiles (8 x 4 nodes) for chunks of zc planes"""
    t = touched_rows(c)
    out = []
    for nodes, ijk, n in levels(c.mesh):
        ntx, nty, nch = -(-n[0] // T3X), -(-n[1] // T3Y), -(-n[2] // zc)
        tile = ijk[:, 0] // T3X + ntx * (ijk[:, 1] // T3Y + nty * (ijk[:, 2] // zc))
        flagged = np.zeros(ntx * nty * nch, bool)
        flagged[tile[t[nodes]]] = True
        out.append((int(flagged.sum()), int(flagged.size), int((flagged[tile] & ~t[nodes]).sum()), int(t[nodes].sum()), int(nodes.size)))
    return out
