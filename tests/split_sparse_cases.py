"""The states of the tests of the sparse volumetric-deviatoric split Jacobian (PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE = 21,
PFM_SPLIT_ROUTE_LATTICE_ALL_SPARSE = 23; tests/test_gpu_split_sparse_jacobian.py, tests/test_gpu_glue_split_route_sparse.py) that
tests/split_lattice_cases.py and tests/split_jacobian_cases.py do not have already, and what the route does with a state,
computed from the numpy reference's strains alone.  tests/test_split_sparse_ref_cpu.py runs every condition on the CPU, so a
GPU test never fails on its input.

corner(shape, kind): a dilation of 1e-2 plus noise of 2e-4 on unit cells (tension everywhere), and on the nodes of a corner
block the gradient -2e-2 on top: the cells inside the block are compressed by 1e-2, every other cell keeps tr E > 0 -- also the
cells with some vertices in the block, whose trace is a mix of both, see the margin.  Compression is confined to a small
region, as in a fracture run.

  (17, 16, 5)  block x <= 9, y <= 5, z <= 2:  90 of 1360 cells compressed, 180 of 1836 rows touched, margin 0.226; the
               touched rows lie in 12 of the 90 tile-chunks of k_cart_uu3's tiles (8 x 4 nodes) with 1-plane chunks and in 4 of
               30 with 4-plane chunks; 204 and 332 untouched rows sit inside flagged tile-chunks (the per-row skip)
  (5, 4, 3)    block x <= 2, y <= 1, z <= 2:  4 of 60 cells compressed, 18 of 120 rows touched, margin 0.304

kinds: "lame" (blocked, active set, per-cell Lame), "homogeneous" (its twin with the scalars), "monolithic" (interleaved,
monolithic scheme with the penalty term, per-cell Lame).

two_rank_corner(blocked): the corner state on the (33, 5, 4) unit-cell box of the two-rank tests, block x <= 19, y <= 2, z <= 1:
it straddles the cut between the ranks (x = 16 | 17)."""
import functools

import numpy as np

import split_lattice_cases as LC
import split_voldev_cases as SC
import split_voldev_ref as V
from test_gpu_split3d import _box, _params
from test_gpu_split3d_routes import faces_and_active_set

MARGIN = 1e-6   # min |tr E| / |E|_F over the q-points
T3X, T3Y = 8, 4  # owned nodes per tile of k_cart_uu3 (cracks_amd/csrc/pfm_cart_plan.h)
SEED = 101
BLOCK = {(17, 16, 5): (9, 5, 2), (5, 4, 3): (2, 1, 2), LC.TWO_RANK_N: (19, 2, 1)}
# shape -> (compressed cells, cells, touched rows, rows, margin to three digits)
COUNTS = {(17, 16, 5): (90, 1360, 180, 1836, 0.226), (5, 4, 3): (4, 60, 18, 120, 0.304)}
# (17, 16, 5): chunk length -> (flagged tile-chunks, tile-chunks, untouched rows inside flagged tile-chunks)
TILE_CHUNKS = {1: (12, 90, 204), 4: (4, 30, 332)}
# name -> (blocked, outer_solver, gamma_penal, per-cell Lame)
KINDS = {"lame": (True, 0, 0.0, True), "homogeneous": (True, 0, 0.0, False), "monolithic": (False, 1, 1e-2, True)}
CORNER_IDS = [(s, k) for s in ((5, 4, 3), (17, 16, 5)) for k in KINDS]


def _corner(name, mesh, shape, blocked, prm, lame, n_active):
    c = SC.mixed_case(name, mesh, blocked, prm, SEED, faces_and_active_set(n_active)(mesh), cell_lame=lame, grad=SC.EXPAND, noise=2e-4)
    bx, by, bz = BLOCK[shape]
    blk = np.nonzero((mesh.coords[:, 0] <= bx) & (mesh.coords[:, 1] <= by) & (mesh.coords[:, 2] <= bz))[0]
    for k in range(3):
        c.sol[c.layout.dof(blk, k)] += mesh.coords[blk] @ (-2.0 * SC.EXPAND)[k]
    assert c.mesh.box_shape is not None
    return c


@functools.lru_cache(maxsize=None)
def corner(shape, kind="lame"):
    blocked, solver, gamma, lame = KINDS[kind]
    mesh = _box(shape, perturb=False)
    return _corner(f"sparse/corner/{shape}/{kind}", mesh, shape, blocked, _params(1.0, 1.0, outer_solver=solver, gamma_penal=gamma), lame, 6)


@functools.lru_cache(maxsize=None)
def two_rank_corner(blocked):
    mesh = _box(LC.TWO_RANK_N, perturb=False)
    return _corner(f"sparse/two_ranks/{'blocked' if blocked else 'interleaved'}", mesh, LC.TWO_RANK_N, blocked, _params(), False, 5)


def compressed_cells(c):
    """bool per cell: some q-point of the reference has tr E < 0 (h(0) = 1: a zero trace is not compressed)"""
    tr = np.trace(SC.strains(c), axis1=-2, axis2=-1)
    return (tr < 0.0).any(axis=1)


def touched_rows(c):
    """bool per node: the node is a vertex of a compressed cell -- its four rows are those of route 5 under route 21"""
    t = np.zeros(c.mesh.n_nodes, bool)
    t[np.unique(c.mesh.cells[compressed_cells(c)])] = True
    return t


def margin(c):
    return V.trace_conditions(SC.strains(c))[1]


def tile_chunks(c, zc):
    """(flagged tile-chunks, tile-chunks, untouched rows inside the flagged ones) of a single-rank box for chunks of zc planes"""
    t = touched_rows(c)
    ijk = np.rint(c.mesh.coords).astype(int)
    n = ijk.max(axis=0) + 1
    ntx, nty, nch = -(-n[0] // T3X), -(-n[1] // T3Y), -(-n[2] // zc)
    tile = ijk[:, 0] // T3X + ntx * (ijk[:, 1] // T3Y + nty * (ijk[:, 2] // zc))
    flagged = np.zeros(ntx * nty * nch, bool)
    flagged[tile[t]] = True
    return int(flagged.sum()), int(flagged.size), int((flagged[tile] & ~t).sum())
