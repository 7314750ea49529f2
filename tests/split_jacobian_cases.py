"""The states of the tests of the volumetric-deviatoric split Jacobian on the row-owner lattice kernels
(PFM_SPLIT_ROUTE_LATTICE_JACOBIAN / _ALL; tests/test_gpu_split_lattice_jacobian.py, tests/test_gpu_glue_split_route_jacobian.py)
that tests/split_lattice_cases.py does not have already, and the full references (matrix, residual, residual_total) of all of
them, computed once per case.  tests/test_split_jacobian_ref_cpu.py runs every input condition on the CPU.

  weights_case(d_mat, d_rhs)   (5, 4, 3) unit cells with decompose_stress_matrix != decompose_stress_rhs: the identity
                               R_u = pressure part - K_uu u does not hold there
  dead_case()                  (5, 4, 3), kappa = 0, phi_old = phi_oldold = 0 and a dilation in a corner block of cells: g = 0 and
                               h = 1 at all their q-points (a compressed q-point keeps d_mat C-), so their (u,u) element
                               diagonals vanish and constrained displacement rows take deal.II's mean-|diagonal| placeholder
                               from those cells (the diagonal patches); the rest of the box stays mixed"""
import functools

import numpy as np

import cases
import split3d_ref as R
import split_lattice_cases as LC
import split_voldev_cases as SC
import split_voldev_ref as V
from cracks_amd import mesh as M
from test_gpu_split3d import _box, _copy, _params
from test_gpu_split3d_routes import faces_and_active_set

SHARE = (0.25, 0.75)  # of tensile q-points
MARGIN = 1e-6         # min |tr E| / |E|_F
WEIGHTS = [(1.0, 0.0), (0.5, 1.0)]  # (decompose_stress_matrix, decompose_stress_rhs)


@functools.lru_cache(maxsize=None)
def weights_case(d_mat, d_rhs, blocked=True):
    mesh = _box((5, 4, 3), perturb=False)
    prm = _params(d_rhs, d_mat, outer_solver=0 if blocked else 1, gamma_penal=0.0 if blocked else 1e-2)
    return SC.mixed_case(f"jacobian/weights/mat{d_mat}/rhs{d_rhs}", mesh, blocked, prm, LC.SEED[(5, 4, 3)], faces_and_active_set(6)(mesh), cell_lame=True)


@functools.lru_cache(maxsize=None)
def dead_case():
    c = LC.box_case((5, 4, 3), "blocked/active_set/rhs1/lame/lines")
    lay, mesh = c.layout, c.mesh
    dead = np.nonzero((mesh.coords[:, 0] <= 2.0) & (mesh.coords[:, 1] <= 2.0))[0]  # the nodes of the cells [0,2] x [0,2] x [0,3]
    old, oo = c.old.copy(), c.oldold.copy()
    old[lay.dof(dead, 3)] = 0.0
    oo[lay.dof(dead, 3)] = 0.0
    sol = c.sol.copy()
    for k in range(3):  # the dilation in the place of the deviatoric gradient, the noise kept
        sol[lay.dof(dead, k)] += mesh.coords[dead] @ (SC.EXPAND - np.asarray(SC.DEV))[k]
    d = cases.Case("jacobian/dead", mesh, lay, _copy(c.params, constant_k=0.0), sol, old, oo, c.cu, c.ch, None, c.cell_lambda, c.cell_mu)
    return d


@functools.lru_cache(maxsize=None)
def two_rank_case(blocked):
    """split_lattice_cases.two_rank_case on unit cells: the cell size of the global box and of each sub-box is 1.0 exactly, so
    a rank's matrix rows can be compared with the single rank's byte for byte (with the default extents h = 20 / 33 is taken
    from rounded coordinates and differs in its last bits between a sub-box and the box)"""
    g = _box(LC.TWO_RANK_N, perturb=False)
    return SC.mixed_case(f"jacobian/two_ranks/{'blocked' if blocked else 'interleaved'}", g, blocked, _params(), 61, faces_and_active_set(5)(g))  # seed chosen on the CPU: share 0.506, margin 2.1e-5


class Ref:
    """matrix on the oracle's pattern, residual_pde (of both calls), residual_total, and the matrix of residual_total's rows"""

    def __init__(self, c):
        Ke, Re, self.E = V.element_matrices(c.mesh, c.layout, c.params, c.sol, c.old, c.oldold, c.cell_lambda, c.cell_mu)
        self.A, self.pde = R.distribute_matrix(c.mesh, c.layout, Ke, Re, c.cu)
        self.tot = R.residual_total(c.layout, c.mesh.cells, c.params, Re, c.cu, c.ch)
        self.A_tot = self.A if c.params.outer_solver != 0 else R.distribute_matrix(c.mesh, c.layout, Ke, Re, c.ch)[0]


@functools.lru_cache(maxsize=None)
def ref(case, *args):
    return Ref(case(*args))


def conditions(c):
    """(share of tensile q-points, margin) of the reference's strains, held to the bounds above"""
    share, margin = V.trace_conditions(SC.strains(c))
    assert SHARE[0] <= share <= SHARE[1] and margin >= MARGIN, (c.name, share, margin)
    return share, margin


# every mixed state a Jacobian test uses
MIXED = ([lambda a=a: LC.box_case(*a) for a in LC.BOX_IDS] + [lambda b=b: two_rank_case(b) for b in (True, False)] + [LC.block_case] +
         [lambda w=w: weights_case(*w) for w in WEIGHTS] + [dead_case])
