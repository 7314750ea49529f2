"""The states of the tests of the volumetric-deviatoric split on the row-owner lattice kernels (pfm_set_split_route;
tests/test_gpu_split_lattice.py, tests/test_gpu_glue_split_route.py), built with split_voldev_cases.mixed_case, and their
numpy references (split_voldev_ref.element_matrices(jacobian=False) with split3d_ref.distribute_vector / residual_total),
computed once per case.  tests/test_split_lattice_ref_cpu.py runs every input condition on the CPU, so a GPU test never
fails on its input.

Boxes: unit cells with the box hint, so the context is a lattice context (kernel path 1).
  (5, 4, 3)    6 x 5 x 4 nodes: one partial tile of the 15 x 15 owned nodes of k_cart_residual3
  (17, 16, 5)  18 x 17 x 6 nodes: 2 x 2 tiles, partial in x and y; six planes are one z-chunk by default and three under
               pfm_ctx_force_zchunk(ctx, PFM_ZC_RES3, 2), with seams at every tile edge"""
import functools

import numpy as np

import cases
import split3d_ref as R
import split_voldev_cases as SC
import split_voldev_ref as V
from cracks_amd import mesh as M
from test_gpu_split3d import _box, _case, _copy, _params
from test_gpu_split3d_routes import faces_and_active_set

SHAPES = [(5, 4, 3), (17, 16, 5)]
# name -> (blocked, outer_solver, gamma_penal, decompose_stress_rhs, per-cell Lame, Dirichlet faces + active set, use_old_timestep_pf)
BOX = {
    "blocked/active_set/rhs1": (True, 0, 0.0, 1.0, False, False, 0),
    "interleaved/monolithic/rhs0/lame": (False, 1, 1e-2, 0.0, True, False, 0),
    "blocked/active_set/rhs1/lame/lines": (True, 0, 0.0, 1.0, True, True, 0),
    "interleaved/monolithic/rhs1/lines/use_old": (False, 1, 1e-2, 1.0, False, True, 1),
    "blocked/monolithic/rhs0/use_old": (True, 1, 1e-2, 0.0, False, False, 1),
    "interleaved/active_set/rhs0.5/lame/lines": (False, 0, 0.0, 0.5, True, True, 0),
}
BOX_IDS = [(s, k) for s in SHAPES for k in BOX]
SEED = {(5, 4, 3): 100, (17, 16, 5): 101}  # (the displacement is the first draw: share 0.506 / 0.507, margin 5.4e-5 / 1.1e-5 for every kind)


@functools.lru_cache(maxsize=None)
def box_case(shape, kind):
    blocked, solver, gamma, d_rhs, lame, lines, use_old = BOX[kind]
    mesh = _box(shape, perturb=False)
    prm = _params(d_rhs, 1.0, outer_solver=solver, gamma_penal=gamma, use_old_timestep_pf=use_old)
    c = SC.mixed_case(f"lattice/{shape}/{kind}", mesh, blocked, prm, SEED[shape], faces_and_active_set(6)(mesh) if lines else None, cell_lame=lame)
    assert c.mesh.box_shape is not None
    return c


class Ref:
    """residual_pde and residual_total of the numpy reference at c.sol (or sol)"""

    def __init__(self, c, sol=None):
        _, Re, self.E = V.element_matrices(c.mesh, c.layout, c.params, c.sol if sol is None else sol, c.old, c.oldold, c.cell_lambda, c.cell_mu,
                                           jacobian=False)
        self.pde = R.distribute_vector(c.layout, c.mesh.cells, Re, c.cu)
        self.tot = R.residual_total(c.layout, c.mesh.cells, c.params, Re, c.cu, c.ch)
        self._c, self._sol, self._mats = c, (c.sol if sol is None else sol), None

    def matrices(self):
        """(A, A_tot) of the reference's law at the same state, made on first use: the matrices whose rows belong to
        residual_pde and residual_total -- what the per-row scale of tests/parity_scale.py is taken from"""
        if self._mats is None:
            c = self._c
            Ke, Re, _ = V.element_matrices(c.mesh, c.layout, c.params, self._sol, c.old, c.oldold, c.cell_lambda, c.cell_mu)
            A = R.distribute_matrix(c.mesh, c.layout, Ke, Re, c.cu)[0]
            self._mats = (A, A if c.params.outer_solver != 0 else R.distribute_matrix(c.mesh, c.layout, Ke, Re, c.ch)[0])
        return self._mats


@functools.lru_cache(maxsize=None)
def ref(case, *args):
    return Ref(case(*args))


# ---- one-sided and edge states on a lattice ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def one_sided_case(sign):
    """a dilation (+1) / compression (-1) of 1e-2 plus noise on (5, 4, 3) unit cells, Dirichlet faces and an active set"""
    mesh = _box((5, 4, 3), perturb=False)
    return SC.mixed_case(f"lattice/{'tension' if sign > 0 else 'compression'}", mesh, sign > 0, _params(1.0, 1.0, outer_solver=1, gamma_penal=1e-2), 31,
                         faces_and_active_set(5)(mesh), grad=sign * SC.EXPAND, noise=2e-4)


@functools.lru_cache(maxsize=None)
def edge_case(kind):
    """zero: u = 0.  shear: u = (gamma y, 0, 0), gamma = 2^-7, on (4, 3, 3) unit cells.  The residual is continuous at tr E = 0
    (sigma+ + sigma- = sigma on either side), so whichever sign the device's trace has at a q-point, the bar holds."""
    grad = np.zeros((3, 3))
    if kind == "shear":
        grad[0, 1] = 2.0 ** -7
    c = _case(_box((4, 3, 3), perturb=False), kind == "shear", _params(1.0, 1.0, outer_solver=1, gamma_penal=1e-2), grad, 0.0, seed=25)
    c.name = f"lattice/edge/{kind}"
    return c


# ---- two ranks -------------------------------------------------------------------------------------------------------------
TWO_RANK_N = (33, 5, 4)  # 34 node planes in x, 17 per rank: a tile of 15 that reads no ghost and one of 2 that does (or the reverse)


@functools.lru_cache(maxsize=None)
def two_rank_case(blocked):
    """split_voldev_cases.two_rank_case, longer in x"""
    g = M.box_mesh(3, TWO_RANK_N)
    return SC.mixed_case(f"lattice/two_ranks/{'blocked' if blocked else 'interleaved'}", g, blocked, _params(), 60, faces_and_active_set(5)(g))


# ---- overlay ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block_case(blocked=True):
    """split_voldev_cases.block_case (the refined (8, 8, 8) block: hanging nodes, Dirichlet faces, an active set) with per-cell Lame"""
    from test_gpu_overlay3d import refined_block_case

    shape = refined_block_case((8, 8, 8), blocked)
    lines = lambda lay, rng: np.nonzero(shape.cu.flag.astype(bool) & ~shape.ch.flag.astype(bool))[0]
    c = SC.mixed_case("lattice/refined_block", shape.mesh, blocked, _params(), 50, lines, cell_lame=True)
    assert np.array_equal(c.cu.flag, shape.cu.flag) and c.ch.flag.any() and c.cell_lambda is not None
    return c


# ---- fused entry, line search, living context, glue -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def line_search_case(blocked, solver):
    """split_voldev_cases.line_search_case on the unperturbed box: a lattice context"""
    mesh = _box((5, 4, 3), perturb=False)
    prm = _params(outer_solver=solver, gamma_penal=1e-2 if solver == 1 else 0.0)
    return SC.mixed_case(f"lattice/line_search/{'blocked' if blocked else 'interleaved'}/solver={solver}", mesh, blocked, prm, 70,
                         faces_and_active_set(5)(mesh))


def unsplit(c):
    """the same case with the split off (time step 0 of the reference's gate, cracks.cc:2294)"""
    return cases.Case(c.name + "/step0", c.mesh, c.layout, _copy(c.params, timestep_number=0), c.sol, c.old, c.oldold, c.cu, c.ch, None,
                      c.cell_lambda, c.cell_mu)


LINE_SEARCH = [(True, 0), (False, 1)]
MIXED = ([lambda a=a: box_case(*a) for a in BOX_IDS] + [lambda b=b: two_rank_case(b) for b in (True, False)] + [block_case] +
         [lambda a=a: line_search_case(*a) for a in LINE_SEARCH])
