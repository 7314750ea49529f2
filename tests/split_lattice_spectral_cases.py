"""The states of the tests of the spectral split on the row-owner lattice kernels (pfm_set_split_route with
PFM_SPLIT_ROUTE_LATTICE_ANY under PFM_SPLIT_SPECTRAL; tests/test_gpu_split_lattice_spectral.py,
tests/test_gpu_glue_split_route_spectral.py) and their numpy references (split3d_ref.element_matrices(jacobian=False) with
split3d_ref.distribute_vector / residual_total), computed once per case.  tests/test_split_lattice_spectral_ref_cpu.py runs
every input condition on the CPU, so a GPU test never fails on its input.

State recipe: that of test_gpu_split3d_routes.mixed_case, u = x SHEAR^T +- 2e-4 h, the three phase fields random in
(0.3, 0.9), on unit cells with the box hint (a lattice context, kernel path 1).  Conditions on every mixed state
(assert_mixed): every q-point has eigenvalues of both signs with margin >= 1e-2 (split3d_ref.eigen_margin), and the
reference residual differs from the same case with the split off by at least 1e-3 of |r_ref|_inf, so a kernel that ignores
the law cannot pass.

Boxes, kinds and the two-rank box are those of tests/split_lattice_cases.py (SHAPES, BOX, TWO_RANK_N)."""
import functools

import numpy as np

import cases
import split3d_ref as R
import split_lattice_cases as LC
import split_voldev_cases as SC
from cracks_amd import mesh as M
from test_gpu_split3d import SHEAR, _box, _case, _params
from test_gpu_split3d_routes import faces_and_active_set

NOISE = 2e-4
MARGIN, LAW_SHARE = 1e-2, 1e-3
SHAPES, BOX, BOX_IDS, TWO_RANK_N, LINE_SEARCH = LC.SHAPES, LC.BOX, LC.BOX_IDS, LC.TWO_RANK_N, LC.LINE_SEARCH
SEED = {(5, 4, 3): 100, (17, 16, 5): 101}  # margins 0.128 / 0.123 with per-cell Lame (numpy)
unsplit = LC.unsplit


def mixed_case(name, mesh, blocked, prm, seed, lines=None, cell_lame=False, grad=SHEAR, noise=NOISE):
    return SC.mixed_case(name, mesh, blocked, prm, seed, lines, cell_lame=cell_lame, grad=grad, noise=noise)


@functools.lru_cache(maxsize=None)
def box_case(shape, kind):
    blocked, solver, gamma, d_rhs, lame, lines, use_old = BOX[kind]
    mesh = _box(shape, perturb=False)
    prm = _params(d_rhs, 1.0, outer_solver=solver, gamma_penal=gamma, use_old_timestep_pf=use_old)
    c = mixed_case(f"lattice_spectral/{shape}/{kind}", mesh, blocked, prm, SEED[shape], faces_and_active_set(6)(mesh) if lines else None,
                   cell_lame=lame)
    assert c.mesh.box_shape is not None
    return c


class Ref:
    """residual_pde and residual_total of the numpy reference (the spectral law) at c.sol (or sol)"""

    def __init__(self, c, sol=None):
        self._c, self._sol, self._mats = c, (c.sol if sol is None else sol), None
        _, self.Re, self.E = R.element_matrices(c.mesh, c.layout, c.params, self._sol, c.old, c.oldold, c.cell_lambda, c.cell_mu, jacobian=False)
        self.pde = R.distribute_vector(c.layout, c.mesh.cells, self.Re, c.cu)
        self.tot = R.residual_total(c.layout, c.mesh.cells, c.params, self.Re, c.cu, c.ch)

    def matrices(self):
        """(A, A_tot) of the reference's law at the same state, made on first use: the matrices whose rows belong to
        residual_pde and residual_total -- what the per-row scale of tests/parity_scale.py is taken from"""
        if self._mats is None:
            c = self._c
            Ke, Re, _ = R.element_matrices(c.mesh, c.layout, c.params, self._sol, c.old, c.oldold, c.cell_lambda, c.cell_mu)
            A = R.distribute_matrix(c.mesh, c.layout, Ke, Re, c.cu)[0]
            self._mats = (A, A if c.params.outer_solver != 0 else R.distribute_matrix(c.mesh, c.layout, Ke, Re, c.ch)[0])
        return self._mats


@functools.lru_cache(maxsize=None)
def ref(case, *args):
    return Ref(case(*args))


def assert_mixed(c, r=None):
    """the two conditions of a mixed state -> (eigenvalue margin, share of the law in the residual)"""
    r = r or Ref(c)
    margin, mixed = R.eigen_margin(r.E)
    off = Ref(unsplit(c))
    share = float(np.abs(r.pde - off.pde).max()) / float(np.abs(r.pde).max())
    assert mixed and margin >= MARGIN and share >= LAW_SHARE, (c.name, mixed, margin, share)
    return margin, share


# ---- one-sided and edge states on a lattice ------------------------------------------------------------------------------
one_sided_case = LC.one_sided_case  # a dilation / compression of 1e-2 +- 2e-4 h on (5, 4, 3), Dirichlet faces and an active set


def assert_one_sided(c, sign):
    l = np.linalg.eigvalsh(Ref(c).E)
    assert (l > 0.0).all() if sign > 0 else (l < 0.0).all(), (c.name, float(l.min()), float(l.max()))


EDGE = ["zero", "diagonal", "isotropic", "shear"]


@functools.lru_cache(maxsize=None)
def edge_case(kind):
    """States where the eigen-solve meets its special cases, on (4, 3, 3) unit cells with power-of-two displacement gradients,
    so that the strain the device forms is exact: zero: u = 0 (nothing to rotate).  diagonal: grad u = diag(2^-9, -2^-11, 2^-9),
    an exactly diagonal strain of both signs (no rotation; a repeated eigenvalue).  isotropic: grad u = 2^-9 I.  shear:
    u = (2^-7 y, 0, 0), eigenvalues +-2^-8 and a zero eigenvalue.  E+ is continuous in E and independent of the basis inside
    an eigenspace: the bar holds whatever sign rounding gives a zero eigenvalue, and no margin condition applies."""
    a, b = 2.0 ** -9, 2.0 ** -11
    grad = {"zero": np.zeros((3, 3)), "diagonal": np.diag([a, -b, a]), "isotropic": a * np.eye(3), "shear": np.zeros((3, 3))}[kind]
    if kind == "shear":
        grad[0, 1] = 2.0 ** -7
    c = _case(_box((4, 3, 3), perturb=False), kind in ("shear", "diagonal"), _params(1.0, 1.0, outer_solver=1, gamma_penal=1e-2), grad, 0.0, seed=25)
    c.name = f"lattice_spectral/edge/{kind}"
    return c


def assert_edge(c):
    kind = c.name.rsplit("/", 1)[1]
    l = np.linalg.eigvalsh(Ref(c).E)
    top = np.abs(l).max()
    if kind == "zero":
        assert top == 0.0
    elif kind == "diagonal":
        assert np.allclose(l, [-2.0 ** -11, 2.0 ** -9, 2.0 ** -9], rtol=0, atol=1e-15)
    elif kind == "isotropic":
        assert np.allclose(l, 2.0 ** -9, rtol=0, atol=1e-15)
    else:
        assert np.allclose(l, [-2.0 ** -8, 0.0, 2.0 ** -8], rtol=0, atol=1e-15)


# ---- two ranks -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def two_rank_case(blocked):
    g = M.box_mesh(3, TWO_RANK_N)
    return mixed_case(f"lattice_spectral/two_ranks/{'blocked' if blocked else 'interleaved'}", g, blocked, _params(), 60, faces_and_active_set(5)(g))


# ---- overlay ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block_case(blocked=True):
    """the refined (8, 8, 8) block (hanging nodes, Dirichlet faces, an active set) with per-cell Lame: split_lattice_cases.block_case
    with the spectral recipe"""
    from test_gpu_overlay3d import refined_block_case

    shape = refined_block_case((8, 8, 8), blocked)
    lines = lambda lay, rng: np.nonzero(shape.cu.flag.astype(bool) & ~shape.ch.flag.astype(bool))[0]
    c = mixed_case("lattice_spectral/refined_block", shape.mesh, blocked, _params(), 50, lines, cell_lame=True)
    assert np.array_equal(c.cu.flag, shape.cu.flag) and c.ch.flag.any() and c.cell_lambda is not None
    return c


# ---- fused entry, line search, living context, glue -------------------------------------------------------------------------
LINE_SEARCH_SEED = 70


@functools.lru_cache(maxsize=None)
def line_search_case(blocked, solver):
    """split_lattice_cases.line_search_case with the spectral recipe"""
    mesh = _box((5, 4, 3), perturb=False)
    prm = _params(outer_solver=solver, gamma_penal=1e-2 if solver == 1 else 0.0)
    return mixed_case(f"lattice_spectral/line_search/{'blocked' if blocked else 'interleaved'}/solver={solver}", mesh, blocked, prm, LINE_SEARCH_SEED,
                      faces_and_active_set(5)(mesh))


LS_MAX_STEPS, LS_GAP = 4, 1e-9


@functools.lru_cache(maxsize=None)
def line_search_numpy_case(blocked, solver, norm, restore):
    """The Newton update of the line-search test and newton.line_search_numpy around the reference: (update, the norms of all
    LS_MAX_STEPS trials, the reference norm of the test, the result of the numpy search with it).  The reference norm sits
    between the norm of trial 2 and the smaller of trials 0 and 1 where the norms fall, so that trial 2 is accepted."""
    import line_search_cases as L
    from cracks_amd.newton import LineSearchOpts, line_search_numpy
    from test_gpu_split3d_routes import smallest_edge

    c = line_search_case(blocked, solver)
    upd = L.newton_update(c, seed=5, u_amp=NOISE * smallest_edge(c.mesh), phi_amp=0.5)
    trials = []

    def norm_of(sol):
        z = c.cu.set_zero(Ref(c, sol).pde)
        trials.append(float(np.linalg.norm(z)) if norm == "l2" else float(np.abs(z).max()))
        return trials[-1]

    line_search_numpy(norm_of, c.sol, upd, LineSearchOpts(LS_MAX_STEPS, L.DAMPING, 0.0, restore))  # exhaustion: every trial
    all_trials = tuple(trials)
    reference = 0.5 * (all_trials[2] + min(all_trials[:2])) if all_trials[2] < min(all_trials[:2]) else 2.0 * max(all_trials)
    del trials[:]
    result = line_search_numpy(norm_of, c.sol, upd, LineSearchOpts(LS_MAX_STEPS, L.DAMPING, reference, restore))
    return upd, all_trials, reference, result, tuple(trials)


MIXED = ([lambda a=a: box_case(*a) for a in BOX_IDS] + [lambda b=b: two_rank_case(b) for b in (True, False)] + [block_case] +
         [lambda a=a: line_search_case(*a) for a in LINE_SEARCH])
