"""The constraint machinery of the numpy reference (tests/split3d_ref.py: element_matrices, distribute_matrix,
distribute_vector, residual_total) against the oracle, with the split off, where both compute the same thing: hanging nodes,
lines of constraints_update on about 10 % of the dofs, per-cell Lame coefficients.  What the GPU tests of the split on
constrained meshes (tests/test_gpu_split3d_routes.py) rest on.  Bar: gpu_util.TOL."""
import numpy as np
import pytest
import scipy.sparse as sp

import cases
import split3d_ref as R
import topology_cases as T
from cracks_amd import mesh as M
from gpu_util import TOL, linf_scaled, oracle


def _hang(blocked):
    c = T.make_case("h", T.hang3d_mesh(), blocked)
    assert c.mesh.hn_nodes.size == 72
    return c


def _hetero(perturb):
    c = cases.kat_hetero_3d()
    if perturb:  # (the step-0 state has u = 0: the stress terms of the residual vanish there)
        c = cases.perturbed(c)
    assert c.cell_lambda is not None and c.mesh.hn_nodes.size > 0
    return c


def _monolithic(c):
    """the other rule of residual_total (constraints_update instead of the hanging-node constraints) and the penalty"""
    c.params.outer_solver = 1
    c.params.gamma_penal = 1e-2
    c.params.timestep_number = 2
    return c


CASES = {"hang3d_blocked": lambda: _hang(True), "hang3d_interleaved": lambda: _hang(False), "hetero_3d": lambda: _hetero(False),
         "hetero_3d_perturbed": lambda: _hetero(True), "hang3d_monolithic": lambda: _monolithic(_hang(True))}


@pytest.mark.parametrize("name", list(CASES))
def test_reference_with_constraints_equals_the_oracle_with_the_split_off(name):
    c = CASES[name]()
    lines = c.cu.flag.astype(bool) & ~c.ch.flag.astype(bool)
    assert c.ch.flag.any() and lines.any()
    args = (c.mesh, c.layout, c.params, c.sol, c.old, c.oldold, c.cell_lambda, c.cell_mu)
    r, rowptr, colind = oracle(c, False)
    A_ref = sp.csr_matrix((r.values, colind, rowptr), shape=(c.layout.n_dofs,) * 2)
    A, res, _ = R.assemble(*args, split=False, cu=c.cu, ch=c.ch)
    assert A.nnz == A_ref.nnz and (A.indptr == A_ref.indptr).all() and (A.indices == A_ref.indices).all()
    e_A, e_R = linf_scaled(A.data, A_ref.data), linf_scaled(res, r.residual_pde)
    # the placeholder diagonals are there: a row of constraints_update holds its diagonal and nothing else
    d = int(np.nonzero(lines)[0][0])
    row = A[d].toarray().ravel()
    assert row[d] > 0.0 and np.count_nonzero(row) == 1
    r2, _, _ = oracle(c, True)
    pde, tot, _ = R.assemble_residuals(*args, split=False, cu=c.cu, ch=c.ch)
    e_2, e_t = linf_scaled(pde, r2.residual_pde), linf_scaled(tot, r2.residual_total)
    print(f"split3d_ref {name}: matrix {e_A:.2e} residual {e_R:.2e} residual-only {e_2:.2e} / {e_t:.2e}")
    assert e_A < TOL and e_R < TOL and e_2 < TOL and e_t < TOL
    # the two vectors differ on the lines of constraints_update exactly when the scheme is the active set's
    assert (np.abs(tot - pde)[lines].max() > 0.0) == (c.params.outer_solver == 0)


def test_without_constraints_the_distribution_is_the_plain_sum():
    """assemble(cu=None, ch=None) as before: every local entry lands on its own dofs"""
    c = T.make_case("box", M.box_mesh(3, (3, 2, 2)), True)
    args = (c.mesh, c.layout, c.params, c.sol, c.old, c.oldold)
    Ke, Re, _ = R.element_matrices(*args, split=False)
    A, res, _ = R.assemble(*args, split=False)
    dofs = c.layout.cell_dofs(c.mesh.cells)
    want, want_r = np.zeros((c.layout.n_dofs,) * 2), np.zeros(c.layout.n_dofs)
    for k, d in enumerate(dofs):
        want[np.ix_(d, d)] += Ke[k]
        want_r[d] += Re[k]
    assert np.abs(A.toarray() - want).max() <= 1e-15 * np.abs(want).max() and np.abs(res - want_r).max() <= 1e-15 * np.abs(want_r).max()
    pde, tot, _ = R.assemble_residuals(*args, split=False)
    assert np.array_equal(pde, res) and np.array_equal(tot, res)
