"""tests/split_voldev_ref.py -- the numpy assembly reference of the volumetric-deviatoric split -- pinned on the CPU:

* with the split off it is tests/split3d_ref.py (which tests/test_split3d_ref_cpu.py pins to the oracle);
* in a state with tr E >= 0 everywhere it is the unsplit assembly;
* on a single perturbed hex its (u,u) block is the central-difference derivative of its displacement residual;
* every input condition of tests/test_gpu_split_voldev.py (tests/split_voldev_cases.py), so that no GPU test fails on its input.

Bar where two assemblies are compared: gpu_util.TOL."""
import numpy as np
import pytest

import split3d_ref as R
import split_voldev_cases as SC
import split_voldev_ref as V
from gpu_util import TOL, linf_scaled
from test_gpu_split3d import _box, _case, _copy, _params


def _args(c):
    return (c.mesh, c.layout, c.params, c.sol, c.old, c.oldold, c.cell_lambda, c.cell_mu)


def _mat_err(A, A_ref):
    return float(abs(A - A_ref).max()) / max(1.0, float(abs(A_ref).max()))


def test_with_the_split_off_it_is_the_spectral_reference():
    """constraints, hanging nodes and per-cell Lame included: the same statements, so the same numbers"""
    c = SC.hanging_case(True, 0)
    A, res, E = V.assemble(*_args(c), split=False, cu=c.cu, ch=c.ch)
    A0, res0, E0 = R.assemble(*_args(c), split=False, cu=c.cu, ch=c.ch)
    assert np.array_equal(E, E0) and (A.indices == A0.indices).all()
    assert linf_scaled(A.data, A0.data) < 1e-15 and linf_scaled(res, res0) < 1e-15
    pde, tot, _ = V.assemble_residuals(*_args(c), split=False, cu=c.cu, ch=c.ch)
    pde0, tot0, _ = R.assemble_residuals(*_args(c), split=False, cu=c.cu, ch=c.ch)
    assert linf_scaled(pde, pde0) < 1e-15 and linf_scaled(tot, tot0) < 1e-15


@pytest.mark.parametrize("case", [lambda: SC.tension_case(0), lambda: SC.tension_case(1), SC.tension_hetero_case], ids=["active_set", "monolithic", "hetero_3d"])
def test_without_compression_it_is_the_unsplit_assembly(case):
    c = case()
    SC.assert_one_sided(c, +1)
    A, res, _ = V.assemble(*_args(c), cu=c.cu, ch=c.ch)  # the split on, as the parameters say
    A0, res0, _ = V.assemble(*_args(c), split=False, cu=c.cu, ch=c.ch)
    e_A, e_R = _mat_err(A, A0), linf_scaled(res, res0)
    print(f"split_voldev_ref {c.name}: split on against off, matrix {e_A:.2e} residual {e_R:.2e}")
    assert e_A < TOL and e_R < TOL


def test_uu_block_is_the_derivative_of_the_displacement_residual():
    """One perturbed hex in the mixed state, d_rhs = d_mat = 0.5 (the residual carries the stress whose tangent the matrix
    holds).  K_uu = -d R_u / d u by central differences with step s = 1e-8.  The law is piecewise linear in u, and
    min |tr E| >= 1e-5 is asserted: a step moves tr E by at most s |grad N| < 1e-7, no q-point changes sides and the
    quotient has no truncation error.  Its rounding error is ulp |R| / s ~ 1e-16 * 3 / 1e-8 = 3e-8 next to |K_uu|_inf ~ 1e2;
    the bound is 1e-7 |K_uu|_inf."""
    mesh = _box((1, 1, 1), perturb=False)
    rng = np.random.default_rng(2)
    mesh.coords += rng.uniform(-0.12, 0.12, mesh.coords.shape)
    mesh.box_shape = None
    c = _case(mesh, False, _params(0.5, 0.5, outer_solver=1, gamma_penal=1e-2), SC.DEV, SC.NOISE, seed=13)
    Ke, Re, E = V.element_matrices(*_args(c))
    tr = np.trace(E, axis1=-2, axis2=-1)
    assert (tr > 0).any() and (tr < 0).any() and np.abs(tr).min() >= 1e-5, (tr.min(), tr.max(), np.abs(tr).min())
    udofs = np.array([c.layout.dof(n, k) for n in range(8) for k in range(3)])  # cell-dof order: local index 4 v + k
    loc = np.array([4 * v + k for v in range(8) for k in range(3)])
    Kuu = Ke[0][np.ix_(loc, loc)]
    s = 1e-8
    num = np.zeros_like(Kuu)
    for j, d in enumerate(udofs):
        sol1, sol0 = c.sol.copy(), c.sol.copy()
        sol1[d] += s
        sol0[d] -= s
        R1 = V.element_matrices(c.mesh, c.layout, c.params, sol1, c.old, c.oldold, jacobian=False)[1][0]
        R0 = V.element_matrices(c.mesh, c.layout, c.params, sol0, c.old, c.oldold, jacobian=False)[1][0]
        num[:, j] = -(R1 - R0)[loc] / (2 * s)
    err = np.abs(num - Kuu).max() / np.abs(Kuu).max()
    print(f"split_voldev_ref single hex: |K_uu - (-dR_u/du)| / |K_uu| = {err:.2e}, |K_uu|_inf = {np.abs(Kuu).max():.3g}")
    assert err < 1e-7
    # ... and the split matters here: the unsplit tangent is another matrix
    Ke0, _, _ = V.element_matrices(*_args(c), split=False)
    assert np.abs(Ke0[0][np.ix_(loc, loc)] - Kuu).max() > 1e-2 * np.abs(Kuu).max()


@pytest.mark.parametrize("k", range(len(SC.MIXED)))
def test_mixed_states_hold_their_conditions(k):
    c = SC.MIXED[k]()
    share, margin = SC.assert_mixed(c)
    print(f"split_voldev input {c.name}: share of tr E > 0 {share:.3f}, min |tr E| / |E|_F {margin:.2e}")


def test_one_sided_and_edge_states_hold_their_conditions():
    for solver in (0, 1):
        SC.assert_one_sided(SC.tension_case(solver), +1)
    SC.assert_one_sided(SC.tension_hetero_case(), +1)
    for blocked in (True, False):
        SC.assert_one_sided(SC.compression_case(blocked), -1)
    for kind in ("zero", "shear"):
        SC.assert_edge(SC.edge_case(kind))
