"""Every input condition of tests/test_gpu_split_lattice.py and tests/test_gpu_glue_split_route.py (tests/split_lattice_cases.py)
on the CPU, from the numpy reference alone, so that no GPU test fails on its input: the mixed states have their share of
q-points on either side of the split and their margin (split_voldev_cases.assert_mixed), the one-sided states are one-sided,
the edge states have tr E = 0 in the reference, and the boxes carry the box hint that makes their context a lattice context."""
import numpy as np
import pytest

import split_lattice_cases as LC
import split_voldev_cases as SC
import split_voldev_ref as V
from gpu_util import TOL, linf_scaled


@pytest.mark.parametrize("k", range(len(LC.MIXED)))
def test_mixed_states_hold_their_conditions(k):
    c = LC.MIXED[k]()
    share, margin = SC.assert_mixed(c)
    print(f"{c.name}: share {share:.3f}, margin {margin:.1e}")
    assert c.params.decompose_stress_matrix > 0 and c.params.timestep_number > 0


def test_box_cases_cover_the_parameters_and_are_lattices():
    kinds = list(LC.BOX.values())
    for col, values in ((0, {True, False}), (1, {0, 1}), (4, {True, False}), (5, {True, False}), (6, {0, 1})):
        assert {k[col] for k in kinds} == values
    assert {0.0, 1.0} <= {k[3] for k in kinds} and all((k[2] > 0) == (k[1] == 1) for k in kinds)
    for shape, kind in LC.BOX_IDS:
        c = LC.box_case(shape, kind)
        blocked, solver, gamma, d_rhs, lame, lines, use_old = LC.BOX[kind]
        assert tuple(c.mesh.box_shape) == shape and c.layout.blocked == blocked and (c.cell_lambda is not None) == lame
        assert c.params.outer_solver == solver and c.params.decompose_stress_rhs == d_rhs and c.params.use_old_timestep_pf == use_old
        assert c.cu.flag.any() == lines
    assert tuple(LC.two_rank_case(True).mesh.box_shape) == LC.TWO_RANK_N


@pytest.mark.parametrize("sign", [+1, -1])
def test_one_sided_states(sign):
    c = LC.one_sided_case(sign)
    SC.assert_one_sided(c, sign)
    on = LC.Ref(c)
    assert np.isfinite(on.pde).all() and np.isfinite(on.tot).all()
    if sign > 0:  # without compression the law is the unsplit one: the reference says so itself
        args = (c.mesh, c.layout, c.params, c.sol, c.old, c.oldold, c.cell_lambda, c.cell_mu)
        _, Re, _ = V.element_matrices(*args, jacobian=False)
        _, Re0, _ = V.element_matrices(*args, jacobian=False, split=False)
        assert linf_scaled(np.asarray(Re), np.asarray(Re0)) < TOL


@pytest.mark.parametrize("kind", ["zero", "shear"])
def test_edge_states(kind):
    c = LC.edge_case(kind)
    SC.assert_edge(c)
    r = LC.Ref(c)
    assert np.isfinite(r.pde).all() and np.isfinite(r.tot).all() and c.mesh.box_shape is not None
