"""Every input condition of tests/test_gpu_split_lattice_jacobian.py and tests/test_gpu_glue_split_route_jacobian.py on the CPU,
from the numpy reference alone, so that no GPU test fails on its input: every mixed state has its share of tensile q-points
within [0.25, 0.75] and min |tr E| / |E|_F >= 1e-6 (split_voldev_ref.trace_conditions), the one-sided states are one-sided, the
weights differ where they should, the dead zone has vanishing element diagonals, and the two-rank box has unit cells."""
import numpy as np
import pytest

import split_jacobian_cases as JC
import split_lattice_cases as LC
import split_voldev_cases as SC
import split_voldev_ref as V
from gpu_util import TOL, linf_scaled


@pytest.mark.parametrize("k", range(len(JC.MIXED)))
def test_mixed_states_hold_their_conditions(k):
    c = JC.MIXED[k]()
    share, margin = JC.conditions(c)
    print(f"{c.name}: share {share:.3f}, margin {margin:.1e}")
    assert JC.SHARE == (0.25, 0.75) and JC.MARGIN == 1e-6
    assert c.params.decompose_stress_matrix > 0 and c.params.timestep_number > 0


@pytest.mark.parametrize("sign", [+1, -1])
def test_one_sided_states(sign):
    c = LC.one_sided_case(sign)
    SC.assert_one_sided(c, sign)
    if sign > 0:  # without compression the element matrices of the law are the unsplit ones: the reference says so itself
        args = (c.mesh, c.layout, c.params, c.sol, c.old, c.oldold, c.cell_lambda, c.cell_mu)
        Ke, _, _ = V.element_matrices(*args)
        Ke0, _, _ = V.element_matrices(*args, split=False)
        assert linf_scaled(np.asarray(Ke), np.asarray(Ke0)) < TOL


def test_weights_dead_zone_and_unit_cells():
    for d_mat, d_rhs in JC.WEIGHTS:
        c = JC.weights_case(d_mat, d_rhs)
        assert c.params.decompose_stress_matrix == d_mat and c.params.decompose_stress_rhs == d_rhs and d_mat != d_rhs and d_mat > 0
        assert c.mesh.box_shape is not None and c.cell_lambda is not None and c.cu.flag.any()
    d = JC.dead_case()
    assert d.params.constant_k == 0.0 and d.cu.flag.any() and d.mesh.box_shape is not None
    Ke, _, _ = V.element_matrices(d.mesh, d.layout, d.params, d.sol, d.old, d.oldold, d.cell_lambda, d.cell_mu)
    diag = np.abs(np.einsum("eii->ei", np.asarray(Ke)))
    print(f"dead zone: {int((diag == 0.0).any(axis=1).sum())} cells with a vanishing element diagonal entry")
    assert (diag == 0.0).any(), "no element diagonal vanishes: the case does not reach the mean-|diagonal| placeholder"
    for blocked in (True, False):
        c = JC.two_rank_case(blocked)
        assert tuple(c.mesh.box_shape) == LC.TWO_RANK_N and c.layout.blocked == blocked
        x = np.unique(c.mesh.coords[:, 0])
        assert np.array_equal(np.diff(x), np.ones(x.size - 1)), "unit cells: the same cell size on the box and on every sub-box"
