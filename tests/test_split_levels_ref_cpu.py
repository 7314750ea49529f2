"""Every input condition of tests/test_gpu_split_levels_jacobian.py on the CPU, from the numpy reference alone, so that no GPU
test fails on its input: every mixed state has its share of tensile q-points within split_jacobian_cases.SHARE and
min |tr E| / |E|_F >= split_jacobian_cases.MARGIN (on the reference's strains), the one-sided states are one-sided, in the
tension state the reference of the law is the unsplit oracle, and the numpy copy of "regular row" finds rows on both levels
of both blocks."""
import numpy as np
import pytest
import scipy.sparse as sp

import cases
import split_jacobian_cases as JC
import split_levels_cases as VC
import split_voldev_cases as SC
from gpu_util import linf_scaled, oracle
from test_gpu_split3d import _copy


@pytest.mark.parametrize("k", range(len(VC.MIXED)))
def test_mixed_states_hold_their_conditions(k):
    c = VC.MIXED[k]()
    share, margin = JC.conditions(c)
    print(f"{c.name}: share {share:.3f}, margin {margin:.1e}")
    assert JC.SHARE == (0.25, 0.75) and JC.MARGIN == 1e-6
    assert c.params.decompose_stress_matrix > 0 and c.params.timestep_number > 0
    assert c.mesh.hn_nodes.size > 0 and c.cell_lambda is not None and c.cu.flag.any()


def test_the_states_are_what_the_tests_say_they_are():
    a, b = VC.MIXED[0](), VC.MIXED[1]()
    assert a.layout.blocked and not b.layout.blocked and a.mesh.n_cells == b.mesh.n_cells == 960
    big, free = VC.big_block_case(True), VC.big_block_case(False)
    for c in (big, free):
        assert not c.layout.blocked and c.params.outer_solver == 1 and c.params.gamma_penal > 0 and c.params.use_old_timestep_pf == 1
        fine = np.unique(np.round(c.mesh.coords[np.asarray(c.mesh.hn_nodes)], 9), axis=0)
        assert fine.size > 0
    # the fine lattice of the (12, 10, 12) block: 13 x 9 x 13 nodes (6 x 4 x 6 coarse cells are refined: the centres within a
    # quarter of the extent of the middle), so more than one 8 x 4 tile of k_cart_split3_jac in x and in y on both levels
    x = big.mesh.coords[big.mesh.cells]
    size = (x.max(axis=1) - x.min(axis=1))[:, 0]
    fine_nodes = np.unique(big.mesh.cells[size < 0.75 * size.max()])
    dims = [np.unique(np.round(big.mesh.coords[fine_nodes, d], 9)).size for d in range(3)]
    assert dims == [13, 9, 13] and dims[0] > 8 and dims[1] > 4, dims
    phi_lines = lambda c: (c.cu.flag.astype(bool) & ~c.ch.flag.astype(bool))[c.layout.dof(np.arange(c.mesh.n_nodes), 3)]
    assert phi_lines(big).any() and not phi_lines(free).any(), "the active set is what the two states differ in"


@pytest.mark.parametrize("k", range(len(VC.MIXED)))
def test_regular_rows_of_both_levels(k):
    c = VC.MIXED[k]()
    reg = VC.regular_rows(c.mesh)
    x = c.mesh.coords[c.mesh.cells]
    size = (x.max(axis=1) - x.min(axis=1))[:, 0]
    fine = np.zeros(c.mesh.n_nodes, bool)
    fine[np.unique(c.mesh.cells[size < 0.75 * size.max()])] = True
    print(f"{c.name}: {int(reg.sum())} regular rows of {c.mesh.n_nodes}, {int((reg & fine).sum())} on the fine level")
    assert (reg & fine).sum() >= 64 and (reg & ~fine).sum() >= 64  # each level keeps its lattice (PFM_OVERLAY3_MIN_ROWS)
    hanging = np.zeros(c.mesh.n_nodes, bool)
    hanging[np.asarray(c.mesh.hn_nodes)] = True
    assert not (reg & hanging).any() and not reg[np.unique(c.mesh.hn_parents)].any()
    assert 0.3 * c.mesh.n_nodes < reg.sum() < c.mesh.n_nodes


def test_weights_and_the_cells_the_level_kernels_count():
    assert [(VC.MIXED[k]().params.decompose_stress_matrix, VC.MIXED[k]().params.decompose_stress_rhs) for k in (-2, -1)] == JC.WEIGHTS
    for w in JC.WEIGHTS:
        assert w[0] != w[1] and w[0] > 0
    # the compression state: the cells whose lowest vertex is a regular row -- fewer than the regular rows, because the coarse
    # level reaches the boundary of the domain and the regular rows on its upper faces have no cell above them
    c = VC.one_sided_case(-1)
    reg = VC.regular_rows(c.mesh)
    owning = VC.rows_owning_a_cell(c.mesh, reg)
    top = (c.mesh.coords >= c.mesh.coords.max(axis=0) - 1e-9).any(axis=1)
    print(f"{c.name}: {int(reg.sum())} regular rows, {owning.size} own a cell, {int((reg & top).sum())} lie on an upper face of the domain")
    assert (int(reg.sum()), owning.size) == (729, 512) and int((reg & top).sum()) == 729 - 512 and not top[owning].any()
    assert int(VC.general_cells(c.mesh, reg).sum()) == 600


@pytest.mark.parametrize("sign", [+1, -1])
def test_one_sided_states(sign):
    c = VC.one_sided_case(sign)
    SC.assert_one_sided(c, sign)
    assert c.params.decompose_stress_matrix == 1.0 and c.params.decompose_stress_rhs == 1.0  # the weights of route 0's tests
    if sign > 0:
        # without compression the law is the identity: its reference equals the UNSPLIT oracle, within 1e-13
        off = cases.Case(c.name, c.mesh, c.layout, _copy(c.params, decompose_stress_matrix=0.0, decompose_stress_rhs=0.0), c.sol, c.old, c.oldold,
                         c.cu, c.ch, None, c.cell_lambda, c.cell_mu)
        r, rowptr, colind = oracle(off, False)
        ref = JC.ref(VC.one_sided_case, +1)
        A_ref = sp.csr_matrix((r.values, colind, rowptr), shape=ref.A.shape)
        A_ref.sort_indices()
        assert ref.A.nnz == A_ref.nnz and (ref.A.indices == A_ref.indices).all()
        e = (linf_scaled(ref.A.data, A_ref.data), linf_scaled(ref.pde, r.residual_pde))
        print(f"{c.name}: reference of the law against the unsplit oracle: matrix {e[0]:.2e} residual {e[1]:.2e}")
        assert max(e) < 1e-13, e
