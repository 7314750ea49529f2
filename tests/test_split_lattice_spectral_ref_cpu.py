"""Every input condition of tests/test_gpu_split_lattice_spectral.py and tests/test_gpu_glue_split_route_spectral.py
(tests/split_lattice_spectral_cases.py) on the CPU, from the numpy reference alone, so that no GPU test fails on its input:
every q-point of a mixed state has eigenvalues of both signs with margin >= 1e-2 and the law moves the residual by at least
1e-3 of its size, the one-sided states are one-sided in every eigenvalue, the edge states have the eigenvalues they are named
after, every accept / reject of the line search is decided by a relative gap >= 1e-9, and the boxes carry the box hint that
makes their context a lattice context.  Also: the route constant of the binding."""
import numpy as np
import pytest

import split3d_ref as R
import split_lattice_spectral_cases as XC
from cracks_amd import capi
from gpu_util import TOL, linf_scaled


def test_the_route_constant():
    assert (capi.SPLIT_ROUTE_GENERAL, capi.SPLIT_ROUTE_LATTICE, capi.SPLIT_ROUTE_LATTICE_ANY) == (0, 1, 3)
    assert capi.SPLIT_ROUTE_LATTICE_ANY == capi.SPLIT_ROUTE_LATTICE | 2


@pytest.mark.parametrize("k", range(len(XC.MIXED)))
def test_mixed_states_hold_their_conditions(k):
    c = XC.MIXED[k]()
    margin, share = XC.assert_mixed(c)
    print(f"{c.name}: eigenvalue margin {margin:.3f}, the law's share of the residual {share:.2e}")
    assert c.params.decompose_stress_matrix > 0 and c.params.timestep_number > 0


def test_box_cases_cover_the_parameters_and_are_lattices():
    for shape, kind in XC.BOX_IDS:
        c = XC.box_case(shape, kind)
        blocked, solver, gamma, d_rhs, lame, lines, use_old = XC.BOX[kind]
        assert tuple(c.mesh.box_shape) == shape and c.layout.blocked == blocked and (c.cell_lambda is not None) == lame
        assert c.params.outer_solver == solver and c.params.decompose_stress_rhs == d_rhs and c.params.use_old_timestep_pf == use_old
        assert c.cu.flag.any() == lines
    assert {k[3] for k in XC.BOX.values()} == {0.0, 0.5, 1.0}
    assert tuple(XC.two_rank_case(True).mesh.box_shape) == XC.TWO_RANK_N


@pytest.mark.parametrize("sign", [+1, -1])
def test_one_sided_states(sign):
    c = XC.one_sided_case(sign)
    XC.assert_one_sided(c, sign)
    on = XC.Ref(c)
    assert np.isfinite(on.pde).all() and np.isfinite(on.tot).all() and c.mesh.box_shape is not None
    if sign > 0:  # without compression the law is the unsplit one: the reference says so itself
        args = (c.mesh, c.layout, c.params, c.sol, c.old, c.oldold, c.cell_lambda, c.cell_mu)
        _, Re0, _ = R.element_matrices(*args, jacobian=False, split=False)
        assert linf_scaled(np.asarray(on.Re), np.asarray(Re0)) < TOL


@pytest.mark.parametrize("kind", XC.EDGE)
def test_edge_states(kind):
    c = XC.edge_case(kind)
    XC.assert_edge(c)
    r = XC.Ref(c)
    assert np.isfinite(r.pde).all() and np.isfinite(r.tot).all() and c.mesh.box_shape is not None


@pytest.mark.parametrize("blocked,solver,norm,restore", [(True, 0, "l2", "saved"), (False, 1, "linf", "subtract")])
def test_every_comparison_of_the_line_search_has_a_gap(blocked, solver, norm, restore):
    upd, trials, reference, result, seen = XC.line_search_numpy_case(blocked, solver, norm, restore)
    print(f"trial norms {trials}, reference {reference}, numpy search: steps {result['steps']}, accepted {result['accepted']}")
    assert len(trials) == XC.LS_MAX_STEPS and all(np.isfinite(trials))
    assert all(abs(reference - t) >= XC.LS_GAP * abs(reference) for t in trials), (reference, trials)
    assert seen == trials[:len(seen)] and len(seen) == result["steps"] + 1  # the comparisons made are among those
    assert result["accepted"] and result["steps"] == (2 if trials[2] < min(trials[:2]) else 0)
