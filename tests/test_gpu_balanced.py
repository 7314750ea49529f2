"""The row-owner (cartesian) kernels, the (u,u) overlay and the general family on the balanced box states of
tests/balanced_cases.py -- states in which the elastic-energy, fracture, pressure and penalty terms are each a visible share
of every block they enter (the condition is checked on the CPU by tests/test_parity_scale_cpu.py) -- against the oracle with
gpu_util.full_parity: the project's bar and the four checks of tests/parity_scale.py (per entry, per block, per residual row,
per residual part), on the full assembly and on the residual-only call.

Last: the volumetric-deviatoric model with the lattice residual route on one balanced 3-D box against the numpy reference
(tests/split_voldev_ref.py)."""
import numpy as np
import pytest

import balanced_cases as B
import parity_scale as PS
import split_voldev_ref as V
from cracks_amd import capi
from cracks_amd.assembler import Context, node_flags_from_dof_flags
from gpu_util import TOL, blocks_to_global, full_parity, linf_scaled, make_context

pytestmark = pytest.mark.gpu

IDS = [B.case_id(a) for a in B.NAMES]
NAMES_3D = [a for a in B.NAMES if len(a[0]) == 3]


@pytest.mark.parametrize("a", B.NAMES, ids=IDS)
def test_cartesian_path_on_balanced_states(a):
    c = B.balanced_case(*a)
    ctx = make_context(c)
    assert ctx.kernel_path == 1, "a uniform box selects the cartesian family"
    ctx.force_path(1)
    full_parity(c, ctx=ctx)
    assert ctx.kernel_path == 1
    # no launch counter tells which kernels ran, so: the row-owner kernels give the same bits twice (no atomics, fixed order),
    # and not the bits of the general family, which sums each row in another order -- a quiet fall-back would give its bits
    v1, r1, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
    v2, r2, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
    assert all(np.array_equal(a, b) for a, b in zip(v1, v2)) and np.array_equal(r1, r2)
    v1 = [np.array(a, copy=True) for a in v1]
    ctx.force_path(0)
    v0, _, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
    assert not all(np.array_equal(a, b) for a, b in zip(v1, v0)), "the cartesian path gave the general family's bits"
    ctx.close()


@pytest.mark.parametrize("a", NAMES_3D, ids=[B.case_id(a) for a in NAMES_3D])
def test_uu_overlay_on_balanced_states(a):
    c = B.balanced_case(*a)
    ctx = make_context(c)
    ctx.force_path(2)
    assert ctx.kernel_path == 2
    full_parity(c, ctx=ctx)
    assert ctx.kernel_path == 2
    ctx.close()


@pytest.mark.parametrize("a", B.NAMES, ids=IDS)
def test_general_family_on_balanced_states(a):
    c = B.balanced_case(*a)
    ctx = make_context(c)
    ctx.force_path(0)
    assert ctx.kernel_path == 0
    full_parity(c, ctx=ctx)
    assert ctx.kernel_path == 0
    ctx.close()


def test_voldev_lattice_route_on_a_balanced_state():
    """PFM_SPLIT_VOLDEV with PFM_SPLIT_ROUTE_LATTICE: the residual-only call on k_cart_residual3<false, true>, the full assembly
    on the general family, both against the numpy reference of the law; scales from the reference's own matrix."""
    c = B.voldev_case()
    assert B.trace_margin(c) >= B.TRACE_MARGIN  # no q-point whose side of the split rounding decides
    A_ref, res_ref, _ = V.assemble(c.mesh, c.layout, c.params, c.sol, c.old, c.oldold, c.cell_lambda, c.cell_mu, cu=c.cu, ch=c.ch)
    pde_ref, tot_ref, _ = V.assemble_residuals(c.mesh, c.layout, c.params, c.sol, c.old, c.oldold, c.cell_lambda, c.cell_mu, cu=c.cu, ch=c.ch)
    ctx = Context(c.mesh, c.layout.blocked, cell_lambda=c.cell_lambda, cell_mu=c.cell_mu)
    ctx.set_split_model(capi.SPLIT_VOLDEV)
    ctx.set_split_route(capi.SPLIT_ROUTE_LATTICE)
    ctx.set_params(c.params)
    ctx.set_constraints(node_flags_from_dof_flags(c.layout, c.cu.flag, c.ch.flag))
    assert ctx.kernel_path == 1 and ctx.split_route_info() == (capi.SPLIT_ROUTE_LATTICE, 1)
    _, pde, tot = ctx.assemble_host(c.sol, c.old, c.oldold, True)
    assert linf_scaled(pde, pde_ref) < TOL and linf_scaled(tot, tot_ref) < TOL
    # monolithic scheme: residual_total is distributed with constraints_update, its rows are A_ref's
    assert c.params.outer_solver == 1
    PS.assert_residual(pde, pde_ref, A_ref, c.layout, c.sol, TOL, c.name + " lattice route residual_pde")
    PS.assert_residual(tot, tot_ref, A_ref, c.layout, c.sol, TOL, c.name + " lattice route residual_total")
    values, res, _ = ctx.assemble_host(c.sol, c.old, c.oldold, False)
    A = blocks_to_global(ctx, c.layout, values)
    A.sort_indices()
    assert linf_scaled(A.data, A_ref.data) < TOL and linf_scaled(res, res_ref) < TOL
    PS.assert_matrix(A, A_ref, c.layout, TOL, c.name + " full assembly")
    PS.assert_residual(res, res_ref, A_ref, c.layout, c.sol, TOL, c.name + " full assembly residual")
    ctx.close()
