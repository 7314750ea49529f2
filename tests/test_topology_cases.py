"""The fixtures of tests/topology_cases.py are what they claim (no GPU): every case reaches the fallback it is named for,
its hanging-node table is closed, the oracle assembles it, and the oracle's own summation-order noise on these thin cells
is far below the parity bar the GPU tests hold the kernels to."""
import numpy as np
import pytest

import oracle_api as O
import topology_cases as T
from cracks_amd import mesh as M
from gpu_util import linf_scaled

MAX_COLOURS = 62  # greedy_colours (pfm_mesh_plan.cpp)
MAX_ROW = 254     # pfm_graph.hip
HG_DEG = 64       # k_hanging_gather (pfm_kernels.hip)


def _rows(mesh):
    return np.diff(M.node_graph(mesh)[0])


def _cells_per_node(mesh):
    return np.bincount(mesh.cells.ravel(), minlength=mesh.n_nodes)


def _max_parents(mesh):
    return int(np.diff(mesh.hn_ptr).max()) if mesh.hn_nodes.size else 0


@pytest.mark.parametrize("closed", [True, False])
@pytest.mark.parametrize("v", [3, 30])
def test_fan_cells_are_strictly_convex_and_positively_oriented(v, closed):
    m = T.fan2d(v, closed)
    x = m.coords[m.cells[:, [0, 1, 3, 2]]]  # the perimeter pole -> P_2k -> P_2k+1 -> P_2k+2
    for i in range(4):
        a, b = x[:, (i + 1) % 4] - x[:, i], x[:, (i + 2) % 4] - x[:, (i + 1) % 4]
        assert (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0] > 0).all()
    assert _rows(m)[0] == (2 * v + 1 if closed else 2 * v + 2) and _cells_per_node(m)[0] == v
    m3 = T.extrude(m, 2)
    pole = m.n_nodes
    assert _cells_per_node(m3)[pole] == 2 * v and _rows(m3)[pole] == 3 * m.n_nodes


def test_colour_overflow_cases():
    c = T.fan2d_closed64()
    assert _cells_per_node(c.mesh).max() == 64 > MAX_COLOURS and _rows(c.mesh).max() == 129
    pole = c.extra["pole"]
    assert c.cu.flag[c.layout.dof(pole, 0)] and c.cu.flag[c.layout.dof(pole, 2)] and not c.cu.flag[c.layout.dof(pole, 1)]
    c = T.fan3d_41()
    pole = c.extra["pole"]
    assert _cells_per_node(c.mesh).max() == _cells_per_node(c.mesh)[pole] == 82 > MAX_COLOURS
    assert _rows(c.mesh).max() == _rows(c.mesh)[pole] == 249 <= MAX_ROW
    assert c.cu.flag[c.layout.dof(pole, 1)] and c.cu.flag[c.layout.dof(pole, 3)] and not c.cu.flag[c.layout.dof(pole, 0)]


def test_row_length_cases():
    c = T.fan2d_open126()
    assert _rows(c.mesh).max() == _rows(c.mesh)[0] == MAX_ROW  # accepted, the last slot is 253
    assert not c.cu.flag[[int(c.layout.dof(0, k)) for k in range(3)]].any()  # the row of 254 is alive
    assert _rows(T.fan2d_closed127().mesh).max() == MAX_ROW + 1
    assert _rows(T.fan3d_42().mesh).max() == MAX_ROW + 1
    for make in T.ACCEPTED:
        assert _rows(make().mesh).max() <= MAX_ROW, make.__name__


def test_parent_count_cases():
    c = T.hang2d_3parents()
    assert _max_parents(c.mesh) == 3 > 2 and _max_parents(M.sneddon_2d_prerefined_mesh()) == 2
    c = T.hang3d_5parents()
    assert _max_parents(c.mesh) == 5 > 4 and _max_parents(T.hang3d_mesh()) == 4
    assert _max_parents(T.hang3d_17resolved().mesh) <= 4 and _max_parents(T.fan3d_30_hanging().mesh) == 2


def test_resolved_node_case():
    c = T.hang3d_17resolved()
    cell = c.extra["cell"]
    assert len(T.resolved_nodes(c.mesh, cell)) > 16
    assert len(T.resolved_nodes(T.hang3d_mesh(), cell)) == 8
    # every other cell at a hanging vertex keeps a reduced record
    hanging = np.zeros(c.mesh.n_nodes, bool)
    hanging[c.mesh.hn_nodes] = True
    others = [k for k in np.nonzero(hanging[c.mesh.cells].any(axis=1))[0] if k != cell]
    assert others and all(len(T.resolved_nodes(c.mesh, k)) <= 16 for k in others)


def test_gather_into_a_long_row_case():
    c = T.fan3d_30_hanging()
    pole, node = c.extra["pole"], c.extra["node"]
    at_node = np.nonzero((c.mesh.cells == node).any(axis=1))[0]
    assert at_node.size == 2 and all(pole in T.resolved_nodes(c.mesh, k) for k in at_node)
    assert HG_DEG < _rows(c.mesh)[pole] == 183 <= MAX_ROW
    assert _cells_per_node(c.mesh).max() == 60 <= MAX_COLOURS  # no colour overflow: the default gather path stays on
    k = int(np.nonzero(c.mesh.hn_nodes == node)[0][0])
    assert list(c.mesh.hn_weights[c.mesh.hn_ptr[k]:c.mesh.hn_ptr[k + 1]]) == [0.4, 0.6]


def test_overflow_and_gather_case():
    c = T.fan3d_41_hanging()
    pole, node = c.extra["pole"], c.extra["node"]
    assert _cells_per_node(c.mesh)[pole] == 82 > MAX_COLOURS and HG_DEG < _rows(c.mesh)[pole] == 249 <= MAX_ROW
    at_node = np.nonzero((c.mesh.cells == node).any(axis=1))[0]
    assert at_node.size == 2 and all(pole in T.resolved_nodes(c.mesh, k) and len(T.resolved_nodes(c.mesh, k)) <= 16 for k in at_node)
    assert _max_parents(c.mesh) == 2  # slot table and reduced records exist: the default mode gathers


def _assemble(c, mesh):
    rp, ci = M.dof_sparsity(c.mesh, c.layout)
    r = O.assemble(mesh, c.layout, c.params, c.sol, c.old, c.oldold, c.cu, c.ch, False, rp, ci)
    ro = O.assemble(mesh, c.layout, c.params, c.sol, c.old, c.oldold, c.cu, c.ch, True)
    return r, ro


@pytest.mark.parametrize("make", T.ALL, ids=lambda f: f.__name__)
def test_oracle_assembles_and_its_order_noise_is_far_below_the_parity_bar(make):
    """The table is closed, the oracle returns err == 0 and finite values, and assembling the cells in a seeded random order
    instead of the given one changes values and residuals by less than 1e-14 (scaled by max(1, |reference|_inf)): the parity
    bar of 1e-12 of the GPU tests is two orders and more above the reference's own summation-order noise.

    Measured (|A|_inf, scaled difference of the values / residual_pde / residual_total):
      fan2d_closed64     2.4e+01  3.7e-17 / 1.5e-20 / 1.3e-17
      fan2d_open126      9.5e+01  1.2e-18 / 4.2e-18 / 4.2e-18
      fan3d_41           7.1e+00  3.8e-16 / 1.5e-16 / 1.5e-16
      hang2d_3parents    9.0e+00  2.0e-16 / 1.9e-16 / 1.9e-16
      hang3d_5parents    1.2e+02  9.3e-16 / 3.5e-16 / 3.5e-16
      hang3d_17resolved  1.2e+02  9.3e-16 / 3.5e-16 / 3.5e-16
      fan3d_30_hanging   7.1e+00  2.5e-16 / 1.6e-16 / 1.6e-16
      fan3d_41_hanging   7.1e+00  1.3e-16 / 1.5e-16 / 1.5e-16
      fan2d_closed127    4.8e+01  2.8e-17 / 8.1e-21 / 8.1e-21
      fan3d_42           7.1e+00  2.5e-16 / 1.3e-16 / 1.3e-16
    """
    c = make()
    m = c.mesh
    hanging = np.zeros(m.n_nodes, bool)
    hanging[m.hn_nodes] = True
    assert not hanging[m.hn_parents].any() and np.unique(m.hn_nodes).size == m.hn_nodes.size
    for k in range(m.hn_nodes.size):
        w = m.hn_weights[m.hn_ptr[k]:m.hn_ptr[k + 1]]
        assert abs(w.sum() - 1.0) < 1e-15 and (w > 0).all()
    r, ro = _assemble(c, m)
    assert r.err == 0 and ro.err == 0
    assert np.isfinite(r.values).all() and np.isfinite(r.residual_pde).all() and np.isfinite(ro.residual_total).all()
    assert np.abs(r.values).max() > 0 and np.abs(ro.residual_total).max() > 0
    perm = np.random.default_rng(3).permutation(m.n_cells)
    shuffled = M.Mesh(dim=m.dim, coords=m.coords, cells=np.ascontiguousarray(m.cells[perm]), boundary_nodes=m.boundary_nodes,
                      hn_nodes=m.hn_nodes, hn_ptr=m.hn_ptr, hn_parents=m.hn_parents, hn_weights=m.hn_weights)
    s, so = _assemble(c, shuffled)
    assert s.err == 0 and so.err == 0
    noise = (linf_scaled(s.values, r.values), linf_scaled(so.residual_pde, ro.residual_pde), linf_scaled(so.residual_total, ro.residual_total))
    print(f"      {c.name:18s} {np.abs(r.values).max():.1e}  " + " / ".join(f"{x:.1e}" for x in noise))
    assert max(noise) < 1e-14
