"""Small meshes whose topology reaches the fallbacks of the general cell kernels (tests/test_topology_cases.py asserts that
they do, tests/test_gpu_topology.py runs them):

* more than 62 cells at a node: no colour left, the cell goes to the atomic class and every cell adds atomically;
* a node-graph row of exactly 254 neighbours (the last uint8 slot is 253) and one of 255 (refused);
* a hanging node with more parents than the slot table of the cells at hanging vertices holds (row search instead);
* a 3-D cell at hanging vertices with more than 16 distinct constraint-resolved nodes (no reduced record: gather given up);
* contributions gathered into a row of more than 64 neighbours (the slow branch of the ordered gather);
* two of these at once: colour overflow on a 3-D mesh whose cells at hanging vertices take the ordered gather.

The meshes are fans of thin quadrilaterals around a pole node, their extrusions, and the refined meshes of the parity tests
with lines of the hanging-node table edited.  Assembly and oracle treat the table algebraically (C^T K C), so an edited line
need not be geometrically conforming; it only has to be closed (parents unconstrained).
"""
from __future__ import annotations

import numpy as np

import cases
from cracks_amd import mesh as M
from oracle_api import lame_from_E_nu, make_params


# ---- meshes -------------------------------------------------------------------------------------------------------------
def fan2d(v: int, closed: bool) -> M.Mesh:
    """``v`` strictly convex quadrilaterals around the pole (node 0, the origin).  Ring node P_j = node 1 + j lies on the
    unit circle at angle j * delta; cell k = [pole, P_2k, P_2k+2, P_2k+1] in deal.II vertex order (counter-clockwise
    pole -> P_2k -> P_2k+1 -> P_2k+2).  Closed: 2 v ring nodes around the full circle (P_2v = P_0), the pole's row has
    2 v + 1 neighbours; open: 2 v + 1 ring nodes on a half circle, 2 v + 2 neighbours."""
    n_ring = 2 * v if closed else 2 * v + 1
    delta = (2.0 * np.pi if closed else np.pi) / (2 * v)
    ang = delta * np.arange(n_ring)
    coords = np.concatenate([np.zeros((1, 2)), np.stack([np.cos(ang), np.sin(ang)], axis=1)])
    k = np.arange(v)
    ring = lambda j: 1 + (j % n_ring)
    cells = np.stack([np.zeros(v, np.int64), ring(2 * k), ring(2 * k + 2), ring(2 * k + 1)], axis=1).astype(np.int32)
    return M.Mesh(dim=2, coords=np.ascontiguousarray(coords), cells=np.ascontiguousarray(cells),
                  boundary_nodes={0: np.arange(1, 1 + n_ring, dtype=np.int32)})


def extrude(mesh2d: M.Mesh, layers: int, hz: float = 0.5) -> M.Mesh:
    """``layers`` layers of hexahedra over a 2-D mesh without hanging nodes: node n of plane p is node p * N2 + n."""
    assert mesh2d.dim == 2 and mesh2d.hn_nodes.size == 0
    n2 = mesh2d.n_nodes
    coords = np.concatenate([np.column_stack([mesh2d.coords, np.full(n2, hz * p)]) for p in range(layers + 1)])
    cells = np.concatenate([np.concatenate([mesh2d.cells + n2 * p, mesh2d.cells + n2 * (p + 1)], axis=1) for p in range(layers)])
    bn = {b: np.concatenate([nodes + n2 * p for p in range(layers + 1)]).astype(np.int32) for b, nodes in mesh2d.boundary_nodes.items()}
    return M.Mesh(dim=3, coords=np.ascontiguousarray(coords), cells=np.ascontiguousarray(cells.astype(np.int32)), boundary_nodes=bn)


def with_hanging(mesh: M.Mesh, node: int, parents, weights) -> M.Mesh:
    """A copy of the mesh in which ``node`` hangs on ``parents`` with ``weights`` (a new line of the closed table, or the
    replacement of the node's line).  Parents must not hang, and ``node`` must not be a parent."""
    parents, weights = [int(p) for p in parents], [float(w) for w in weights]
    assert len(parents) == len(weights) == len(set(parents)) and node not in parents
    lines = {int(n): (list(mesh.hn_parents[mesh.hn_ptr[k]:mesh.hn_ptr[k + 1]]), list(mesh.hn_weights[mesh.hn_ptr[k]:mesh.hn_ptr[k + 1]]))
             for k, n in enumerate(mesh.hn_nodes)}
    lines[int(node)] = (parents, weights)
    for n, (par, _) in lines.items():
        assert not any(int(p) in lines for p in par), "the table must stay closed"
    nodes = sorted(lines)
    ptr = np.concatenate([[0], np.cumsum([len(lines[n][0]) for n in nodes])]).astype(np.int64)
    return M.Mesh(dim=mesh.dim, coords=mesh.coords.copy(), cells=mesh.cells.copy(), boundary_nodes=dict(mesh.boundary_nodes),
                  hn_nodes=np.asarray(nodes, np.int32), hn_ptr=ptr,
                  hn_parents=np.asarray([p for n in nodes for p in lines[n][0]], np.int32),
                  hn_weights=np.asarray([w for n in nodes for w in lines[n][1]], np.float64))


def hang3d_mesh() -> M.Mesh:
    """The mesh of test_gpu_parity.test_hanging_nodes_3d: 4^3 cells, the inner 2^3 refined once."""
    m = M.box_mesh(3, 4)
    x = m.coords[m.cells].mean(axis=1)
    return M.refine_cells(m, (np.abs(x) < 5.0).all(axis=1))


def resolved_nodes(mesh: M.Mesh, cell: int) -> list:
    """The distinct constraint-resolved nodes of a cell: a vertex that does not hang is its own, a hanging one brings its
    parents."""
    line = {int(n): k for k, n in enumerate(mesh.hn_nodes)}
    out = []
    for n in mesh.cells[cell]:
        k = line.get(int(n))
        for p in ([int(n)] if k is None else mesh.hn_parents[mesh.hn_ptr[k]:mesh.hn_ptr[k + 1]]):
            if int(p) not in out:
                out.append(int(p))
    return out


def _free_nodes(mesh: M.Mesh) -> np.ndarray:
    """nodes that neither hang nor are a parent"""
    free = np.ones(mesh.n_nodes, bool)
    free[mesh.hn_nodes] = False
    free[mesh.hn_parents] = False
    return np.nonzero(free)[0]


# ---- state and parameters ----------------------------------------------------------------------------------------------------
def make_case(name: str, mesh: M.Mesh, blocked: bool = True, keep_free=(), flag=(), seed: int = 77, **extra) -> cases.Case:
    """Pressure and constant_k on; random u, phi in [0.2, 1] and independent old / old_old fields (cases.perturbed); about
    10 % of the dofs that do not hang carry a line of constraints_update.  ``keep_free``: nodes none of whose dofs is
    flagged (a long row that stays alive); ``flag``: (node, component) pairs that are."""
    lay = M.DofLayout(mesh.n_nodes, mesh.dim, blocked)
    h = mesh.min_cell_diameter()
    lam, mu = lame_from_E_nu(1.0, 0.2)
    prm = make_params(**{"lambda": lam}, mu=mu, G_c=1.0, alpha_eps=2.0 * h, constant_k=1e-8 * h, pressure=1.0e-3, timestep=1.0,
                      time=1.0, old_timestep=1.0, old_old_timestep=1.0, timestep_number=0)
    ch = M.hanging_constraints(mesh, lay)
    rng = np.random.default_rng(seed)
    node, comp = lay.node_comp_of_dof()
    pick = (rng.uniform(size=lay.n_dofs) < 0.1) & ~ch.flag.astype(bool) & ~np.isin(node, np.asarray(keep_free, np.int64))
    dd = set(int(d) for d in np.nonzero(pick)[0]) | set(int(lay.dof(n, c)) for n, c in flag)
    cu = M.update_constraints(mesh, lay, sorted(dd))
    sol = ch.distribute(lay.pack(np.zeros((mesh.n_nodes, mesh.dim)), np.full(mesh.n_nodes, 0.6)))
    base = cases.Case(name, mesh, lay, prm, sol, sol.copy(), sol.copy(), cu, ch)
    c = cases.perturbed(base, seed=seed + 1, u_amp=1e-3, phi_amp=0.4)
    c.name = name
    c.extra = dict(extra)
    return c


# ---- the named cases -----------------------------------------------------------------------------------------------------
def _fan2d_case(name, v, closed, blocked, flag_pole):
    # the pole's row is the one the case is about: alive, except where the case sums placeholder diagonals over its cells
    return make_case(name, fan2d(v, closed), blocked, keep_free=[0], flag=[(0, 0), (0, 2)] if flag_pole else [], pole=0)


def _fan3d_case(name, v, blocked, flag_pole):
    m2 = fan2d(v, True)
    pole = m2.n_nodes  # the pole of the middle plane
    return make_case(name, extrude(m2, 2), blocked, keep_free=[pole], flag=[(pole, 1), (pole, 3)] if flag_pole else [], pole=pole)


def fan2d_closed64(blocked=True):
    return _fan2d_case("fan2d_closed64", 64, True, blocked, True)


def fan2d_open126(blocked=True):
    return _fan2d_case("fan2d_open126", 126, False, blocked, False)


def fan2d_closed127(blocked=True):
    return _fan2d_case("fan2d_closed127", 127, True, blocked, False)


def fan3d_41(blocked=True):
    return _fan3d_case("fan3d_41", 41, blocked, True)


def fan3d_42(blocked=True):
    return _fan3d_case("fan3d_42", 42, blocked, False)


def hang2d_3parents(blocked=True):
    m = M.sneddon_2d_prerefined_mesh()
    node = int(m.hn_nodes[0])
    par = [int(p) for p in m.hn_parents[m.hn_ptr[0]:m.hn_ptr[1]]]
    third = int(_free_nodes(m)[5])
    return make_case("hang2d_3parents", with_hanging(m, node, par + [third], [0.5, 0.3, 0.2]), blocked, node=node)


def hang3d_5parents(blocked=True):
    m = hang3d_mesh()
    k = int(np.nonzero(np.diff(m.hn_ptr) == 4)[0][0])  # the centre of a coarse face
    node = int(m.hn_nodes[k])
    par = [int(p) for p in m.hn_parents[m.hn_ptr[k]:m.hn_ptr[k + 1]]]
    fifth = int(_free_nodes(m)[7])
    return make_case("hang3d_5parents", with_hanging(m, node, par + [fifth], [0.3, 0.25, 0.2, 0.15, 0.1]), blocked, node=node)


def hang3d_17resolved(blocked=True):
    """The lines of the hanging vertices of one cell, one after the other, replaced by four parents that no line has used
    yet, until the cell has more than 16 distinct resolved nodes."""
    m = hang3d_mesh()
    hanging = np.zeros(m.n_nodes, bool)
    hanging[m.hn_nodes] = True
    cell = int(np.argmax(hanging[m.cells].sum(axis=1)))  # a child in a corner of the refined block: 7 hanging vertices
    fresh = [int(n) for n in _free_nodes(m) if int(n) not in m.cells[cell]]
    for n in m.cells[cell]:
        if hanging[n] and len(resolved_nodes(m, cell)) <= 16:
            m = with_hanging(m, int(n), fresh[:4], [0.4, 0.3, 0.2, 0.1])
            fresh = fresh[4:]
    return make_case("hang3d_17resolved", m, blocked, cell=cell)


def _fan3d_hanging_case(name, v, blocked):
    m2 = fan2d(v, True)
    n2 = m2.n_nodes
    node = n2 + 2  # P_1 of the middle plane, between P_0 and P_2
    m = with_hanging(extrude(m2, 2), node, [n2 + 1, n2 + 3], [0.4, 0.6])
    return make_case(name, m, blocked, keep_free=[n2], pole=n2, node=node)


def fan3d_30_hanging(blocked=True):
    return _fan3d_hanging_case("fan3d_30_hanging", 30, blocked)


def fan3d_41_hanging(blocked=True):
    """Colour overflow and the ordered gather in one context: the last class holds the cells that found no colour next to
    the cells at the hanging vertex, and the pole's row of 249 receives all three kinds of adds."""
    return _fan3d_hanging_case("fan3d_41_hanging", 41, blocked)


ACCEPTED = [fan2d_closed64, fan2d_open126, fan3d_41, hang2d_3parents, hang3d_5parents, hang3d_17resolved, fan3d_30_hanging,
            fan3d_41_hanging]
REFUSED = [fan2d_closed127, fan3d_42]
ALL = ACCEPTED + REFUSED
