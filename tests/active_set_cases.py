"""Meshes, partitions and states of the tests of the partitioned active-set update (pfm_active_set_exchange,
newton.active_set_partitioned_numpy): three meshes with hanging nodes cut so that hanging nodes and their parents lie on
different ranks, a random state that is a function of the global node id, and the global statement of the update
(newton.py, ActiveSetDriver.newton_active_set) on the phase-field dofs."""
import functools

import numpy as np

import topology_cases
from cracks_amd import mesh as M
from cracks_amd import newton as NW
from cracks_amd import partition as P

MESHES = {"sneddon2d_amr": M.sneddon_2d_prerefined_mesh, "hang3d": topology_cases.hang3d_mesh,
          "hetero3d": M.hetero_3d_prerefined_mesh}
C_CONST = 10.0


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    return MESHES[name]()


@functools.lru_cache(maxsize=None)
def partition_of(name, world, ghost_layer="closure"):
    return P.partition_general(mesh_of(name), world, ghost_layer=ghost_layer)


def split_hanging_counts(lps):
    """(owned hanging nodes with a ghost parent, ghost hanging nodes with an owned parent), summed over the ranks"""
    a = b = 0
    for lp in lps:
        m, no = lp.mesh, lp.n_owned
        for k, n in enumerate(m.hn_nodes):
            par = m.hn_parents[m.hn_ptr[k]:m.hn_ptr[k + 1]]
            a += int(n < no and (par >= no).any())
            b += int(n >= no and (par < no).any())
    return a, b


@functools.lru_cache(maxsize=None)
def node_state(name, seed=11):
    """Random inputs of the update as functions of the global node id (test_gpu_newton_device.node_state, with the lumped
    mass from numpy): boundary nodes carry the displacement lines, about 30 % of the nodes the previous active set; the
    state is conforming (a hanging node's value is its parents')."""
    g = mesh_of(name)
    rng = np.random.default_rng(seed)
    N, dim = g.n_nodes, g.dim
    lay = M.DofLayout(N, dim, True)
    mass = NW.lumped_phase_mass(g, lay)[dim * N:]
    on_bnd = np.zeros(N, bool)
    for nodes in g.boundary_nodes.values():
        on_bnd[nodes] = True
    flags = np.where(on_bnd, (1 << dim) - 1, 0).astype(np.uint8)
    flags |= ((rng.random(N) < 0.3).astype(np.uint8) << dim).astype(np.uint8)
    flags[g.hn_nodes] = 0  # the lines of hanging nodes travel in the mesh description, not in the flag bytes
    st = dict(mass=mass, flags=flags, res_u=rng.standard_normal((N, dim)), res_phi=rng.standard_normal(N) * mass,
              u=rng.uniform(-1e-3, 1e-3, (N, dim)), phi=rng.uniform(0.0, 1.0, N), phi_old=rng.uniform(0.0, 1.0, N),
              cyc=rng.integers(0, 7, N).astype(np.int32))
    v = M.hanging_constraints(g, lay).distribute(lay.pack(st["u"], st["phi"]))
    st["u"] = np.stack([v[lay.dof(np.arange(N), k)] for k in range(dim)], axis=1)
    st["phi"] = v[lay.dof(np.arange(N), dim)]
    return st


def global_statement(g, st, c=C_CONST):
    """newton.py's statement (ActiveSetDriver.newton_active_set: criterion, phi := phi_old, distribute, cycle counter) on
    node arrays: dict(active [N] bool, u [N, dim], phi [N], cyc [N], counts (active, cycling, changed))"""
    N, dim = g.n_nodes, g.dim
    lay = M.DofLayout(N, dim, True)
    hanging = np.zeros(N, bool)
    hanging[g.hn_nodes] = True
    was = ((st["flags"] >> dim) & 1).astype(bool)
    gap = st["phi"] - st["phi_old"]
    with np.errstate(divide="ignore", invalid="ignore"):
        crit = st["res_phi"] / st["mass"] + c * gap
    inactive = (crit <= 0.0) & (st["cyc"] < 5)
    active = ~hanging & ~inactive
    n_cycling = int(np.sum(active & (st["cyc"] >= 5)))
    phi = st["phi"].copy()
    phi[active] = st["phi_old"][active]
    v = M.hanging_constraints(g, lay).distribute(lay.pack(st["u"], phi))
    cyc = st["cyc"].copy()
    cyc[was & ~active] += 1
    return dict(active=active, u=np.stack([v[lay.dof(np.arange(N), k)] for k in range(dim)], axis=1),
                phi=v[lay.dof(np.arange(N), dim)], phi_before_distribute=phi, cyc=cyc,
                counts=(int(active.sum()), n_cycling, int(np.any(was != active))))
