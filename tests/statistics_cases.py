"""Meshes and cases shared by the tests of the COD bucket profile and the point evaluation (tests/test_statistics_numpy.py,
tests/test_gpu_statistics2.py)."""
import dataclasses

import numpy as np

import cases
from cracks_amd import mesh as M


def warp(mesh):
    """A smooth map of the coordinates (MappingQ1 is no longer affine per cell); the structured-box tag is dropped."""
    x = mesh.coords
    y = x.copy()
    nxt = (np.arange(mesh.dim) + 1) % mesh.dim
    for d in range(mesh.dim):
        y[:, d] += 0.04 * np.sin(1.3 * x[:, nxt[d]] + 0.4 + d) * np.cos(0.9 * x[:, (d + 2) % mesh.dim] + 0.2 * d)
    return dataclasses.replace(mesh, coords=np.ascontiguousarray(y), box_shape=None, boundary_nodes={})


def box2d():
    return M.box_mesh(2, (12, 8), lo=-1.5, hi=1.5)


def box3d():
    return M.box_mesh(3, (6, 5, 4), lo=-1.5, hi=1.5)


def box3d_warped():
    return warp(box3d())


def one_hexahedron():
    """One warped hexahedron spanning x in [-1.5, 1.5] and beyond."""
    c = np.array([[-1.55, -0.4, -0.3], [1.52, -0.5, -0.35], [-1.6, 0.45, -0.25], [1.58, 0.5, -0.4],
                  [-1.5, -0.35, 0.3], [1.6, -0.45, 0.4], [-1.57, 0.5, 0.35], [1.51, 0.4, 0.45]])
    return M.Mesh(dim=3, coords=c, cells=np.arange(8, dtype=np.int32)[None, :])


def threepoint():
    return cases.kat_threepoint().mesh


# name -> (mesh builder, [(n_buckets, x_lo, x_hi, n_sub), ...]); the first entry of the first six rows and the rows after
# them are the table of the issue that introduced pfm_cod_buckets
COD_CASES = {
    "box2d": (box2d, [(75, -1.5, 1.5, 100), (75, -1.5, 1.5, 1), (1, -1.37, 1.41, 4), (128, -1.37, 1.41, 4)]),
    "box3d": (box3d, [(75, -1.5, 1.5, 10)]),
    "box3d_warped": (box3d_warped, [(75, -1.5, 1.5, 10)]),
    "one_hexahedron": (one_hexahedron, [(75, -1.5, 1.5, 100)]),
    "threepoint": (threepoint, [(75, -1.5, 1.5, 100), (75, -4.03, 4.01, 7)]),
    "sneddon2d_amr": (M.sneddon_2d_prerefined_mesh, [(75, -1.5, 1.5, 100)]),
    "hetero3d_amr": (M.hetero_3d_prerefined_mesh, [(75, -1.5, 1.5, 6)]),
    "slit": (lambda: M.slit_mesh(3), [(75, -1.5, 1.5, 9)]),
}
TIE_MARGIN = 1e-9  # smallest allowed distance of value_to_bucket from an integer (in buckets)


def smooth_nodal(mesh, seed=7):
    """The smooth_state of tests/test_gpu_postproc.py as nodal values [n_nodes, dim + 1], hanging nodes distributed."""
    x = mesh.coords
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.5, 1.5, (4, mesh.dim))
    u = np.stack([1e-3 * np.sin(x @ a[c]) + 1e-4 * x[:, c] for c in range(mesh.dim)], axis=1)
    phi = 0.5 + 0.5 * np.tanh(np.abs(x[:, 1]) - 0.3 + 0.1 * np.cos(x @ a[3]))
    lay = M.DofLayout(mesh.n_nodes, mesh.dim, blocked=True)
    sol = M.hanging_constraints(mesh, lay).distribute(lay.pack(u, phi))
    n = np.arange(mesh.n_nodes)
    return np.stack([sol[lay.dof(n, c)] for c in range(mesh.dim + 1)], axis=1)


def eval_points(mesh, seed=3):
    """The points of the point-evaluation parity: 64 random interior points, every vertex of three cells, the face midpoints
    of those cells, points outside the bounding box and one just outside a boundary face (1e-3 of the cell size)."""
    dim, nv = mesh.dim, mesh.nv
    rng = np.random.default_rng(seed)
    X = mesh.coords[mesh.cells]
    cells = rng.integers(0, mesh.n_cells, 64)
    xi = rng.uniform(0.05, 0.95, (64, dim))
    N = np.ones((64, nv))
    for b in range(nv):
        for d in range(dim):
            N[:, b] *= xi[:, d] if (b >> d) & 1 else 1.0 - xi[:, d]
    pts = [np.einsum("kbi,kb->ki", X[cells], N)]
    three = sorted({0, mesh.n_cells // 2, mesh.n_cells - 1})
    for c in three:
        pts.append(X[c])
        for f in range(2 * dim):
            on = [b for b in range(nv) if ((b >> (f >> 1)) & 1) == (f & 1)]
            pts.append(X[c][on].mean(axis=0)[None, :])
    lo, hi = mesh.coords.min(axis=0), mesh.coords.max(axis=0)
    pts.append(np.stack([hi + 0.5, lo - 0.25, 0.5 * (lo + hi) + (hi - lo)]))
    # just outside the boundary face at the largest x: off the node with the largest x, by 1e-3 of a cell size
    n = int(np.argmax(mesh.coords[:, 0]))
    off = np.zeros(dim)
    off[0] = 1e-3 * float(mesh.cell_diameters().min())
    pts.append((mesh.coords[n] + off)[None, :])
    return np.concatenate(pts, axis=0)
