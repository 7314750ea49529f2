"""float64 numpy restatement of the post-processing functionals (include/pfm_newton.h: pfm_face_load, pfm_cod_lines,
pfm_sneddon_phi_error), written from the reference's loops (cracks.cc:3453-3550, 3726-3790, 4495-4516, 418-450) with
MappingQ1 per point: the checker of the device entries and of the fixtures."""
from __future__ import annotations

import numpy as np


GX = np.array([0.5 - 0.5 * 0.7745966692414834, 0.5, 0.5 + 0.5 * 0.7745966692414834])
GW = np.array([5.0 / 18.0, 8.0 / 18.0, 5.0 / 18.0])


def _shape(dim, xi):
    """Q1 values [P, nv] and reference gradients [P, nv, dim] at the points xi [P, dim]."""
    nv = 1 << dim
    P = xi.shape[0]
    N = np.ones((P, nv))
    dN = np.ones((P, nv, dim))
    for v in range(nv):
        for d in range(dim):
            bit = (v >> d) & 1
            f = xi[:, d] if bit else 1.0 - xi[:, d]
            N[:, v] *= f
            for e in range(dim):
                dN[:, v, e] *= (1.0 if bit else -1.0) if e == d else f
    return N, dN


def _node_state(mesh, layout, sol):
    n = np.arange(mesh.n_nodes)
    U = np.stack([sol[layout.dof(n, c)] for c in range(mesh.dim)], axis=1)
    return U, sol[layout.dof(n, mesh.dim)]


def face_points(dim, f):
    """QGauss<dim-1>(3) on face f in cell coordinates (QProjector's axis order) and the weights."""
    a, s = f >> 1, float(f & 1)
    pts, wts = [], []
    if dim == 2:
        for q in range(3):
            xi = np.zeros(2)
            xi[a], xi[1 - a] = s, GX[q]
            pts.append(xi)
            wts.append(GW[q])
    else:
        for q in range(9):
            q0, q1 = GX[q % 3], GX[q // 3]
            xi = {0: (s, q0, q1), 1: (q1, s, q0), 2: (q0, q1, s)}[a]
            pts.append(np.array(xi))
            wts.append(GW[q % 3] * GW[q // 3])
    return np.array(pts), np.array(wts)


def _face_eval(x, f, xi):
    """At one reference point xi on face f for the cells x [C, nv, dim]: N [nv], physical gradients [C, nv, dim], the
    outward unit normal [C, dim] and the surface element |cof(J) n_ref| [C]."""
    dim = x.shape[2]
    N, dN = _shape(dim, xi[None, :])
    N, dN = N[0], dN[0]
    J = np.einsum("cvi,vj->cij", x, dN)
    inv = np.linalg.inv(J)
    det = np.linalg.det(J)
    g = np.einsum("cej,ve->cvj", inv, dN)
    c = (1.0 if f & 1 else -1.0) * det[:, None] * inv[:, f >> 1, :]
    ln = np.sqrt(np.sum(c * c, axis=1))
    return N, g, c / ln[:, None], ln


def face_load(mesh, layout, sol, lam, mu, cells, faces):
    """Raw sum of int sigma(u) n dA over the (cell, face) pairs, undegraded stress (cracks.cc:3766-3785)."""
    dim = mesh.dim
    U, _ = _node_state(mesh, layout, sol)
    cells, faces = np.asarray(cells), np.asarray(faces)
    out = np.zeros(dim)
    for f in range(2 * dim):
        cs = cells[faces == f]
        if cs.size == 0:
            continue
        x = mesh.coords[mesh.cells[cs]]
        Uc = U[mesh.cells[cs]]
        pts, wts = face_points(dim, f)
        for xi, w in zip(pts, wts):
            N, g, n, ln = _face_eval(x, f, xi)
            gu = np.einsum("cvi,cvj->cij", Uc, g)
            E = 0.5 * (gu + np.swapaxes(gu, 1, 2))
            sig = lam * np.trace(E, axis1=1, axis2=2)[:, None, None] * np.eye(dim) + 2 * mu * E
            out += np.einsum("cij,cj->i", sig, n * (ln * w)[:, None])
    return out


def cod_lines(mesh, layout, sol, lines, eps=1e-8, cell_owned=None):
    """compute_cod of every line (cracks.cc:3485-3535) before the /2 and the MPI sum: (cod, n_faces)."""
    dim, nv = mesh.dim, mesh.nv
    lines = np.asarray(lines, float)
    U, PH = _node_state(mesh, layout, sol)
    x = mesh.coords[mesh.cells]
    cx = np.zeros(mesh.n_cells)
    for b in range(nv):
        cx = cx + x[:, b, 0]
    cx = cx / nv
    diam = mesh.cell_diameters()
    own = np.ones(mesh.n_cells, bool) if cell_owned is None else np.asarray(cell_owned, bool)
    near = own[None, :] & ~((cx - diam)[None, :] > lines[:, None]) & ~((cx + diam)[None, :] < lines[:, None])  # [L, C]
    cod = np.zeros(lines.size)
    n_faces = np.zeros(lines.size, np.int64)
    per_face = []
    for f in range(2 * dim):
        pts, wts = face_points(dim, f)
        N0, _, n0, _ = _face_eval(x, f, pts[0])
        q0x = x[:, :, 0] @ N0
        val = np.zeros(mesh.n_cells)
        for xi, w in zip(pts, wts):
            N, g, _, ln = _face_eval(x, f, xi)
            u = np.einsum("cvi,v->ci", U[mesh.cells], N)
            gp = np.einsum("cv,cvj->cj", PH[mesh.cells], g)
            val += 0.5 * np.sum(u * gp, axis=1) * (ln * w)
        ok = ~(np.abs(n0[:, 0]) < 0.5)
        match = near & ok[None, :] & (q0x[None, :] < lines[:, None] + eps) & (q0x[None, :] > lines[:, None] - eps)
        per_face.append((match, val))
    for match, val in per_face:
        cod += match.astype(float) @ val
        n_faces += match.sum(axis=1)
    return cod, n_faces


def exact_phi_sneddon(p, alpha_eps):
    """ExactPhiSneddon::value, cracks.cc:428-450 (l_0 = 1)."""
    dim = p.shape[1]
    left = np.zeros(dim)
    left[0] = -1.0
    right = -left
    d_left = np.sqrt(np.sum((p - left) ** 2, axis=1))
    d_right = np.sqrt(np.sum((p - right) ** 2, axis=1))
    d_mid = np.sqrt(np.sum(p[:, 1:] ** 2, axis=1))
    dist = np.where(p[:, 0] < -1.0, d_left, np.where(p[:, 0] > 1.0, d_right, d_mid))
    return 1.0 - np.exp(-dist / alpha_eps)


def sneddon_phi_error_sq(mesh, layout, sol, alpha_eps, cell_owned=None):
    """sum over the (owned) cells of int (phi_h - phi_exact)^2, QGauss(3)^dim (cracks.cc:4504-4516 before the root)."""
    dim = mesh.dim
    _, PH = _node_state(mesh, layout, sol)
    own = np.ones(mesh.n_cells, bool) if cell_owned is None else np.asarray(cell_owned, bool)
    x = mesh.coords[mesh.cells[own]]
    ph = PH[mesh.cells[own]]
    total = 0.0
    for q in range(3 ** dim):
        qi = [q % 3, (q // 3) % 3, q // 9][:dim]
        xi = np.array([GX[i] for i in qi])
        w = float(np.prod([GW[i] for i in qi]))
        N, dN = _shape(dim, xi[None, :])
        J = np.einsum("cvi,vj->cij", x, dN[0])
        p = np.einsum("cvi,v->ci", x, N[0])
        diff = exact_phi_sneddon(p, alpha_eps) - ph @ N[0]
        total += np.sum(diff * diff * np.linalg.det(J) * w)
    return float(total)


def tcv(mesh, layout, sol):
    """compute_tcv (cracks.cc:3575-3588): int u . grad phi, QGauss(3)^dim."""
    dim = mesh.dim
    U, PH = _node_state(mesh, layout, sol)
    x = mesh.coords[mesh.cells]
    total = 0.0
    for q in range(3 ** dim):
        qi = [q % 3, (q // 3) % 3, q // 9][:dim]
        xi = np.array([GX[i] for i in qi])
        w = float(np.prod([GW[i] for i in qi]))
        N, dN = _shape(dim, xi[None, :])
        J = np.einsum("cvi,vj->cij", x, dN[0])
        g = np.einsum("cej,ve->cvj", np.linalg.inv(J), dN[0])
        u = np.einsum("cvi,v->ci", U[mesh.cells], N[0])
        gp = np.einsum("cv,cvj->cj", PH[mesh.cells], g)
        total += np.sum(np.sum(u * gp, axis=1) * np.linalg.det(J) * w)
    return float(total)
