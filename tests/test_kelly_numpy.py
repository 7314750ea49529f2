"""RefinementStrategy::mix without a GPU (cracks.cc:4043-4103): the numpy statement of the Kelly indicator against closed
forms -- a kink on a mesh plane of a uniform box and on a refinement interface, a linear field across hanging faces --, the
face-neighbour table on meshes whose neighbours are known, the exact selection against np.sort, the fixed-number marking
rule, and the four new entry points of include/pfm_newton.h: declared, exported, and refusing a NULL context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cracks_amd import adapt as A
from cracks_amd import build, capi
from cracks_amd import mesh as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pfm_kelly_indicator", "pfm_indicator_select", "pfm_indicator_count", "pfm_refine_flags_mix"]


def kink_value(dim, h):
    """eta of a cell of edge h with one face on the plane of the kink u_0 = |x - x0|: the jump of the normal derivative
    is 2 on that face and 0 on the others, h_K = sqrt(dim) h:  sqrt(sqrt(dim) h / 24 * 4 h^(dim-1))"""
    return np.sqrt(np.sqrt(dim) * h ** dim / 6.0)


def half_refined(dim):
    """box_mesh(dim, 4, 0, 4) with the cells of centre x < 2 refined: the interface is the plane x = 2"""
    base = M.box_mesh(dim, 4, 0.0, 4.0)
    cx = base.coords[base.cells].mean(axis=1)[:, 0]
    return M.refine_cells(base, cx < 2.0)


def kink_field(mesh, x0):
    U = np.zeros((mesh.n_nodes, mesh.dim))
    U[:, 0] = np.abs(mesh.coords[:, 0] - x0)
    return U


def distributed(mesh, U):
    U = U.copy()
    for k, n in enumerate(mesh.hn_nodes):
        s = slice(mesh.hn_ptr[k], mesh.hn_ptr[k + 1])
        U[n] = mesh.hn_weights[s] @ U[mesh.hn_parents[s]]
    return U


# ---- the indicator ---------------------------------------------------------------------------------------------------

def test_published_kink_values():
    assert kink_value(2, 1.0) == pytest.approx(0.48549177170732344, abs=1e-15)
    assert kink_value(3, 1.0) == pytest.approx(0.537284965911771, abs=1e-15)


@pytest.mark.parametrize("dim", [2, 3])
def test_kink_on_a_uniform_box(dim):
    m = M.box_mesh(dim, 4, 0.0, 4.0)
    eta = A.kelly_numpy(m, kink_field(m, 2.0))
    cx = m.coords[m.cells].mean(axis=1)[:, 0]
    touching = np.abs(cx - 2.0) < 0.6
    assert touching.sum() == 2 * 4 ** (dim - 1)
    assert np.abs(eta[touching] - kink_value(dim, 1.0)).max() <= 1e-15
    assert np.abs(eta[~touching]).max() <= 1e-15
    # the other components and phi carry nothing; phi alone sees nothing of a displacement kink
    full = np.zeros((m.n_nodes, dim + 1))
    full[:, 0] = kink_field(m, 2.0)[:, 0]
    assert np.array_equal(A.kelly_numpy(m, full), eta)
    assert np.abs(A.kelly_numpy(m, full, component_mask=1 << dim)).max() == 0.0
    assert np.abs(A.kelly_numpy(m, full, component_mask=0b10)).max() == 0.0
    assert np.array_equal(A.kelly_numpy(m, full, component_mask=(1 << (dim + 1)) - 1), eta)
    for bad in (0, 1 << (dim + 1)):
        with pytest.raises(ValueError):
            A.kelly_numpy(m, full, component_mask=bad)
    own = (np.arange(m.n_cells) % 2).astype(np.uint8)
    assert np.array_equal(A.kelly_numpy(m, full, cell_owned=own), np.where(own != 0, eta, 0.0))


@pytest.mark.parametrize("dim", [2, 3])
def test_kink_on_a_refinement_interface(dim):
    m = half_refined(dim)
    assert m.hn_nodes.size > 0
    eta = A.kelly_numpy(m, kink_field(m, 2.0))
    d = m.cell_diameters()
    coarse = d > 1.5 * d.min()
    cx = m.coords[m.cells].mean(axis=1)[:, 0]
    at_c = coarse & (np.abs(cx - 2.0) < 0.6)
    at_f = ~coarse & (np.abs(cx - 2.0) < 0.3)
    assert at_c.sum() == 4 ** (dim - 1) and at_f.sum() == 8 ** (dim - 1)
    assert np.abs(eta[at_c] - kink_value(dim, 1.0)).max() <= 1e-15
    assert np.abs(eta[at_f] - kink_value(dim, 0.5)).max() <= 1e-15
    assert np.abs(eta[~(at_c | at_f)]).max() <= 1e-15


@pytest.mark.parametrize("dim", [2, 3])
def test_linear_field_across_hanging_faces(dim):
    m = half_refined(dim)
    a = np.random.default_rng(0).normal(size=(dim, dim))
    assert 0.1 < np.abs(a).max() < 10.0
    eta = A.kelly_numpy(m, m.coords @ a + 1.0)
    assert eta.max() < 1e-12


# ---- the face-neighbour table ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [2, 3])
def test_neighbours_of_a_uniform_box(dim):
    n = 3
    m = M.box_mesh(dim, n, 0.0, 1.0)
    fn = A.face_neighbours_numpy(m)
    idx = np.stack(np.unravel_index(np.arange(m.n_cells), (n,) * dim)[::-1], axis=1)  # (i, j, k) of a cell, x fastest
    for f in range(2 * dim):
        ax, side = f >> 1, f & 1
        j = idx.copy()
        j[:, ax] += 1 if side else -1
        inside = (j[:, ax] >= 0) & (j[:, ax] < n)
        want = np.where(inside, sum(j[:, d] * n ** d for d in range(dim)), -1)
        assert np.array_equal(fn.nbr[:, f], want)
        assert np.array_equal(fn.rel[:, f], np.where(inside, A.REL_SAME, A.REL_NONE))
    assert fn.sub.shape[0] == 0


@pytest.mark.parametrize("dim", [2, 3])
def test_neighbours_across_an_interface(dim):
    m = half_refined(dim)
    fn = A.face_neighbours_numpy(m)
    nsub = 1 << (dim - 1)
    counts = np.bincount(fn.rel.ravel(), minlength=4)
    assert counts[A.REL_COARSE] == 4 ** (dim - 1) and counts[A.REL_FINE] == nsub * counts[A.REL_COARSE]
    assert fn.sub.shape == (counts[A.REL_COARSE], nsub) and (fn.sub >= 0).all()
    assert (np.diff(fn.sub, axis=1) > 0).all()
    centre = m.coords[m.cells].mean(axis=1)
    cc, cf = np.nonzero(fn.rel == A.REL_COARSE)
    assert (cf == 0).all()  # the coarse cells look at the interface through their face x = lo
    for c, f in zip(cc, cf):
        fine = fn.sub[fn.nbr[c, f]]
        fc, ff = fine // (2 * dim), fine % (2 * dim)
        assert (ff == 1).all() and (fn.rel[fc, ff] == A.REL_FINE).all() and (fn.nbr[fc, ff] == c).all()
        assert np.abs(centre[fc, 1:] - centre[c, 1:]).max() <= 0.25 + 1e-12  # the fine cells sit on that face
    # symmetric among cells of one level
    c, f = np.nonzero(fn.rel == A.REL_SAME)
    back = fn.nbr[fn.nbr[c, f]]
    assert ((back == c[:, None]) & (fn.rel[fn.nbr[c, f]] == A.REL_SAME)).any(axis=1).all()


def test_slit_lips_and_hanging_boundary_edges_have_no_neighbour():
    m = M.slit_mesh(2)
    fn = A.face_neighbours_numpy(m)
    # 8 x 8 cells: 32 faces on the outer boundary + the two lips of four cell faces each
    assert (fn.rel == A.REL_NONE).sum() == 32 + 8
    # a fine cell's boundary face whose vertex hangs: the Sneddon 2-D mesh refines a block in the interior, the half-refined
    # box refines up to the boundary (the midpoint on the interface hangs and lies on boundary faces)
    h = half_refined(2)
    fn = A.face_neighbours_numpy(h)
    centre = h.coords[h.cells].mean(axis=1)
    for c, f in zip(*np.nonzero(fn.rel == A.REL_NONE)):
        x = h.coords[h.cells[c, M.face_vertices(2)[f]]]
        assert (np.ptp(x, axis=0) == 0.0).any() and ((x == 0.0) | (x == 4.0)).all(axis=0).any(), (c, f, centre[c])


# ---- selection and marking -------------------------------------------------------------------------------------------

def test_select_against_sort():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(1000)
    x[::7] = x[3]        # exact ties
    x[1::11] = 0.0
    x[2::13] = -0.0
    x[5::17] = np.nan
    x[6] = np.inf
    x[8] = -np.inf
    n_num = int((~np.isnan(x)).sum())
    desc = np.sort(x[~np.isnan(x)])[::-1]  # np.sort: ascending, NaN last
    for k in (1, 2, 10, 143, 144, 500, n_num - 1, n_num):
        t, above, equal = A.indicator_select_numpy(x, k)
        assert t == desc[k - 1] and not (t == 0.0 and np.signbit(t))
        assert above == (desc > t).sum() and equal == (desc == t).sum()
        assert above < k <= above + equal
        assert A.indicator_count_numpy(x, t) == (above, equal)
    t, above, equal = A.indicator_select_numpy(x, n_num + 1)  # rank k falls on a NaN: below every number
    assert np.isnan(t) and above == n_num and equal == x.size - n_num
    assert A.indicator_count_numpy(x, float("nan")) == (n_num, x.size - n_num)
    mask = (np.arange(x.size) % 3 == 0)
    sub = np.sort(x[mask & ~np.isnan(x)])[::-1]
    assert A.indicator_select_numpy(x, 20, mask)[0] == sub[19]
    for bad in (0, x.size + 1):
        with pytest.raises(ValueError):
            A.indicator_select_numpy(x, bad)
    # -0.0 and 0.0 are one value
    t, above, equal = A.indicator_select_numpy(np.array([-0.0, 0.0, -1.0, 1.0]), 2)
    assert t == 0.0 and not np.signbit(t) and (above, equal) == (1, 2)


@pytest.mark.parametrize("dim", [2, 3])
def test_fixed_number_marking(dim):
    m = half_refined(dim)
    rng = np.random.default_rng(1)
    nodal = np.ones((m.n_nodes, dim + 1))
    nodal[:, :dim] = distributed(m, rng.normal(size=(m.n_nodes, dim)))
    eta = A.kelly_numpy(m, nodal)
    s = np.sort(eta)[::-1]
    k = int(0.3 * m.n_cells)
    assert (s[k - 1] - s[k]) > 1e-9 * s[0]
    flags, n, t = A.refine_flags_mix_numpy(m, nodal, 0.3)
    assert n == k == flags.sum() and t == s[k - 1] and np.array_equal(flags.astype(bool), eta >= t)
    # k = 0: nothing beyond phi
    flags, n, t = A.refine_flags_mix_numpy(m, nodal, 0.5 / m.n_cells)
    assert n == 0 and t == np.inf
    # the cells phi flags are flagged, and their indicator does not take part
    nodal2 = nodal.copy()
    low = m.cells[np.argmax(eta)]
    nodal2[low, dim] = 0.1
    by_phi, n_phi = A.refine_flags_numpy(m, nodal2[:, dim], 0.5)
    assert by_phi[np.argmax(eta)] and n_phi >= 1
    flags, n, t = A.refine_flags_mix_numpy(m, nodal2, 0.3, phi_threshold=0.5)
    rest = np.where(by_phi.astype(bool), 0.0, eta)
    assert t == np.sort(rest)[::-1][k - 1] and np.array_equal(flags.astype(bool), by_phi.astype(bool) | (rest >= t))
    # the level limit comes last
    level = (m.cell_diameters() < 1.5 * m.cell_diameters().min()).astype(np.uint8)
    lim, n_lim, t_lim = A.refine_flags_mix_numpy(m, nodal2, 0.3, phi_threshold=0.5, max_level=1, cell_level=level)
    assert t_lim == t and np.array_equal(lim, flags * (level != 1))
    # top_fraction = 1 on an indicator with zeros (the cells that are not owned): t == 0 becomes the smallest positive
    # value, zeros never flag
    U = kink_field(m, 2.0)
    own = (np.arange(m.n_cells) % 3 != 0).astype(np.uint8)
    eta = A.kelly_numpy(m, U, cell_owned=own)
    assert (eta[own == 0] == 0.0).all() and np.sort(eta)[::-1][m.n_cells - 1] == 0.0
    flags, n, t = A.refine_flags_mix_numpy(m, np.column_stack([U, np.ones(m.n_nodes)]), 1.0, cell_owned=own)
    assert t == eta[eta > 0].min() and np.array_equal(flags.astype(bool), eta > 0) and 0 < n == (eta > 0).sum() < m.n_cells
    # all indicators zero
    still = np.zeros((m.n_nodes, dim + 1))
    still[:, dim] = 1.0
    flags, n, t = A.refine_flags_mix_numpy(m, still, 1.0)
    assert n == 0 and t == np.inf
    with pytest.raises(ValueError):
        A.refine_flags_mix_numpy(m, nodal, 1.5)


# ---- ABI -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    build.build_native()
    return capi.load()


def test_symbols_are_declared_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "pfm_newton.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pfm_[a-z0-9_]+)\s*\(", text))
    for n in NAMES:
        assert n in declared and n in capi.EXPORTS and hasattr(lib, n), n


def test_null_context_is_refused_without_a_gpu(lib):
    crit = capi.PfmRefineCriteria()
    n, t = C.c_int64(7), C.c_double(-1.0)
    counts = (C.c_int64 * 2)(5, 6)
    flags = (C.c_uint8 * 4)()
    buf = (C.c_double * 4)()
    assert lib.pfm_kelly_indicator(None, None, 3, buf) == 1  # PFM_ERR_BAD_ARG
    assert lib.pfm_indicator_select(None, buf, None, 1, C.byref(t), counts) == 1
    assert lib.pfm_indicator_count(None, buf, None, 0.5, counts) == 1
    assert lib.pfm_refine_flags_mix(None, C.byref(crit), 0.3, 3, None, None, flags, C.byref(n), C.byref(t)) == 1
    assert lib.pfm_refine_flags_mix(None, None, 0.3, 3, None, None, None, None, None) == 1
    assert (n.value, t.value, counts[0], counts[1]) == (7, -1.0, 5, 6)
