"""Every input condition of tests/test_gpu_split_levels_sparse_jacobian.py and tests/test_gpu_glue_split_route_levels_sparse.py,
on the CPU from the numpy reference's strains and split_levels_cases.regular_rows (tests/split_levels_sparse_cases.py): a GPU
test never fails on its input."""
import numpy as np
import pytest

import split_jacobian_cases as JC
import split_levels_cases as VC
import split_levels_sparse_cases as YC
import split_voldev_cases as SC
from cracks_amd import capi

IDS = [f"{s[0]}x{s[1]}x{s[2]}-{k}" for s, k in YC.CORNER_IDS]


def test_route_values():
    assert capi.SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS_SPARSE == 61 == capi.SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS | 16 | 32
    assert capi.SPLIT_ROUTE_LATTICE_ALL_LEVELS_SPARSE == 63 == capi.SPLIT_ROUTE_LATTICE_ALL_LEVELS | 16 | 32


@pytest.mark.parametrize("shape,kind", YC.CORNER_IDS, ids=IDS)
def test_corner_counts_margin_and_what_each_level_holds(shape, kind):
    c = YC.corner(shape, kind)
    cells, n_cells, counted, general, margin = YC.COUNTS[shape]
    comp, m = YC.compressed_cells(c), YC.margin(c)
    reg = VC.regular_rows(c.mesh)
    gen = VC.general_cells(c.mesh, reg)
    print(f"split_levels_sparse {c.name}: {comp.sum()} of {comp.size} cells compressed, {YC.counted_cells(c)} of them counted by the level kernels, "
          f"{(comp & gen).sum()} of them cells of the general family, margin {m:.3e}")
    assert (int(comp.sum()), comp.size, YC.counted_cells(c), int((comp & gen).sum())) == (cells, n_cells, counted, general)
    assert m >= YC.MARGIN and abs(m - margin) < 5e-6
    assert general >= 1, "a compressed cell is a cell of the general family"
    assert (c.cell_lambda is not None) == YC.KINDS[kind][3] and c.layout.blocked == YC.KINDS[kind][0]
    assert c.cu.flag.any() and c.ch.flag.any()
    # the hanging nodes hold what their parents give them
    assert np.array_equal(c.ch.distribute(c.sol.copy()), c.sol)
    # the block lies partly in either region: compressed cells of both sizes
    x = c.mesh.coords[np.asarray(c.mesh.cells, np.int64)]
    size = (x.max(axis=1) - x.min(axis=1))[:, 0]
    assert np.unique(np.round(size[comp], 9)).size == 2
    # each level: at least one touched and one untouched regular row
    t = YC.touched_rows(c)
    lv = YC.levels(c.mesh)
    assert len(lv) == 2 and sum(nodes.size for nodes, _, _ in lv) == int(reg.sum())
    for (nodes, ijk, n), (touched, rows, dims) in zip(lv, YC.LEVEL_ROWS[shape]):
        assert (int(t[nodes].sum()), nodes.size, tuple(int(k) for k in n)) == (touched, rows, dims)
        assert 0 < touched < rows and (ijk >= 0).all() and (ijk < n).all()


@pytest.mark.parametrize("shape", [YC.SMALL, YC.BIG], ids=["8x8x8", "12x10x12"])
def test_corner_tile_chunks(shape):
    c = YC.corner(shape)
    for zc, want in YC.TILE_CHUNKS[shape].items():
        got = YC.tile_chunks(c, zc)
        assert tuple(g[:3] for g in got) == want, (zc, got)
        assert all(g[3:] == w[:2] for g, w in zip(got, YC.LEVEL_ROWS[shape]))
    if shape == YC.BIG:  # 1-plane chunks: per level a flagged and an unflagged tile-chunk, an untouched regular row inside a flagged one
        for flagged, total, untouched in YC.TILE_CHUNKS[shape][1]:
            assert 0 < flagged < total and untouched > 0


def test_reused_states():
    for sign in (+1, -1):
        c = VC.one_sided_case(sign)
        SC.assert_one_sided(c, sign)
        reg = VC.regular_rows(c.mesh)
        assert (YC.touched_rows(c) == reg).all() == (sign < 0) and YC.touched_rows(c).any() == (sign < 0)
    for d_mat, d_rhs in JC.WEIGHTS:
        JC.conditions(VC.weights_case(d_mat, d_rhs))
    JC.conditions(VC.big_block_case(False))
    JC.conditions(VC.line_search_case())
