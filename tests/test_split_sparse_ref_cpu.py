"""Every input condition of tests/test_gpu_split_sparse_jacobian.py and tests/test_gpu_glue_split_route_sparse.py, on the CPU
from the numpy reference's strains (tests/split_sparse_cases.py): a GPU test never fails on its input."""
import numpy as np
import pytest

import split_jacobian_cases as JC
import split_lattice_cases as LC
import split_sparse_cases as XC
import split_voldev_cases as SC
from cracks_amd import capi


def test_route_values():
    assert capi.SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE == 21 == capi.SPLIT_ROUTE_LATTICE_JACOBIAN | 16
    assert capi.SPLIT_ROUTE_LATTICE_ALL_SPARSE == 23 == capi.SPLIT_ROUTE_LATTICE_ALL | 16
    assert "pfm_ctx_split_sparse_info" in capi.EXPORTS


@pytest.mark.parametrize("shape,kind", XC.CORNER_IDS, ids=[f"{s[0]}x{s[1]}x{s[2]}-{k}" for s, k in XC.CORNER_IDS])
def test_corner_counts_and_margin(shape, kind):
    c = XC.corner(shape, kind)
    cells, n_cells, rows, n_rows, margin = XC.COUNTS[shape]
    comp, touched, m = XC.compressed_cells(c), XC.touched_rows(c), XC.margin(c)
    print(f"split_sparse {c.name}: {comp.sum()} of {comp.size} cells compressed, {touched.sum()} of {touched.size} rows touched, margin {m:.3f}")
    assert (int(comp.sum()), comp.size, int(touched.sum()), touched.size) == (cells, n_cells, rows, n_rows)
    assert m >= XC.MARGIN and abs(m - margin) < 5e-4
    assert (c.cell_lambda is not None) == XC.KINDS[kind][3] and c.layout.blocked == XC.KINDS[kind][0]
    assert c.cu.flag.any() and c.mesh.box_shape is not None
    # a compressed cell is compressed at every q-point, every other cell at none: the block is sharp
    tr = np.trace(SC.strains(c), axis1=-2, axis2=-1)
    assert ((tr < 0.0).all(axis=1) == comp).all()


def test_corner_tile_chunks():
    c = XC.corner((17, 16, 5))
    for zc, want in XC.TILE_CHUNKS.items():
        assert XC.tile_chunks(c, zc) == want, zc
    flagged, total, untouched = XC.tile_chunks(c, 6)  # the six planes in one chunk
    assert 0 < flagged < total and untouched > 0


@pytest.mark.parametrize("blocked", [True, False])
def test_two_rank_corner_straddles_the_cut(blocked):
    c = XC.two_rank_corner(blocked)
    comp, touched = XC.compressed_cells(c), XC.touched_rows(c)
    x = c.mesh.coords[:, 0]
    cut = (LC.TWO_RANK_N[0] + 1) // 2  # 34 node planes, 17 per rank: nodes 0 .. 16 | 17 .. 33
    assert XC.margin(c) >= XC.MARGIN and 0 < comp.sum() < comp.size
    assert (touched & (x < cut)).any() and (touched & (x >= cut)).any() and (~touched & (x < cut)).any() and (~touched & (x >= cut)).any()
    assert c.cu.flag.any() and c.layout.blocked == blocked


def test_reused_states():
    for sign in (+1, -1):
        c = LC.one_sided_case(sign)
        SC.assert_one_sided(c, sign)
        assert XC.touched_rows(c).all() == (sign < 0) and XC.touched_rows(c).any() == (sign < 0)
    for shape, kind in LC.BOX_IDS:
        c = LC.box_case(shape, kind)
        JC.conditions(c)
        assert XC.compressed_cells(c).any()
    JC.conditions(JC.dead_case())
    t = XC.touched_rows(JC.dead_case())
    assert t.any() and not t.all()
