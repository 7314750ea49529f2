"""PfmGlue::split_route = PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE (21) with split_model = PFM_SPLIT_VOLDEV of
glue/cracks_gpu_assemble.cc through the mock of tests/test_glue_mock.py, on one rank, with the driver of
tests/test_gpu_glue_split_route_levels.py (tests/cpp/glue_split_route_levels_driver.cpp takes the route on its command line and
stays as it is): the corner state on (5, 4, 3) unit cells of tests/split_sparse_cases.py (homogeneous material, which is what
the mock's Problem carries) in the mock's shuffled vertex numbering.  The route reaches the context (pfm_ctx_split_route_info
answers 21, the residual-only and the full assembly on the lattice kernels, the 4 compressed cells -- where the mock's
numbering gives a lattice context; where it gives the one level lattice of an overlay, the full assembly is the general
family's), and the matrix, block by
block, and both residuals are within the 1e-12 bar of the numpy reference (split_jacobian_cases.Ref) and of the general route;
on the lattice kernels residual_pde of the full assembly is the residual-only call's, byte for byte."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import parity_scale as PS
import split_jacobian_cases as JC
import split_sparse_cases as XC
from cracks_amd import capi
from gpu_util import TOL, linf_scaled
from test_glue_mock import ROOT, _write_problem
from test_gpu_glue_split_route_levels import build_driver

GENERAL, SPARSE, VOLDEV = capi.SPLIT_ROUTE_GENERAL, capi.SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE, capi.SPLIT_VOLDEV
SHAPE, KIND = (5, 4, 3), "homogeneous"


def test_the_glue_documents_the_sparse_routes():
    text = open(os.path.join(ROOT, "glue", "cracks_gpu_assemble.cc")).read()
    assert "pfm_set_split_route(ctx, split_route)" in text and "PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE" in text
    header = open(os.path.join(ROOT, "include", "pfm_assemble.h")).read()
    assert "PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_SPARSE = 21" in header and "PFM_SPLIT_ROUTE_LATTICE_ALL_SPARSE = 23" in header


@pytest.mark.gpu
def test_glue_route_21_with_model_3_reaches_the_context(tmp_path):
    exe = build_driver()
    c = XC.corner(SHAPE, KIND)
    assert XC.margin(c) >= XC.MARGIN and c.cell_lambda is None and c.layout.blocked
    ref = JC.ref(XC.corner, SHAPE, KIND)
    lay = c.layout
    d = str(tmp_path)
    to_mock, blocks = _write_problem(c, d, seed=7)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess_run([exe, d, str(VOLDEV), str(GENERAL), str(SPARSE)], env)
    assert r.returncode == 0 and "glue_split_route_levels_driver: OK" in r.stdout, r.stdout + r.stderr
    read = lambda route, what: np.fromfile(os.path.join(d, f"sl_r{route}_{what}.bin"))
    ig, ix = read(GENERAL, "info"), read(SPARSE, "info")
    print(f"glue split route sparse {c.name}: info general {list(ig)}, route 21 {list(ix)}")
    assert list(ig[:4]) == [0.0, 0.0, 0.0, -1.0] and ig[4] == ix[4] and ix[4] in (1.0, 3.0)
    if ix[4] == 1.0:  # a box: the full assembly on the lattice kernels, the compressed cells of tests/split_sparse_cases.py
        assert list(ix[:4]) == [21.0, 1.0, 1.0, float(XC.COUNTS[SHAPE][0])]
    else:  # the one level lattice of an overlay: the full assembly keeps the general family
        assert list(ix[:4]) == [21.0, 1.0, 0.0, -1.0]
    # the reference in the mock's numbering, block by block on the mock's pattern
    rows = np.repeat(np.arange(lay.n_dofs), np.diff(ref.A.indptr))
    R = sp.csr_matrix((ref.A.data, (to_mock[rows], to_mock[ref.A.indices])), shape=ref.A.shape)
    R.sort_indices()
    nu = lay.n_u
    cut = ((0, nu), (nu, lay.n_dofs))
    want = [R[r0:r1, c0:c1].tocsr() for (r0, r1) in cut for (c0, c1) in cut]
    out = {}
    for route in (GENERAL, SPARSE):
        vals = [read(route, f"val{b}") for b in range(4)]
        for b in range(4):
            want[b].sort_indices()
            assert (want[b].indptr == blocks[b].indptr).all() and (want[b].indices == blocks[b].indices).all() and vals[b].size == want[b].nnz
        e = (max(linf_scaled(v, w.data) for v, w in zip(vals, want) if v.size), linf_scaled(read(route, "full")[to_mock], ref.pde),
             linf_scaled(read(route, "pde")[to_mock], ref.pde))
        print(f"glue split route sparse, route {route}: matrix {e[0]:.2e}, residual of the full assembly {e[1]:.2e}, residual-only {e[2]:.2e}")
        assert max(e) < TOL
        PS.assert_blocks(vals, [w.data for w in want], TOL, f"glue split route sparse, route {route} against the reference", list(PS.BLOCKS))
        for what in ("full", "pde"):
            PS.assert_parts(read(route, what)[to_mock], ref.pde, PS.is_phi(lay), TOL, f"glue split route sparse, route {route}, {what}")
        assert not vals[1].any()  # the structurally zero (u,phi) block
        out[route] = vals
    PS.assert_blocks(out[SPARSE], out[GENERAL], TOL, "glue split route sparse, route 21 against the general route", list(PS.BLOCKS))
    if ix[4] == 1.0:
        assert read(SPARSE, "full").tobytes() == read(SPARSE, "pde").tobytes(), "the Jacobian call's residual_pde is the line search's"
    else:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(out[SPARSE], out[GENERAL]))


def subprocess_run(cmd, env):
    import subprocess

    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout, r.stderr)
    return r
