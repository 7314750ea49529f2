"""PfmGlue::split_route = PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS_SPARSE (61) with split_model = PFM_SPLIT_VOLDEV of
glue/cracks_gpu_assemble.cc through the mock of tests/test_glue_mock.py (the driver of tests/test_gpu_glue_split_route_levels.py,
which takes the routes on its command line), on one rank, on a refined mesh: the homogeneous corner state of
tests/split_levels_sparse_cases.py on the refined (8, 8, 8) block (hanging nodes, Dirichlet faces, an active set; homogeneous
material is what the mock's Problem carries) in the mock's shuffled vertex numbering.  The route reaches the context
(pfm_ctx_split_route_info answers 61, the residual-only and the full assembly on the level lattices, the compressed cells the
numpy prediction counts; kernel path 3), and the matrix, block by block, and both residuals are within the 1e-12 bar of the numpy
reference (split_jacobian_cases.Ref), of the general route and of route 13; residual_pde is route 13's, byte for byte."""
import os
import shutil

import numpy as np
import pytest
import scipy.sparse as sp
import subprocess

import parity_scale as PS
import split_jacobian_cases as JC
import split_levels_cases as VC
import split_levels_sparse_cases as YC
from gpu_util import TOL, linf_scaled
from test_glue_mock import GLUE, ROOT, _write_problem
from test_gpu_glue_split_route_levels import build_driver

GENERAL, JACL, LS, VOLDEV = 0, 13, 61, 3


def test_header_and_glue_name_the_new_constants():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    assert os.path.exists(build_driver())
    header = open(os.path.join(ROOT, "include", "pfm_assemble.h")).read()
    assert "PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS_SPARSE = 61" in header and "PFM_SPLIT_ROUTE_LATTICE_ALL_LEVELS_SPARSE = 63" in header
    text = open(GLUE).read()
    assert "pfm_set_split_route(ctx, split_route)" in text
    assert "PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS_SPARSE" in text and "PFM_SPLIT_ROUTE_LATTICE_ALL_LEVELS_SPARSE" in text


@pytest.mark.gpu
def test_glue_route_61_with_model_3_reaches_the_context_on_a_refined_mesh(tmp_path):
    exe = build_driver()
    c = YC.corner(YC.SMALL, "homogeneous")
    ref = JC.ref(YC.corner, YC.SMALL, "homogeneous")
    lay = c.layout
    d = str(tmp_path)
    to_mock, blocks = _write_problem(c, d, seed=7)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([exe, d, str(VOLDEV), str(GENERAL), str(JACL), str(LS)], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "glue_split_route_levels_driver: OK" in r.stdout, r.stdout + r.stderr
    read = lambda route, what: np.fromfile(os.path.join(d, f"sl_r{route}_{what}.bin"))
    info = {route: read(route, "info") for route in (GENERAL, JACL, LS)}
    print(f"glue split route levels sparse {c.name}: info general {list(info[GENERAL])}, route 13 {list(info[JACL])}, route 61 {list(info[LS])}")
    reg = VC.regular_rows(c.mesh)
    assert list(info[GENERAL][:5]) == [0.0, 0.0, 0.0, -1.0, 3.0]
    assert list(info[LS][:3]) == [61.0, 1.0, 1.0] and list(info[LS][3:]) == list(info[JACL][3:])
    assert info[LS][3] == YC.counted_cells(c) and info[LS][4] == 3.0 and info[LS][5] == float(reg.sum())
    # the reference in the mock's numbering, block by block on the mock's pattern
    rows = np.repeat(np.arange(lay.n_dofs), np.diff(ref.A.indptr))
    R = sp.csr_matrix((ref.A.data, (to_mock[rows], to_mock[ref.A.indices])), shape=ref.A.shape)
    R.sort_indices()
    nu = lay.n_u
    cut = ((0, nu), (nu, lay.n_dofs))
    want = [R[r0:r1, c0:c1].tocsr() for (r0, r1) in cut for (c0, c1) in cut]
    out = {}
    for route in (GENERAL, JACL, LS):
        vals = [read(route, f"val{b}") for b in range(4)]
        for b in range(4):
            want[b].sort_indices()
            assert (want[b].indptr == blocks[b].indptr).all() and (want[b].indices == blocks[b].indices).all() and vals[b].size == want[b].nnz
        e = (max(linf_scaled(v, w.data) for v, w in zip(vals, want) if v.size), linf_scaled(read(route, "full")[to_mock], ref.pde),
             linf_scaled(read(route, "pde")[to_mock], ref.pde))
        print(f"glue split route levels sparse, route {route}: matrix {e[0]:.2e}, residual of the full assembly {e[1]:.2e}, residual-only {e[2]:.2e}")
        assert max(e) < TOL
        PS.assert_blocks(vals, [w.data for w in want], TOL, f"glue split route levels sparse, route {route} against the reference", list(PS.BLOCKS))
        for what in ("full", "pde"):
            PS.assert_parts(read(route, what)[to_mock], ref.pde, PS.is_phi(lay), TOL, f"glue split route levels sparse, route {route}, {what}")
        assert not vals[1].any()  # the structurally zero (u,phi) block
        out[route] = vals
    PS.assert_blocks(out[LS], out[GENERAL], TOL, "glue split route levels sparse, route 61 against the general route", list(PS.BLOCKS))
    PS.assert_blocks(out[LS], out[JACL], TOL, "glue split route levels sparse, route 61 against route 13", list(PS.BLOCKS))
    print(f"glue split route levels sparse: {sum(int((a != b).sum()) for a, b in zip(out[LS], out[JACL]))} entries differ from route 13's in a bit "
          "(the untouched regular rows: the unsplit level kernels)")
    for what in ("full", "pde"):
        assert read(LS, what).tobytes() == read(JACL, what).tobytes(), f"{what}: the residuals of route 61 are route 13's bytes"
