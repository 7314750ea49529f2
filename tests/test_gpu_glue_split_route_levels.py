"""PfmGlue::split_route = PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS (13) with split_model = PFM_SPLIT_VOLDEV of
glue/cracks_gpu_assemble.cc through the mock of tests/test_glue_mock.py (tests/cpp/glue_split_route_levels_driver.cpp), on one
rank, on a refined mesh: the refined (8, 8, 8) block of tests/split_voldev_cases.py (hanging nodes, Dirichlet faces, an active
set; homogeneous material, which is what the mock's Problem carries) in the mock's shuffled vertex numbering.  The route reaches
the context (pfm_ctx_split_route_info answers 13, the residual-only and the full assembly on the level lattices, a count of
compressed cells; kernel path 3 with the rows and general cells of the general route's context), and the matrix, block by
block, and both residuals are within the 1e-12 bar of the numpy reference (split_jacobian_cases.Ref) and of the general route;
on the regular rows residual_pde of the full assembly is the residual-only call's, byte for byte."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import parity_scale as PS
import split_jacobian_cases as JC
import split_levels_cases as VC
import split_voldev_cases as SC
from cracks_amd import build
from gpu_util import TOL, linf_scaled
from test_glue_mock import GLUE, MOCK, ROOT, _write_problem

SRC = os.path.join(ROOT, "tests", "cpp", "glue_split_route_levels_driver.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "glue_split_route_levels_driver")
GENERAL, JACL, VOLDEV = 0, 13, 3


def build_driver(force=False):
    lib = build.build_native()
    deps = [SRC, GLUE, lib, os.path.join(MOCK, "mock_dealii.h"), os.path.join(ROOT, "tests", "cpp", "glue_driver.cpp")]
    if not force and os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(d) for d in deps):
        return EXE
    libdir = os.path.dirname(lib)
    subprocess.check_call([build.hipcc(), "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", SRC, "-I" + MOCK,
                           "-I" + os.path.join(ROOT, "include"), "-L" + libdir, "-lpfm_hip", "-Wl,-rpath," + libdir, "-o", EXE])
    return EXE


def test_split_route_levels_driver_compiles_against_the_mock_headers():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    assert os.path.exists(build_driver(force=True))
    header = open(os.path.join(ROOT, "include", "pfm_assemble.h")).read()
    assert "PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS = 13" in header and "PFM_SPLIT_ROUTE_LATTICE_ALL_LEVELS = 15" in header
    text = open(GLUE).read()
    assert "pfm_set_split_route(ctx, split_route)" in text and "PFM_SPLIT_ROUTE_LATTICE_JACOBIAN_LEVELS" in text


@pytest.mark.gpu
def test_glue_route_13_with_model_3_reaches_the_context_on_a_refined_mesh(tmp_path):
    exe = build_driver()
    c = SC.block_case(True)
    JC.conditions(c)
    ref = JC.ref(SC.block_case, True)
    lay = c.layout
    d = str(tmp_path)
    to_mock, blocks = _write_problem(c, d, seed=7)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([exe, d, str(VOLDEV), str(GENERAL), str(JACL)], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "glue_split_route_levels_driver: OK" in r.stdout, r.stdout + r.stderr
    read = lambda route, what: np.fromfile(os.path.join(d, f"sl_r{route}_{what}.bin"))
    ig, il = read(GENERAL, "info"), read(JACL, "info")
    print(f"glue split route levels {c.name}: info general {list(ig)}, route 13 {list(il)}")
    reg = VC.regular_rows(c.mesh)
    assert list(ig[:5]) == [0.0, 0.0, 0.0, -1.0, 3.0]
    assert list(il[:3]) == [13.0, 1.0, 1.0] and il[4] == 3.0 and list(il[5:]) == list(ig[5:]) == [float(reg.sum()), float(VC.general_cells(c.mesh, reg).sum())]
    assert 0 < il[3] <= VC.rows_owning_a_cell(c.mesh, reg).size
    # the reference in the mock's numbering, block by block on the mock's pattern
    rows = np.repeat(np.arange(lay.n_dofs), np.diff(ref.A.indptr))
    R = sp.csr_matrix((ref.A.data, (to_mock[rows], to_mock[ref.A.indices])), shape=ref.A.shape)
    R.sort_indices()
    nu = lay.n_u
    cut = ((0, nu), (nu, lay.n_dofs))
    want = [R[r0:r1, c0:c1].tocsr() for (r0, r1) in cut for (c0, c1) in cut]
    out = {}
    for route in (GENERAL, JACL):
        vals = [read(route, f"val{b}") for b in range(4)]
        for b in range(4):
            want[b].sort_indices()
            assert (want[b].indptr == blocks[b].indptr).all() and (want[b].indices == blocks[b].indices).all() and vals[b].size == want[b].nnz
        e = (max(linf_scaled(v, w.data) for v, w in zip(vals, want) if v.size), linf_scaled(read(route, "full")[to_mock], ref.pde),
             linf_scaled(read(route, "pde")[to_mock], ref.pde))
        print(f"glue split route levels, route {route}: matrix {e[0]:.2e}, residual of the full assembly {e[1]:.2e}, residual-only {e[2]:.2e}")
        assert max(e) < TOL
        PS.assert_blocks(vals, [w.data for w in want], TOL, f"glue split route levels, route {route} against the reference", list(PS.BLOCKS))
        for what in ("full", "pde"):
            PS.assert_parts(read(route, what)[to_mock], ref.pde, PS.is_phi(lay), TOL, f"glue split route levels, route {route}, {what}")
        assert not vals[1].any()  # the structurally zero (u,phi) block
        out[route] = vals
    PS.assert_blocks(out[JACL], out[GENERAL], TOL, "glue split route levels, route 13 against the general route", list(PS.BLOCKS))
    dofs = lay.dof(np.repeat(np.nonzero(reg)[0], 4), np.tile(np.arange(4), int(reg.sum())))
    full, pde = read(JACL, "full")[to_mock], read(JACL, "pde")[to_mock]
    assert full[dofs].tobytes() == pde[dofs].tobytes(), "regular rows: the Jacobian call's residual_pde is the line search's"
