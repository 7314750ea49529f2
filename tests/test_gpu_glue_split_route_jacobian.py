"""PfmGlue::split_route = PFM_SPLIT_ROUTE_LATTICE_JACOBIAN with split_model = PFM_SPLIT_VOLDEV of glue/cracks_gpu_assemble.cc
through the mock of tests/test_glue_mock.py (tests/cpp/glue_split_route_jacobian_driver.cpp), on one rank: the route reaches the
context (pfm_ctx_split_route_info answers 5, and where the library runs the mesh as a box, that the full assembly takes the
lattice kernels and how many cells are compressed), and the matrix and residual of the full assembly equal those of the general
route -- which tests/test_gpu_split_voldev.py holds to the oracle's numpy reference -- at the 1e-12 bar, block by block, and the
numpy reference's residual.  Where the library runs the mock's mesh as an overlay (one level lattice, no general cells) the full
assembly is the general route's byte for byte and the info call says so."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import parity_scale as PS
import split_jacobian_cases as JC
import split_lattice_cases as LC
from cracks_amd import build, capi
from gpu_util import TOL, linf_scaled
from test_glue_mock import GLUE, MOCK, ROOT, _write_problem

SRC = os.path.join(ROOT, "tests", "cpp", "glue_split_route_jacobian_driver.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "glue_split_route_jacobian_driver")


def build_driver(force=False):
    lib = build.build_native()
    deps = [SRC, GLUE, lib, os.path.join(MOCK, "mock_dealii.h"), os.path.join(ROOT, "tests", "cpp", "glue_driver.cpp")]
    if not force and os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(d) for d in deps):
        return EXE
    libdir = os.path.dirname(lib)
    subprocess.check_call([build.hipcc(), "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", SRC, "-I" + MOCK,
                           "-I" + os.path.join(ROOT, "include"), "-L" + libdir, "-lpfm_hip", "-Wl,-rpath," + libdir, "-o", EXE])
    return EXE


def test_split_route_jacobian_driver_compiles_against_the_mock_headers():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    assert os.path.exists(build_driver(force=True))
    header = open(os.path.join(ROOT, "include", "pfm_assemble.h")).read()
    assert "PFM_SPLIT_ROUTE_LATTICE_JACOBIAN = 5" in header and "PFM_SPLIT_ROUTE_LATTICE_ALL = 7" in header


@pytest.mark.gpu
def test_glue_route_5_with_model_3_reaches_the_context(tmp_path):
    exe = build_driver()
    blocked, solver = LC.LINE_SEARCH[0]
    c = LC.line_search_case(blocked, solver)
    JC.conditions(c)
    ref = JC.ref(LC.line_search_case, blocked, solver)
    d = str(tmp_path)
    to_mock, _ = _write_problem(c, d, seed=7)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    general, jac = capi.SPLIT_ROUTE_GENERAL, capi.SPLIT_ROUTE_LATTICE_JACOBIAN
    r = subprocess.run([exe, d, str(capi.SPLIT_VOLDEV), str(general), str(jac)], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "glue_split_route_jacobian_driver: OK" in r.stdout, r.stdout + r.stderr
    read = lambda route, what: np.fromfile(os.path.join(d, f"sj_r{route}_{what}.bin"))
    ig, ij = read(general, "info"), read(jac, "info")
    print(f"glue split route jacobian {c.name}: info general {list(ig)}, route 5 {list(ij)}")
    assert list(ig[:4]) == [0.0, 0.0, 0.0, -1.0] and list(ij[:2]) == [5.0, 1.0] and ig[4] == ij[4] and ij[4] in (1.0, 3.0)
    blocks = [0, 1, 2, 3] if blocked else [0]
    vg, vj = [read(general, f"val{b}") for b in blocks], [read(jac, f"val{b}") for b in blocks]
    for route in (general, jac):
        e = (linf_scaled(read(route, "full")[to_mock], ref.pde), linf_scaled(read(route, "pde")[to_mock], ref.pde))
        print(f"glue split route jacobian {route} {c.name}: residual of the full assembly {e[0]:.2e}, residual-only {e[1]:.2e}")
        assert max(e) < TOL
    if ij[4] == 1.0:  # a box: the full assembly on the lattice kernels
        assert ij[2] == 1.0 and 0 < ij[3] <= c.mesh.n_cells
        assert all(a.size == b.size and a.size > 0 for a, b in zip(vj, vg))
        e = max(linf_scaled(a, b) for a, b in zip(vj, vg))
        print(f"glue split route jacobian {c.name}: matrix of route 5 against the general route {e:.2e}")
        assert e < TOL
        PS.assert_blocks(vj, vg, TOL, "glue split route jacobian, route 5 against the general route", [PS.BLOCKS[b] for b in blocks] if blocked else None)
        assert not vj[1].any() if blocked else True  # the structurally zero (u,phi) block
        assert read(jac, "full").tobytes() == read(jac, "pde").tobytes()  # the Jacobian call's residual is the line search's
    else:  # the one level lattice of an overlay: the full assembly keeps the general family
        assert list(ij[2:4]) == [0.0, -1.0]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(vj, vg)) and read(general, "full").tobytes() == read(jac, "full").tobytes()
