"""PfmGlue::split_route = PFM_SPLIT_ROUTE_LATTICE_ANY with split_model = PFM_SPLIT_SPECTRAL of glue/cracks_gpu_assemble.cc through
the mock of tests/test_glue_mock.py (tests/cpp/glue_split_route_any_driver.cpp), on one rank: the route reaches the context
(pfm_ctx_split_route answers 3 and lattice_residual = 1), the residual-only assembly equals the numpy reference of the spectral
law, and the full assembly's residual is the general route's byte for byte; with route 0 the context answers 0 and 0."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import split_lattice_spectral_cases as XC
from cracks_amd import build, capi
from gpu_util import TOL, linf_scaled
from test_glue_mock import GLUE, MOCK, ROOT, _write_problem

SRC = os.path.join(ROOT, "tests", "cpp", "glue_split_route_any_driver.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "glue_split_route_any_driver")


def build_driver(force=False):
    lib = build.build_native()
    deps = [SRC, GLUE, lib, os.path.join(MOCK, "mock_dealii.h"), os.path.join(ROOT, "tests", "cpp", "glue_driver.cpp")]
    if not force and os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(d) for d in deps):
        return EXE
    libdir = os.path.dirname(lib)
    subprocess.check_call([build.hipcc(), "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", SRC, "-I" + MOCK,
                           "-I" + os.path.join(ROOT, "include"), "-L" + libdir, "-lpfm_hip", "-Wl,-rpath," + libdir, "-o", EXE])
    return EXE


def test_split_route_any_driver_compiles_against_the_mock_headers():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    assert os.path.exists(build_driver(force=True))
    assert "PFM_SPLIT_ROUTE_LATTICE_ANY = 3" in open(os.path.join(ROOT, "include", "pfm_assemble.h")).read()


@pytest.mark.gpu
def test_glue_route_3_with_model_1_reaches_the_context(tmp_path):
    exe = build_driver()
    blocked, solver = XC.LINE_SEARCH[0]
    c = XC.line_search_case(blocked, solver)
    ref = XC.ref(XC.line_search_case, blocked, solver)
    d = str(tmp_path)
    to_mock, _ = _write_problem(c, d, seed=7)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    general, lattice = capi.SPLIT_ROUTE_GENERAL, capi.SPLIT_ROUTE_LATTICE_ANY
    r = subprocess.run([exe, d, str(capi.SPLIT_SPECTRAL), str(general), str(lattice)], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "glue_split_route_any_driver: OK" in r.stdout, r.stdout + r.stderr
    read = lambda route, what: np.fromfile(os.path.join(d, f"sr_r{route}_{what}.bin"))
    assert list(read(general, "info"))[:2] == [0.0, 0.0] and list(read(lattice, "info"))[:2] == [3.0, 1.0]
    # (the mock hands the vertices over in a permuted order and without a box hint: the library finds the lattice by itself, as
    # the box or as the one level lattice of an overlay without general cells)
    assert read(general, "info")[2] == read(lattice, "info")[2] and read(lattice, "info")[2] in (1.0, 3.0)
    for route in (general, lattice):
        e = (linf_scaled(read(route, "pde")[to_mock], ref.pde), linf_scaled(read(route, "tot")[to_mock], ref.tot),
             linf_scaled(read(route, "full")[to_mock], ref.pde))
        print(f"glue split route {route} {c.name}: residual-only {e[0]:.2e} / {e[1]:.2e}, full {e[2]:.2e}")
        assert max(e) < TOL
    assert read(general, "full").tobytes() == read(lattice, "full").tobytes()  # the full assembly does not follow the route
