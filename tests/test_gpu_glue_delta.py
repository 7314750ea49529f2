"""The opt-in switch PfmGlue::delta_values of glue/cracks_gpu_assemble.cc through the mock of tests/test_glue_mock.py
(tests/cpp/glue_delta_driver.cpp): assemble() twice within a time step, only the solution changed.  What the glue leaves
in the "Epetra" value arrays equals the oracle at the tolerance of the other glue tests, and equals -- bit for bit -- what
a second glue instance with the switch off leaves in its own arrays."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import cases
import oracle_api as O
from cracks_amd import build
from cracks_amd import mesh as M
from delta_cases import box_case, second_solution, with_active_phi
from gpu_util import linf_scaled
from test_glue_mock import GLUE, MOCK, ROOT, TOL, _write_problem

SRC = os.path.join(ROOT, "tests", "cpp", "glue_delta_driver.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "glue_delta_driver")


def build_driver(force=False):
    lib = build.build_native()
    deps = [SRC, GLUE, lib, os.path.join(MOCK, "mock_dealii.h"), os.path.join(ROOT, "tests", "cpp", "glue_driver.cpp")]
    if not force and os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(d) for d in deps):
        return EXE
    libdir = os.path.dirname(lib)
    subprocess.check_call([build.hipcc(), "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", SRC, "-I" + MOCK,
                           "-I" + os.path.join(ROOT, "include"), "-L" + libdir, "-lpfm_hip", "-Wl,-rpath," + libdir, "-o", EXE])
    return EXE


def test_delta_driver_compiles_against_the_mock_headers():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    assert os.path.exists(build_driver(force=True))
    text = open(GLUE).read()
    assert "delta_values" in text and "pfm_values_to_host_delta" in text


CASES = [
    ("sneddon_3d_blocked", lambda: with_active_phi(cases.perturbed(cases.kat_sneddon_3d(5)))),
    ("box_2d_blocked", lambda: box_case(2, (9, 7), True)),
    ("miehe_slit_interleaved", lambda: cases.perturbed(cases.kat_miehe_shear_1())),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,maker", CASES, ids=[c[0] for c in CASES])
def test_glue_with_delta_values_matches_the_oracle_and_the_plain_glue(name, maker, tmp_path):
    exe = build_driver()
    c = maker()
    d = str(tmp_path)
    to_mock, blocks = _write_problem(c, d, seed=7)
    sol2 = second_solution(c)
    y = np.empty_like(sol2)
    y[to_mock] = sol2
    y.tofile(os.path.join(d, "sol2.bin"))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "glue_delta_driver: OK" in r.stdout, r.stdout + r.stderr
    mesh, lay = c.mesh, c.layout
    rp, ci = M.dof_sparsity(mesh, lay)
    stats = np.fromfile(os.path.join(d, "out_delta_stats.bin"), np.int64).reshape(2, 10)
    for prefix, sol in (("out_first_val", c.sol), ("out_val", sol2)):
        ref = O.assemble(mesh, lay, c.params, sol, c.old, c.oldold, c.cu, c.ch, False, rp, ci, c.cell_lambda, c.cell_mu)
        assert ref.err == 0
        A_ref = sp.csr_matrix((ref.values, ci, rp), shape=(lay.n_dofs,) * 2)
        mats = {b: sp.csr_matrix((np.fromfile(os.path.join(d, f"{prefix}{b}.bin")), B.indices, B.indptr), shape=B.shape) for b, B in blocks.items()}
        A_mock = (sp.bmat([[mats[0], mats[1]], [mats[2], mats[3]]], format="csr") if lay.blocked else mats[0]).tocsr()
        assert np.isfinite(A_mock.data).all() and np.abs(A_mock.data).max() < 1e70  # every value was overwritten (-7e77 marker)
        A = A_mock[to_mock][:, to_mock].tocsr()
        A.sort_indices()
        A_ref.sort_indices()
        assert (A.indptr == A_ref.indptr).all() and (A.indices == A_ref.indices).all()
        assert linf_scaled(A.data, A_ref.data) < TOL, prefix
    for b in blocks:
        got = np.fromfile(os.path.join(d, f"out_val{b}.bin")).view(np.uint64)
        plain = np.fromfile(os.path.join(d, f"out_plain_val{b}.bin")).view(np.uint64)
        assert np.array_equal(got, plain), b
    # the first call ships everything but the (u,phi) block, which the glue's page-locked array has cleared on the host
    chunk = 4096  # the default chunk size (pfm_values_delta_info; the glue does not configure it)
    n_chunks = [-(-B.nnz * 8 // chunk) for b, B in sorted(blocks.items())]
    assert stats[0][3] == sum(n_chunks) and stats[0][2] == sum(n for b, n in enumerate(n_chunks) if not (lay.blocked and b == 1))
    assert stats[1][3] == stats[0][3]
    if c.params.decompose_stress_matrix == 0:  # the displacement rows stay: part of the matrix stays on the device
        assert 0 < stats[1][0] < stats[1][1]
