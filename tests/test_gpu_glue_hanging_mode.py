"""PfmGlue::hanging_mode of glue/cracks_gpu_assemble.cc through the mock of tests/test_glue_mock.py
(tests/cpp/glue_hanging_mode_driver.cpp), on one rank: with hanging_mode = PFM_HANGING_MODE_GATHER the mode reaches the context
(pfm_ctx_hanging_info answers GATHER, gathered, no atomic adds), the slit mesh refined across its tip -- duplicated nodes,
hanging nodes, the reference's stress split -- assembles to the oracle's values in both layouts, and two rounds of assemble()
calls give the same bytes."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from cracks_amd import build
from cracks_amd import mesh as M
from gpu_util import TOL, linf_scaled, oracle, reference_parity, total_matrix
from test_glue_mock import GLUE, MOCK, ROOT, _write_problem

SRC = os.path.join(ROOT, "tests", "cpp", "glue_hanging_mode_driver.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "glue_hanging_mode_driver")


def build_driver(force=False):
    lib = build.build_native()
    deps = [SRC, GLUE, lib, os.path.join(MOCK, "mock_dealii.h"), os.path.join(ROOT, "tests", "cpp", "glue_driver.cpp")]
    if not force and os.path.exists(EXE) and os.path.getmtime(EXE) > max(os.path.getmtime(d) for d in deps):
        return EXE
    libdir = os.path.dirname(lib)
    subprocess.check_call([build.hipcc(), "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", SRC, "-I" + MOCK,
                           "-I" + os.path.join(ROOT, "include"), "-L" + libdir, "-lpfm_hip", "-Wl,-rpath," + libdir, "-o", EXE])
    return EXE


def test_hanging_mode_driver_compiles_against_the_mock_headers():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    assert os.path.exists(build_driver(force=True))
    text = open(GLUE).read()
    assert "pfm_set_hanging_mode(ctx, hanging_mode)" in text and "int hanging_mode = PFM_HANGING_MODE_DEFAULT" in text


@pytest.mark.gpu
@pytest.mark.parametrize("blocked", [True, False])
def test_glue_hanging_mode_reaches_the_context(blocked, tmp_path):
    from test_gpu_hanging_gather2d import case_of

    exe = build_driver()
    c = case_of("slit_split", blocked)
    lay = c.layout
    d = str(tmp_path)
    to_mock, blocks = _write_problem(c, d, seed=7)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "glue_hanging_mode_driver: OK" in r.stdout, r.stdout + r.stderr
    info = list(np.fromfile(os.path.join(d, "hm_info.bin")))
    assert info[0] == 1.0 and info[1] > 0 and info[2] == 1.0 and info[3] > 0 and info[4] > 0 and info[5] == 0.0
    read = lambda k, what: np.fromfile(os.path.join(d, f"hm_k{k}_{what}.bin"))
    names = ["pde", "tot", "full"] + [f"val{b}" for b in blocks]
    for what in names:  # the same bytes from two assemble() calls
        assert read(0, what).tobytes() == read(1, what).tobytes(), what
    ro, _, _ = oracle(c, True)
    rf, rp, ci = oracle(c, False)
    A_ref = sp.csr_matrix((rf.values, ci, rp), shape=(lay.n_dofs,) * 2)
    mats = {b: sp.csr_matrix((read(0, f"val{b}"), B.indices, B.indptr), shape=B.shape) for b, B in blocks.items()}
    A_mock = (mats[0] if not lay.blocked else sp.bmat([[mats[0], mats[1]], [mats[2], mats[3]]], format="csr")).tocsr()
    assert np.isfinite(A_mock.data).all() and np.abs(A_mock.data).max() < 1e70  # every value was overwritten (-7e77 marker)
    A = A_mock[to_mock][:, to_mock].tocsr()
    A.sort_indices()
    A_ref.sort_indices()
    assert (A.indptr == A_ref.indptr).all() and (A.indices == A_ref.indices).all()
    pde, tot, full = read(0, "pde")[to_mock], read(0, "tot")[to_mock], read(0, "full")[to_mock]
    e = (linf_scaled(A.data, A_ref.data), linf_scaled(full, rf.residual_pde), linf_scaled(pde, ro.residual_pde), linf_scaled(tot, ro.residual_total))
    print(f"glue hanging mode blocked={blocked}: matrix {e[0]:.2e} residual {e[1]:.2e} residual-only {e[2]:.2e} / {e[3]:.2e}")
    assert max(e) < TOL
    reference_parity(lay, c.sol, A, A_ref, [(full, rf.residual_pde, "pde"), (pde, ro.residual_pde, "pde"), (tot, ro.residual_total, "tot")],
                     tag=f"glue hanging mode blocked={blocked}", A_tot=total_matrix(c, A_ref))
