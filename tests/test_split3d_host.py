"""cracks_amd/csrc/pfm_split3.h -- the statements the 3-D SPLIT kernels run per q-point -- as a stand-alone host program
under AddressSanitizer and UBSan (tests/cpp/split3_main.cpp), compared with cracks_amd/split3d.py: mixed-sign random
tensors of magnitude 1e-8 ... 1e4, rotated tensors with prescribed spectra, repeated eigenvalues, exactly diagonal tensors
and zero.  hipcc builds the program host side only (the header's functions are __host__ __device__); it makes no HIP call,
needs no GPU and is not loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from cracks_amd.split3d import spectral_split, spectral_tangent, voigt6, voigt21

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "split3_main.cpp")
HDR_DIR = os.path.join(ROOT, "cracks_amd", "csrc")


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    cc = _hipcc()
    if cc is None:
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("split3") / "split3_main")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    cmd = [cc, "-std=c++17", "-O1", "-g", "-x", "hip", "--cuda-host-only", "-I" + HDR_DIR]
    for f in san:
        cmd += ["-Xarch_host", f]
    subprocess.check_call(cmd + ["-c", SRC, "-o", exe + ".o"])
    subprocess.check_call([cc] + san + [exe + ".o", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_the_program_keeps_the_headers_promises(output):
    assert "split3: OK" in output and "FAIL" not in output


def test_header_against_the_numpy_law(output):
    """Bar: 1e-12 relative to (lambda + 2 mu) |E| for the stresses and to (lambda + 2 mu) for the tangents.  The random
    tensors have eigenvalue gaps of the order of |E|; the tangent weights theta_ij are quotients of eigenvalue differences,
    exact (0 or 1) for pairs of one sign."""
    n = 0
    kinds = set()
    worst_s = worst_c = 0.0
    for line in output.splitlines():
        if not line.startswith("case "):
            continue
        head, e, sp, sm, cp, cm = [s.split() for s in line.split("|")]
        name, lam, mu = head[1], float.fromhex(head[2]), float.fromhex(head[3])
        f = lambda xs: np.array([float.fromhex(x) for x in xs])
        e, sp, sm, cp, cm = f(e), f(sp), f(sm), f(cp), f(cm)
        assert len(e) == 6 and len(sp) == 6 and len(sm) == 6 and len(cp) == 21 and len(cm) == 21
        E = np.array([[e[0], e[3], e[4]], [e[3], e[1], e[5]], [e[4], e[5], e[2]]])
        sp_ref, sm_ref = spectral_split(E, lam, mu)
        Cp_ref, Cm_ref = spectral_tangent(E, lam, mu)
        mod = lam + 2 * mu
        s_scale = mod * max(np.abs(E).max(), 1e-300)
        es = max(np.abs(sp - voigt6(sp_ref)).max(), np.abs(sm - voigt6(sm_ref)).max()) / s_scale
        ec = max(np.abs(cp - voigt21(Cp_ref)).max(), np.abs(cm - voigt21(Cm_ref)).max()) / mod
        worst_s, worst_c = max(worst_s, es), max(worst_c, ec)
        assert es < 1e-12, (name, es)
        assert ec < 1e-12, (name, ec)
        n += 1
        kinds.add(name.split("_")[0])
    print(f"{n} tensors, worst deviation: stress {worst_s:.2e}, tangent {worst_c:.2e}")
    assert n >= 70 and kinds == {"random", "rotated", "repeated", "diagonal", "zero"}
