"""The volumetric-deviatoric law of cracks_amd/csrc/pfm_split3.h (voldev, voldev_tangent_a, voldev_stress3, voldev_tangent3:
the statements the PFM_SPLIT_VOLDEV instantiations of k_assemble_general run per q-point) as a stand-alone host program under
AddressSanitizer and UBSan (tests/cpp/split_voldev_main.cpp), compared with cracks_amd/split3d.py: random tensors of
magnitude 1e-8 ... 1e4 with tr E of both signs, tensors with tr E exactly 0, zero, pure compression and dilation.  hipcc
builds the program host side only; it makes no HIP call, needs no GPU and is not loaded into Python (the pattern of
tests/test_split3d_host.py).

Measured agreement (x86-64 host, 92 tensors: 36 with tr E > 0, 34 with tr E < 0, 22 with tr E == 0): stresses 3.5e-16
(lambda + 2 mu) |E|, tangents and the pair (a, b) 1.4e-16 (lambda + 2 mu)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from cracks_amd.split3d import voigt6, voigt21, voldev_split, voldev_tangent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "split_voldev_main.cpp")
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
    exe = str(tmp_path_factory.mktemp("split_voldev") / "split_voldev_main")
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
    assert "split_voldev: OK" in output and "FAIL" not in output


def test_header_against_the_numpy_law(output):
    """Bar: 1e-14 relative to (lambda + 2 mu) |E| for the stresses and to (lambda + 2 mu) for the tangents and for (a, b):
    both sides are a dozen operations in double precision on numbers of that size, without cancellation beyond the
    deviator's tr E / 3 -- a hundred times the unit roundoff."""
    n = n_pos = n_neg = n_zero = 0
    kinds = set()
    worst_s = worst_c = 0.0
    for line in output.splitlines():
        if not line.startswith("case "):
            continue
        head, e, sp, sm, cp, cm, ab = [s.split() for s in line.split("|")]
        name = head[1]
        lam, mu, g, d = [float.fromhex(x) for x in head[2:6]]
        f = lambda xs: np.array([float.fromhex(x) for x in xs])
        e, sp, sm, cp, cm, ab = f(e), f(sp), f(sm), f(cp), f(cm), f(ab)
        assert len(e) == 6 and len(sp) == 6 and len(sm) == 6 and len(cp) == 21 and len(cm) == 21 and len(ab) == 2
        E = np.array([[e[0], e[3], e[4]], [e[3], e[1], e[5]], [e[4], e[5], e[2]]])
        tr = np.trace(E)
        n_pos, n_neg, n_zero = n_pos + (tr > 0), n_neg + (tr < 0), n_zero + (tr == 0)
        sp_ref, sm_ref = voldev_split(E, lam, mu)
        Cp_ref, Cm_ref = voldev_tangent(E, lam, mu)
        mod = lam + 2 * mu
        s_scale = mod * max(np.abs(E).max(), 1e-300)
        es = max(np.abs(sp - voigt6(sp_ref)).max(), np.abs(sm - voigt6(sm_ref)).max()) / s_scale
        ec = max(np.abs(cp - voigt21(Cp_ref)).max(), np.abs(cm - voigt21(Cm_ref)).max()) / mod
        # the isotropic pair the kernel keeps per q-point
        h = 0.0 if tr < 0.0 else 1.0
        a_ref = lam * (g * h + d * (1 - h)) - (2 * mu / 3) * (1 - h) * (g - d)
        ec = max(ec, abs(ab[0] - a_ref) / mod, abs(ab[1] - mu * g) / mod)
        worst_s, worst_c = max(worst_s, es), max(worst_c, ec)
        assert es < 1e-14, (name, es)
        assert ec < 1e-14, (name, ec)
        n += 1
        kinds.add(name.split("_")[0])
    print(f"{n} tensors ({n_pos} with tr E > 0, {n_neg} < 0, {n_zero} == 0), worst deviation: stress {worst_s:.2e}, tangent {worst_c:.2e}")
    assert n >= 90 and kinds == {"random", "traceless", "zero", "isotropic"}
    assert n_pos >= 20 and n_neg >= 20 and n_zero >= 22
