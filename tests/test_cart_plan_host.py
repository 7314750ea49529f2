"""The plan of a cartesian assembly and its tile geometry (cracks_amd/csrc/pfm_cart_plan.h) as a stand-alone host program
under AddressSanitizer and UBSan (tests/cpp/cart_plan_main.cpp): tile grids and chunk lengths on boxes at the edges of every
kernel's tile, the boundary-tile lists of a partitioned rank against a node-by-node ghost test, and the routing of every
combination of dimension, phase, scheme, material, layout, box and switch against the literal tables of the launchers as
they were before there was a plan.  The header includes the HIP runtime's API header (streams in the launchers'
declarations), so hipcc builds the program, host side only, with the sanitizers on the host pass; it makes no HIP call,
needs no GPU and is not loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "cart_plan_main.cpp")
HDR_DIR = os.path.join(ROOT, "cracks_amd", "csrc")
SWITCHES = ("PFM_RES_KERNEL", "PFM_JAC_SEQUENTIAL", "PFM_UU_CLK", "PFM_PHI_CLK", "PFM_UU_ZC", "PFM_PHI_ZC", "PFM_RES_ZC", "PFM_RES2_ZC",
            "PFM_RES_NO_TRANSFERS", "PFM_RES_NO_WIDE_TRANSFERS", "PFM_CART2D_ONE_LAUNCH")


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def test_switch_header_has_no_hip_include():
    text = open(os.path.join(HDR_DIR, "pfm_switches.h")).read()
    includes = [ln for ln in text.splitlines() if ln.lstrip().startswith("#include")]
    assert includes and not any("hip" in ln or "pfm_" in ln for ln in includes)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cc = _hipcc()
    if cc is None:
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("cart_plan") / "cart_plan_main")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    cmd = [cc, "-std=c++17", "-O1", "-g", "-x", "hip", "--cuda-host-only", "-I" + HDR_DIR]
    for f in san:
        cmd += ["-Xarch_host", f]
    subprocess.check_call(cmd + ["-c", SRC, "-o", exe + ".o"])
    subprocess.check_call([cc] + san + [exe + ".o", "-o", exe])
    return exe


@pytest.mark.parametrize("once", [{}, {"PFM_RES_KERNEL": "1"}, {"PFM_JAC_SEQUENTIAL": "1"}, {"PFM_UU_CLK": "1", "PFM_PHI_CLK": "1"},
                                  {"PFM_PHI_CLK": "2"}], ids=lambda e: "+".join(e) or "default")
def test_plan_and_geometry_under_sanitizers(program, once):
    """`once`: the switches that are read once per process, hence one run of the program each"""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(once)
    r = subprocess.run([program], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cart_plan: OK" in r.stdout and "FAIL" not in r.stdout
