"""The host scatter of the delta transfer (cracks_amd/csrc/pfm_delta_host.h) as a stand-alone program under
AddressSanitizer and UBSan (tests/cpp/delta_scatter_main.cpp): tail chunk shorter than the chunk size, destination
offset by 8 bytes, empty chunk list, fewer chunks than threads, 1 and 16 threads, and every destination byte outside the
listed chunks unchanged.  The header is plain C++17 without a HIP include, so the host compiler builds it alone; the
sanitizers see this program only -- nothing that is loaded into Python or runs on the GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "delta_scatter_main.cpp")
HDR_DIR = os.path.join(ROOT, "cracks_amd", "csrc")


def test_header_has_no_hip_include():
    text = open(os.path.join(HDR_DIR, "pfm_delta_host.h")).read()
    includes = [ln for ln in text.splitlines() if ln.lstrip().startswith("#include")]
    assert includes and not any("hip" in ln or "pfm_" in ln for ln in includes)


def test_scatter_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "delta_scatter_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                           "-I" + HDR_DIR, SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "delta_scatter: OK" in r.stdout and "FAIL" not in r.stdout
