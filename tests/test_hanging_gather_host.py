"""The list builder of the ordered gather (pfm::hang_gather_lists in cracks_amd/csrc/pfm_mesh_plan.cpp: records -> rows / ptr /
list / offsets) as a stand-alone host program under AddressSanitizer and UBSan (tests/cpp/hang_gather_main.cpp), on hand-made
records of quads (KCMP 7) and hexes (KCMP 13).  The program checks: rows ascending; the entries of a row ascending by (cell,
index); every (cell, owned resolved node) and (cell, owned hanging vertex) listed exactly once; ghost nodes never listed;
offsets equal to the prefix sum of R * R * KCMP; a record with R = 0xff refused.  No HIP call, no GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cracks_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "cpp", "hang_gather_main.cpp")


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("hang_gather") / "hang_gather_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                           "-I" + CSRC, MAIN, os.path.join(CSRC, "pfm_mesh_plan.cpp"), os.path.join(CSRC, "pfm_host_pool.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_the_list_builder_keeps_its_promises(output):
    assert "hang_gather: OK" in output and "FAIL" not in output


def test_both_dimensions_were_exercised(output):
    """4 records of R = 5, 4, 6, 16: 25 + 16 + 36 + 256 = 333 node pairs, times KCMP doubles of scratch."""
    lines = [l for l in output.splitlines() if l.startswith("nv ")]
    assert len(lines) == 2
    assert lines[0].startswith("nv 4 kcmp 7:") and lines[0].endswith(f"{333 * 7} scratch doubles")
    assert lines[1].startswith("nv 8 kcmp 13:") and lines[1].endswith(f"{333 * 13} scratch doubles")


def test_the_host_side_calls_the_builder_it_tests():
    """ensure_hang_gather has no list code of its own left: it hands the records to pfm::hang_gather_lists."""
    text = open(os.path.join(CSRC, "pfm_host.cpp")).read()
    start = text.index("bool ensure_hang_gather(pfm_ctx *c)\n")  # its definition, up to the next one of the file
    body = text[start:text.index("int pfm_ctx_destroy(pfm_ctx *c)\n", start)]
    assert "pfm::hang_gather_lists(" in body and "HgEntry{(int32_t)(hc * 32" not in body
