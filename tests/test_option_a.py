"""INTEGRATION.md Option A, checked against the reference's own sources (CPU, this container only).

Option A relinks the reference's unchanged EC layer (project/src/ec/{erasure_code,rs,lrc,pc,utils}.cpp)
against libecg by putting include/jerasure_shim/ first on the include path.  This compiles each of those
files with `g++ -std=c++20 -fsyntax-only` (the reference's own standard, project/CmakeLists.txt) against
the shim headers: every Jerasure call it makes must resolve to a shim declaration with a compatible
signature.  -fsyntax-only writes no object; the build and the run of those sources are oracle/Makefile's
(oracle/_ref/ref_ec_cpu, ref_ec_gpu) and tests/test_reference_ec.py / tests/test_gpu_reference_ec.py's.
/root/reference does not exist on the GPU box, so this test skips there.
"""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/project"
SRCS = ["erasure_code.cpp", "rs.cpp", "lrc.cpp", "pc.cpp", "utils.cpp"]

needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src", "ec")) or not shutil.which("g++"),
                               reason="needs the reference sources and g++ (build container only)")


@needs_ref
@pytest.mark.parametrize("src", SRCS)
def test_reference_ec_source_compiles_against_shim(src):
    cmd = ["g++", "-std=c++20", "-fsyntax-only", "-I", os.path.join(ROOT, "include", "jerasure_shim"),
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(REF, "include", "ec"),
           os.path.join(REF, "src", "ec", src)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]


def test_shim_declares_every_jerasure_call_of_the_reference():
    """The calls are the recorded ones (tests/golden/reference_jerasure_calls.json: names only, per source file), so
    the test needs nothing outside the repository; where the reference sources are present, the record is first
    checked against them."""
    recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_jerasure_calls.json")))["calls"]
    assert sorted(recorded) == sorted(SRCS)
    if os.path.isdir(os.path.join(REF, "src", "ec")):
        for src in SRCS:
            text = open(os.path.join(REF, "src", "ec", src)).read()
            found = set(re.findall(r"\b((?:jerasure|reed_sol|cauchy|galois)_[a-z_0-9]+)\s*\(", text))
            assert found == set(recorded[src]), (src, sorted(found))
    called = set().union(*recorded.values())
    shim = "".join(open(os.path.join(ROOT, "include", "jerasure_shim", f)).read()
                   for f in os.listdir(os.path.join(ROOT, "include", "jerasure_shim")))
    declared = set(re.findall(r"static inline [^(]*?\b((?:jerasure|reed_sol|cauchy|galois)_[a-z_0-9]+)\s*\(", shim))
    assert called, "no Jerasure calls found"
    assert called <= declared, sorted(called - declared)
    # the seven entry points SURVEY.md §8(b) lists
    assert called == {"jerasure_matrix_encode", "jerasure_matrix_decode", "reed_sol_vandermonde_coding_matrix",
                      "cauchy_good_general_coding_matrix", "jerasure_invert_matrix", "jerasure_matrix_multiply",
                      "galois_region_xor"}
