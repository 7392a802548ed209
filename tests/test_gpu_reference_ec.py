"""INTEGRATION.md Option A, run: the reference's unchanged EC classes on the GPU's host tier, and the facade's bytes.

oracle/_ref/ref_ec_gpu is the reference's own erasure_code.cpp / rs.cpp / lrc.cpp / pc.cpp compiled against
include/jerasure_shim/ and linked with libecg.so: every jerasure_matrix_encode / jerasure_matrix_decode its classes
make goes to the HIP kernels.  One child process answers the whole request of tests/reference_ec_cases.py (less the
cases the reference exits on); every digest it writes must equal tests/golden/reference_ec.json, which the same classes
wrote on the CPU.  The same calls through ecg.py's ErasureCode facade must give the same bytes: on the host tier for
every code, on the device tier for the (4,1,4,1) product codes and Azure-LRC(12,2,2).

The binary is built only where the reference's sources are (oracle/Makefile); a checkout built elsewhere skips.
"""
import json
import os
import subprocess
import time

import pytest

import reference_ec_cases as C
import reference_ec_replay as R

pytestmark = pytest.mark.gpu

if not os.path.exists(C.REF_GPU):
    pytest.skip("oracle/_ref/ref_ec_gpu did not travel here (it is built only where the reference's sources are)",
                allow_module_level=True)

RECORD = json.load(open(C.RECORD))
CODES = RECORD["codes"]
IDS = [c["name"] for c in CODES]
INPUT = C.input_bytes()
# The child took 5.36 s of wall time for the whole request (40735 answers) on an MI355X; ten times that.
CHILD_TIMEOUT = 54
BAD_ENDS = (134, 139, -6, -11)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return torch


@pytest.fixture(scope="module")
def requests(oracle):
    """Every code's recorded request.  The record keeps the requests' digests, not their text: the partial lines come
    from the oracle's plans (CPU), and the digest says they are the reference's."""
    out = []
    for c in CODES:
        lines = R.request_of(c, R.OracleSubject(c), INPUT, with_bytes=False)[0]
        assert C.fold(lines, [])["request_sha256"] == c["request_sha256"], c["name"]
        out.append(lines)
    return out


@pytest.fixture(scope="module")
def child(torch_cuda, requests, tmp_path_factory):
    """The one GPU process of the reference binary: a fresh child over the whole request (less the cases the reference
    exits on).  Returns the answers per code, or the reason there are none; a child that aborted, faulted or ran into
    its time limit is never started again, and no test of this module touches the GPU after it."""
    kept = [C.kept_lines(ls, c) for ls, c in zip(requests, CODES)]
    lines = [l for ls in kept for l in ls]
    work = str(tmp_path_factory.mktemp("ref_ec_gpu"))
    t0 = time.time()
    try:
        got, rc, err = C.run_driver(C.REF_GPU, lines, work, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        res = os.path.join(work, "result.jsonl")
        done = sum(1 for _ in open(res)) if os.path.exists(res) else 0
        return {"error": "ref_ec_gpu ran into its %d s limit after %d of %d answers; stderr: %s" % (
            CHILD_TIMEOUT, done, len(lines), (e.stderr or b"")[-2000:])}
    wall = time.time() - t0
    print("ref_ec_gpu: %d answers in %.2f s" % (len(got), wall))
    if rc != 0 or len(got) != len(lines):
        return {"error": "ref_ec_gpu ended with %d%s after %d of %d answers (next: %r); stderr: %s" % (
            rc, " (abort or fault)" if rc in BAD_ENDS else "", len(got), len(lines),
            lines[len(got)] if len(got) < len(lines) else None, err[-2000:])}
    it = iter(got)
    return {"error": None, "wall": wall,
            "answers": [C.with_exits(ls, c, [next(it) for _ in k]) for ls, c, k in zip(requests, CODES, kept)]}


def _usable(child):
    if child["error"]:
        pytest.fail(child["error"])


@pytest.mark.parametrize("i", range(len(CODES)), ids=IDS)
def test_reference_classes_on_gpu_match_record(child, requests, i):
    """Every answer the reference's classes gave through the shim and libecg equals what they gave on the CPU."""
    _usable(child)
    got = C.fold(requests[i], child["answers"][i])
    for key, value in got.items():
        assert value == CODES[i][key], key


def _device_tier(code):
    return code["exhaustive"] or (code["type"] == 2 and [code["params"][f] for f in "klg"] == [12, 2, 2])


@pytest.mark.parametrize("i", range(len(CODES)), ids=IDS)
def test_facade_bytes_match_record(ecg, child, requests, i):
    """The same calls through the ErasureCode facade: every answer, bytes included, equals the record."""
    _usable(child)
    code = CODES[i]
    for mem in [R.HostBlocks] + ([R.DeviceBlocks] if _device_tier(code) else []):
        got = R.folded(code, requests[i], R.replay(R.FacadeSubject(code), requests[i], INPUT, mem=mem))
        for key, value in got.items():
            assert value == code[key], (mem.__name__, key)
