"""The delta update, the parts that need no GPU: libecg_update.so's exports and code object, every argument refusal
with its error text (each returns before any device is touched), the two host helpers against tests/update_plain.py and
the fields of the last launch.  Every test here loads libecg_update.so.
"""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import test_kernel_resources as KR
import update_plain as UP

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
K_MAX_NNZ = 8                                              # update_kernels.hpp kUpdateMaxNnz
OTHERS = ("libecg.so", "libecg_scrub.so", "libecg_locate.so", "libecg_heal.so", "libecg_heal2.so", "libecg_sum.so",
          "libecg_psum.so", "libecg_restore.so")


@pytest.fixture(scope="module")
def update(ecg):
    import ecg_update
    ecg_update.lib()
    return ecg_update


def _err(ecg):
    return ecg.lib().ecg_last_error()


# ---- the library

def test_header_symbols_exported(update):
    hdr = open(os.path.join(ROOT, "include", "ecg_update.h")).read()
    declared = sorted(set(re.findall(r"\b(ecg_update_\w+)\s*\(", hdr)))
    assert len(declared) == 8
    assert sorted(update.EXPORTS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", update.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r" T (ecg_\w+)", out))) == declared
    assert sorted(update._SIG) == declared


def test_needs_libecg_only_and_nothing_needs_it(update):
    lib_dir = os.path.dirname(KR.LIB)
    need = subprocess.run(["readelf", "-d", update.LIB_PATH], capture_output=True, text=True).stdout
    needed = re.findall(r"NEEDED.*\[(libecg[^\]]*)\]", need)
    assert needed == ["libecg.so"], needed
    for so in OTHERS:
        need = subprocess.run(["readelf", "-d", os.path.join(lib_dir, so)], capture_output=True, text=True).stdout
        assert "NEEDED" in need and "libecg_update" not in need, so
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(lib_dir, so)], capture_output=True,
                             text=True).stdout
        assert not re.findall(r" T (ecg_update\w*)", out), so


def test_last_launch_reports_four_fields(update):
    L = update.lib()
    assert L.ecg_update_last_launch(None, 0) == 4
    small = (ctypes.c_int * 3)(*([77] * 3))
    assert L.ecg_update_last_launch(small, 3) == 4 and list(small) == [77] * 3
    full = (ctypes.c_int * 6)(*([77] * 6))
    assert L.ecg_update_last_launch(full, 6) == 4 and list(full)[4:] == [77, 77]
    got = update.last_launch()
    assert list(got) == ["cols_per_wg", "wg_per_record", "R", "max_nnz"]
    assert list(got.values()) == list(full)[:4] and all(v >= 0 for v in got.values())
    hdr = open(os.path.join(ROOT, "include", "ecg_update.h")).read()
    assert re.findall(r"v\[(\d)\] (\w+)", hdr) == [(str(i), name) for i, name in enumerate(got)]
    n = [ctypes.c_longlong(-1), ctypes.c_longlong(-1)]
    assert L.ecg_update_counters(ctypes.byref(n[0]), ctypes.byref(n[1])) == 0 and n[0].value >= 0 and n[1].value >= 0
    assert L.ecg_update_counters(None, None) == 0
    assert update.counters() == {"launches": n[0].value, "records": n[1].value}


@pytest.fixture(scope="module")
def meta(update):
    """Kernel metadata of libecg_update.so's gfx950 code object, read as tests/test_kernel_resources.py reads
    libecg.so's."""
    saved = KR.LIB
    KR.LIB = update.LIB_PATH
    try:
        return KR._metadata()
    finally:
        KR.LIB = saved


def test_code_object_is_the_update_family(meta):
    keys = []
    for s in meta:
        v = re.search(r"gf_update_kernelILi(\d+)ELb([01])ELb([01])EE", s)
        assert v, s
        keys.append(tuple(map(int, v.groups())))
    want = {(nr, inl, vec) for nr in range(1, K_MAX_NNZ + 1) for inl in (0, 1) for vec in (0, 1)}
    assert len(keys) == len(set(keys)) == 32 and set(keys) == want


def test_update_kernels_use_no_scratch_no_lds(meta):
    bad = {n: f for n, f in meta.items() if f.get("private_segment_fixed_size", 0) or f.get("vgpr_spill_count", 0)
           or f.get("sgpr_spill_count", 0)}
    assert not bad, list(bad)[:5]
    assert all(f.get("group_segment_fixed_size", 0) == 0 for f in meta.values())
    assert all(f["kernarg_segment_size"] <= 4096 for f in meta.values())
    # eight parity columns of four dwords, delta and the input beside them: four waves per SIMD at the least
    assert max(f["vgpr_count"] for f in meta.values()) <= 128


# ---- arguments (no GPU is touched: every call returns before the first HIP call)

def test_bad_arguments(ecg, update):
    L, EINVAL = update.lib(), ecg.ECG_EINVAL
    G = (ctypes.c_int * 4)(1, 1, 1, 2)
    src = (ctypes.c_int * 2)(0, 1)
    dst = (ctypes.c_int * 2)(2, 3)
    dev, rec, inp, dl, rep = (ctypes.c_void_p(0x10000 * i) for i in (1, 2, 3, 4, 5))   # never read
    ok = dict(k=2, m=2, G=G, src=src, dst=dst, base=dev, ss=4096, bs=1024, B=64, S=1, mode=0, rec=rec, R=1, ml=64,
              inp=inp, nb=64, dl=None, rep=rep)

    def matrix_batch(**kw):
        a = dict(ok, **kw)
        return L.ecg_update_matrix_batch(a["k"], a["m"], a["G"], a["src"], a["dst"], a["base"], a["ss"], a["bs"],
                                         a["B"], a["S"], a["mode"], a["rec"], a["R"], a["ml"], a["inp"], a["nb"],
                                         a["dl"], a["rep"], None)

    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    for kw, text in ((dict(k=0), b"k_in = 0"), (dict(m=0), b"m_out = 0"), (dict(k=-3), b"k_in = -3"),
                     (dict(G=None), b"coef is NULL"), (dict(src=None), b"src_ids is NULL"),
                     (dict(dst=None), b"dst_ids is NULL"), (dict(base=None), b"base is NULL"),
                     (dict(rec=None), b"d_records is NULL"), (dict(inp=None), b"d_in is NULL"),
                     (dict(rep=None), b"d_report is NULL"), (dict(B=-1), b"B = -1"), (dict(S=-1), b"S = -1"),
                     (dict(R=-1), b"R = -1"), (dict(ml=-1), b"max_len = -1"), (dict(nb=-1), b"in_bytes = -1"),
                     (dict(B=1 << 31, ml=0), b"not below 2^31"), (dict(ml=65), b"max_len = 65 exceeds B = 64"),
                     (dict(mode=2), b"mode = 2"), (dict(mode=-1), b"mode = -1"),
                     (dict(mode=1, dl=dl), b"ECG_UPDATE_DELTA"),
                     (dict(rec=ctypes.c_void_p(0x20004)), b"8-byte aligned"),
                     (dict(src=ints(0, -1)), b"negative id"), (dict(dst=ints(-2, 3)), b"negative id"),
                     (dict(src=ints(1, 1)), b"src_ids names block 1 twice"),
                     (dict(dst=ints(3, 3)), b"dst_ids names block 3 twice"),
                     (dict(dst=ints(2, 0)), b"block 0 is both"),
                     (dict(R=(1 << 31) - 1, B=1 << 20, ml=1 << 20), b"2^31 - 1 workgroups")):
        assert matrix_batch(**kw) == EINVAL, kw
        assert _err(ecg).startswith(b"update: ") and text in _err(ecg), (kw, _err(ecg))
    assert matrix_batch(R=0) == 0 and matrix_batch(R=0, dl=dl) == 0      # no record: a no-op
    wide = ints(*([1] * (9 * 120)))
    ids = ints(*range(130))
    assert matrix_batch(k=2, m=9, G=wide, dst=ints(*range(2, 11))) == EINVAL            # nine nonzeros in a column
    assert b"column 0 has 9 nonzero coefficients" in _err(ecg)
    assert matrix_batch(k=120, m=9, G=wide, src=ids, dst=ints(*range(120, 129))) == EINVAL
    assert b"k_in + m_out = 129 exceeds 128" in _err(ecg)
    sparse = ints(*([1] * 8 + [0] * 112 + [0] * 8 + [1] * 112))
    assert matrix_batch(k=120, m=2, G=sparse, src=ids, dst=ints(120, 121), R=0) == 0

    M = ints(*([1] * (9 * 120)))

    def encode_batch(k=2, m=1, matrix=M, base=dev, B=64, S=1, mode=0, r=rec, R=1, ml=64, i=inp, nb=64, d=None, v=rep):
        return L.ecg_update_encode_batch(k, m, matrix, base, 4096, 1024, B, S, mode, r, R, ml, i, nb, d, v, None)

    for kw, text in ((dict(k=0), b"k = 0"), (dict(m=0), b"m = 0"), (dict(matrix=None), b"matrix is NULL"),
                     (dict(base=None), b"base is NULL"), (dict(v=None), b"d_report is NULL"), (dict(B=-1), b"B = -1"),
                     (dict(S=-1), b"S = -1"), (dict(B=1 << 31), b"2^31"), (dict(k=2, m=9), b"9 nonzero"),
                     (dict(k=120, m=9), b"exceeds 128"), (dict(r=None), b"d_records"), (dict(i=None), b"d_in"),
                     (dict(mode=3), b"mode = 3"), (dict(mode=1, d=dl), b"ECG_UPDATE_DELTA"), (dict(ml=65), b"max_len")):
        assert encode_batch(**kw) == EINVAL, kw
        assert text in _err(ecg), (kw, _err(ecg))
    assert encode_batch(R=0) == 0 and encode_batch(k=120, m=8, R=0) == 0

    code = ecg.ec_factory(0, ecg.CodingParameters(k=6, m=4))
    tail = (4096, 256, 64, 1, 0, rec, 1, 64, inp, 64, None, rep, None)
    assert L.ecg_update_ec_batch(None, dev, *tail) == EINVAL and b"ec is NULL" in _err(ecg)
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_HOST, None)
    assert L.ecg_update_ec_batch(code._h, dev, *tail) == EINVAL and b"ECG_MEM_DEVICE" in _err(ecg)
    ptrs = (ctypes.c_void_p * 6)(*[0x10000 + 256 * i for i in range(6)])
    cptrs = (ctypes.c_void_p * 4)(*[0x20000 + 256 * i for i in range(4)])
    assert L.ecg_update_ec(code._h, ptrs, cptrs, 64, 0, 1, 0, 8, inp, None, rep) == EINVAL      # host handle
    assert b"ECG_MEM_DEVICE" in _err(ecg)
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, None)
    assert L.ecg_update_ec_batch(code._h, None, *tail) == EINVAL and b"base is NULL" in _err(ecg)
    assert L.ecg_update_ec_batch(code._h, dev, 4096, 256, 64, 1, 0, rec, 0, 64, inp, 64, None, rep, None) == 0
    holed = (ctypes.c_void_p * 6)(*[0x10000, 0x10100, None, 0x10300, 0x10400, 0x10500])
    for args, text in (((None, cptrs, 64, 0, 1, 0, 8, inp, None, rep), b"pointer array is NULL"),
                       ((ptrs, None, 64, 0, 1, 0, 8, inp, None, rep), b"pointer array is NULL"),
                       ((ptrs, cptrs, -1, 0, 1, 0, 8, inp, None, rep), b"block_size = -1"),
                       ((ptrs, cptrs, 64, 0, 1, 0, 8, None, None, rep), b"d_in is NULL"),
                       ((ptrs, cptrs, 64, 0, 1, 0, 8, inp, None, None), b"d_report is NULL"),
                       ((ptrs, cptrs, 64, 5, 1, 0, 8, inp, None, rep), b"mode = 5"),
                       ((ptrs, cptrs, 64, 1, 1, 0, 8, inp, dl, rep), b"ECG_UPDATE_DELTA"),
                       ((holed, cptrs, 64, 0, 1, 0, 8, inp, None, rep), b"a block pointer is NULL")):
        assert L.ecg_update_ec(code._h, *args) == EINVAL, args
        assert text in _err(ecg), (args, _err(ecg))
    assert L.ecg_update_ec(None, ptrs, cptrs, 64, 0, 1, 0, 8, inp, None, rep) == EINVAL


@pytest.mark.parametrize("name", [c["name"] for c in GOLDEN if "matrix" not in c])
def test_classes_without_an_encoding_matrix_are_refused(ecg, update, name):
    c = next(c for c in GOLDEN if c["name"] == name)
    code = ecg.ec_factory(c["type"], ecg.CodingParameters(**c["params"]))
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, None)
    dev, rec, inp, rep = (ctypes.c_void_p(0x10000 * i) for i in (1, 2, 3, 4))
    L = update.lib()
    assert L.ecg_update_ec_batch(code._h, dev, 1 << 20, 4096, 64, 1, 0, rec, 1, 64, inp, 64, None, rep,
                                 None) == ecg.ECG_EINVAL
    assert b"update: the class defines no encoding matrix" in _err(ecg)
    ptrs = (ctypes.c_void_p * code.k)(*[0x10000 + 256 * i for i in range(code.k)])
    cptrs = (ctypes.c_void_p * code.m)(*[0x20000 + 256 * i for i in range(code.m)])
    assert L.ecg_update_ec(code._h, ptrs, cptrs, 64, 0, 0, 0, 8, inp, None, rep) == ecg.ECG_EINVAL


# ---- the host helpers

def test_check_records_answers_the_plain_helper(ecg, update):
    k, B, S, ml, nb = 4, 64, 3, 16, 32
    ok = [[0, 0, 0, 5, 0], [0, 1, 5, 4, 5], [1, 0, 0, 5, 9], [0, 2, 20, 0, 0]]          # touching ranges are legal
    cases = [(ok, False, b""), (ok, True, b"")]
    for state, rec in ((1, [-1, 0, 30, 2, 20]), (1, [S, 0, 30, 2, 20]), (2, [2, k, 30, 2, 20]), (2, [2, -1, 30, 2, 20]),
                       (3, [2, 0, -1, 2, 20]), (3, [2, 0, 30, -2, 20]), (3, [2, 0, B - 1, 2, 20]),
                       (4, [2, 0, 30, ml + 1, 0]), (5, [2, 0, 30, 2, -1]), (5, [2, 0, 30, 2, nb - 1])):
        cases.append((ok + [rec] + ok, False, f"state {state}".encode()))
    cases += [(ok + [[0, 3, 8, 2, 20]], False, b"overlaps an earlier record's range in stripe 0"),
              (ok + [[0, 3, 3, 1, 20]], False, b"range in stripe 0"),
              (ok + [[1, 3, 5, 9, 20]], False, b""),                                     # [5,14) touches [0,5)
              (ok + [[2, 3, 8, 2, 13]], False, b""),
              (ok + [[2, 3, 8, 2, 13]], True, b"staging range"),
              ([[0, 0, 4, 4, 0], [0, 0, 0, 16, 8]], False, b"record 1 overlaps"),
              ([[0, 0, 0, 16, 8], [1, 0, 0, 1, 0], [0, 0, 4, 4, 0]], False, b"record 2 overlaps")]
    rng = np.random.default_rng(3)
    for _ in range(40):                                                                  # random sets, mostly conflicting
        n = int(rng.integers(1, 9))
        recs = np.stack([rng.integers(0, 2, n), rng.integers(0, k, n), rng.integers(0, 40, n), rng.integers(0, 12, n),
                         rng.integers(0, 20, n)], axis=1)
        cases += [(recs.tolist(), False, b""), (recs.tolist(), True, b"")]
    for recs, with_delta, text in cases:
        want = UP.check_records(recs, k, B, S, ml, nb, with_delta)
        assert update.check_records(recs, k, B, S, ml, nb, with_delta) == want, recs
        if want >= 0 and text:
            assert _err(ecg).startswith(b"update: record %d " % want) and text in _err(ecg), (recs, _err(ecg))
    assert update.check_records(np.zeros((0, 5), np.int64), k, B, S, ml, nb) == -1
    assert update.lib().ecg_update_check_records(None, 3, k, B, S, ml, nb, 0) == ecg.ECG_EINVAL
    assert update.lib().ecg_update_check_records(None, -1, k, B, S, ml, nb, 0) == ecg.ECG_EINVAL


def test_traffic_bytes_equals_the_plain_account(ecg, update):
    c = next(c for c in GOLDEN if c["name"] == "Azure(8,2,2)")
    nnz = update.nnz_per_col(c["matrix"], c["k"])
    assert nnz.tolist() == np.count_nonzero(np.asarray(c["matrix"]).reshape(c["m"], c["k"]), axis=0).tolist()
    rng = np.random.default_rng(9)
    recs = np.stack([rng.integers(0, 4, 50), rng.integers(0, c["k"], 50), rng.integers(0, 1000, 50),
                     rng.integers(0, 5000, 50), rng.integers(0, 1 << 40, 50)], axis=1)
    for mode in (UP.WRITE, UP.DELTA):
        for with_delta in (False, True):
            assert update.traffic_bytes(nnz, recs, mode, with_delta) == UP.traffic_bytes(nnz, recs, mode, with_delta)
    assert update.traffic_bytes(nnz, recs[:1], UP.WRITE) == int(recs[0, 3]) * (3 + 2 * int(nnz[recs[0, 1]]))
    assert update.traffic_bytes(nnz, np.zeros((0, 5), np.int64)) == 0
    with pytest.raises(ecg.EcgError):
        update.traffic_bytes(nnz, recs, 2)
    with pytest.raises(ecg.EcgError):
        update.traffic_bytes(nnz, [[0, c["k"], 0, 4, 0]])
