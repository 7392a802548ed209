"""The update sums, the parts that need no GPU: libecg_usum.so's exports and code object, every argument refusal with
its error text (each returns before any device is touched), the host form ecg_usum_expected against
tests/usum_plain.py and against ecg_sum_combine, the traffic account and the fields of the last launch.  Every test
here loads libecg_usum.so.
"""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import test_kernel_resources as KR
import usum_plain as US

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
K_MAX_NNZ = 8                                              # update_kernels.hpp kUpdateMaxNnz
OTHERS = ("libecg.so", "libecg_scrub.so", "libecg_locate.so", "libecg_heal.so", "libecg_heal2.so", "libecg_sum.so",
          "libecg_psum.so", "libecg_restore.so", "libecg_update.so")


@pytest.fixture(scope="module")
def usum(ecg):
    import ecg_usum
    ecg_usum.lib()
    return ecg_usum


def _err(ecg):
    return ecg.lib().ecg_last_error()


# ---- the library

def test_header_symbols_exported(usum):
    hdr = open(os.path.join(ROOT, "include", "ecg_usum.h")).read()
    declared = sorted(set(re.findall(r"\b(ecg_usum_\w+)\s*\(", hdr)))
    assert len(declared) == 7
    assert sorted(usum.EXPORTS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", usum.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r" T (ecg_\w+)", out))) == declared
    assert sorted(usum._SIG) == declared


def test_needs_libecg_only_and_nothing_needs_it(usum):
    lib_dir = os.path.dirname(KR.LIB)
    need = subprocess.run(["readelf", "-d", usum.LIB_PATH], capture_output=True, text=True).stdout
    needed = re.findall(r"NEEDED.*\[(libecg[^\]]*)\]", need)
    assert needed == ["libecg.so"], needed
    for so in OTHERS:
        need = subprocess.run(["readelf", "-d", os.path.join(lib_dir, so)], capture_output=True, text=True).stdout
        assert "NEEDED" in need and "libecg_usum" not in need, so
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(lib_dir, so)], capture_output=True,
                             text=True).stdout
        assert not re.findall(r" T (ecg_usum\w*)", out), so


def test_last_launch_reports_five_fields(usum):
    L = usum.lib()
    assert L.ecg_usum_last_launch(None, 0) == 5
    small = (ctypes.c_int * 4)(*([77] * 4))
    assert L.ecg_usum_last_launch(small, 4) == 5 and list(small) == [77] * 4
    full = (ctypes.c_int * 7)(*([77] * 7))
    assert L.ecg_usum_last_launch(full, 7) == 5 and list(full)[5:] == [77, 77]
    got = usum.last_launch()
    assert tuple(got) == usum.LAST_LAUNCH_FIELDS == ("cols_per_wg", "wg_per_record", "R", "max_nnz", "piece_bytes")
    assert list(got.values()) == list(full)[:5] and all(v >= 0 for v in got.values())
    hdr = open(os.path.join(ROOT, "include", "ecg_usum.h")).read()
    assert re.findall(r"v\[(\d)\] (\w+)", hdr) == [(str(i), name) for i, name in enumerate(got)]
    n = [ctypes.c_longlong(-1), ctypes.c_longlong(-1)]
    assert L.ecg_usum_counters(ctypes.byref(n[0]), ctypes.byref(n[1])) == 0 and n[0].value >= 0 and n[1].value >= 0
    assert L.ecg_usum_counters(None, None) == 0
    assert usum.counters() == {"launches": n[0].value, "records": n[1].value}


@pytest.fixture(scope="module")
def meta(usum):
    """Kernel metadata of libecg_usum.so's gfx950 code object, read as tests/test_kernel_resources.py reads
    libecg.so's."""
    saved = KR.LIB
    KR.LIB = usum.LIB_PATH
    try:
        return KR._metadata()
    finally:
        KR.LIB = saved


def test_code_object_is_the_usum_family(meta):
    keys = []
    for s in meta:
        v = re.search(r"crc_usum_kernelILi(\d+)EE", s)
        assert v, s
        keys.append(int(v.group(1)))
    assert sorted(keys) == list(range(1, K_MAX_NNZ + 1))


def test_usum_kernels_use_no_scratch(meta):
    bad = {n: f for n, f in meta.items() if f.get("private_segment_fixed_size", 0) or f.get("vgpr_spill_count", 0)
           or f.get("sgpr_spill_count", 0)}
    assert not bad, list(bad)[:5]
    # the x^32 step tables (4 KiB) and a few words for the fold: many workgroups per CU
    assert all(4096 <= f.get("group_segment_fixed_size", 0) <= 4096 + 256 for f in meta.values())
    assert all(f["kernarg_segment_size"] <= 4096 for f in meta.values())
    assert max(f["vgpr_count"] for f in meta.values()) <= 128


# ---- arguments (no GPU is touched: every call returns before the first HIP call)

def test_bad_arguments(ecg, usum):
    L, EINVAL = usum.lib(), ecg.ECG_EINVAL
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    G, src, dst, ids = ints(1, 1, 1, 2), ints(0, 1), ints(2, 3), ints(0, 1, 2, 3)
    rec, dl, sums, up, rep = (ctypes.c_void_p(0x10000 * i) for i in (1, 2, 3, 4, 5))   # never read
    ok = dict(k=2, m=2, G=G, src=src, dst=dst, B=4096, S=1, rec=rec, R=1, ml=64, dl=dl, nb=64, ids=ids, n=4, P=0,
              which=3, sums=sums, up=None, rep=rep)

    def matrix_batch(**kw):
        a = dict(ok, **kw)
        return L.ecg_usum_matrix_batch(a["k"], a["m"], a["G"], a["src"], a["dst"], a["B"], a["S"], a["rec"], a["R"],
                                       a["ml"], a["dl"], a["nb"], a["ids"], a["n"], a["P"], a["which"], a["sums"],
                                       a["up"], a["rep"], None)

    for kw, text in ((dict(k=0), b"k_in = 0"), (dict(m=0), b"m_out = 0"), (dict(k=-3), b"k_in = -3"),
                     (dict(G=None), b"coef is NULL"), (dict(src=None), b"src_ids is NULL"),
                     (dict(dst=None), b"dst_ids is NULL"), (dict(ids=None), b"sum_ids is NULL"),
                     (dict(rec=None), b"d_records is NULL"), (dict(dl=None), b"d_delta is NULL"),
                     (dict(sums=None), b"d_sums is NULL"), (dict(rep=None), b"d_report is NULL"),
                     (dict(B=-1), b"B = -1"), (dict(S=-1), b"S = -1"), (dict(R=-1), b"R = -1"),
                     (dict(ml=-1), b"max_len = -1"), (dict(nb=-1), b"in_bytes = -1"),
                     (dict(B=1 << 31, ml=0), b"not below 2^31"), (dict(ml=4097), b"max_len = 4097 exceeds B = 4096"),
                     (dict(P=256), b"piece_bytes = 256"), (dict(P=768), b"piece_bytes = 768"),
                     (dict(P=1 << 31), b"power of two in [512, 2^30]"), (dict(P=-512), b"piece_bytes = -512"),
                     (dict(which=0), b"which = 0"), (dict(which=4), b"which = 4"), (dict(which=-1), b"which = -1"),
                     (dict(n=0), b"n_sums = 0"), (dict(n=129), b"n_sums = 129"),
                     (dict(ids=ints(0, 1, 2, 2)), b"sum_ids names block 2 twice"),
                     (dict(ids=ints(0, 1, -2, 3)), b"sum_ids holds a negative id"),
                     (dict(S=1 << 30, P=512, B=1 << 20), b"sum words is 2^31 or more"),
                     (dict(rec=ctypes.c_void_p(0x20004)), b"8-byte aligned"),
                     (dict(sums=ctypes.c_void_p(0x30002)), b"4-byte aligned"),
                     (dict(src=ints(0, -1)), b"negative id"), (dict(dst=ints(-2, 3)), b"negative id"),
                     (dict(src=ints(1, 1)), b"src_ids names block 1 twice"),
                     (dict(dst=ints(3, 3)), b"dst_ids names block 3 twice"),
                     (dict(dst=ints(2, 0)), b"block 0 is both"),
                     (dict(R=(1 << 31) - 1, B=1 << 20, ml=1 << 20), b"2^31 - 1 workgroups")):
        assert matrix_batch(**kw) == EINVAL, kw
        assert _err(ecg).startswith(b"usum: ") and text in _err(ecg), (kw, _err(ecg))
    assert matrix_batch(R=0) == 0 and matrix_batch(R=0, up=up) == 0      # no record: a no-op
    for P in (0, 512, 1 << 30):
        assert matrix_batch(R=0, P=P) == 0
    wide = ints(*([1] * (9 * 120)))
    many = ints(*range(130))
    assert matrix_batch(k=2, m=9, G=wide, dst=ints(*range(2, 11))) == EINVAL            # nine nonzeros in a column
    assert b"column 0 has 9 nonzero coefficients" in _err(ecg)
    assert matrix_batch(k=120, m=9, G=wide, src=many, dst=ints(*range(120, 129))) == EINVAL
    assert b"k_in + m_out = 129 exceeds 128" in _err(ecg)

    def encode_batch(k=2, m=1, matrix=wide, B=4096, S=1, r=rec, R=1, ml=64, d=dl, nb=64, P=0, which=3, s=sums, v=rep):
        return L.ecg_usum_encode_batch(k, m, matrix, B, S, r, R, ml, d, nb, P, which, s, None, v, None)

    for kw, text in ((dict(k=0), b"k = 0"), (dict(m=0), b"m = 0"), (dict(matrix=None), b"matrix is NULL"),
                     (dict(s=None), b"d_sums is NULL"), (dict(v=None), b"d_report is NULL"), (dict(B=-1), b"B = -1"),
                     (dict(B=1 << 31), b"2^31"), (dict(k=2, m=9), b"9 nonzero"), (dict(k=120, m=9), b"exceeds 128"),
                     (dict(r=None), b"d_records"), (dict(d=None), b"d_delta"), (dict(P=100), b"piece_bytes = 100"),
                     (dict(which=8), b"which = 8"), (dict(ml=4097), b"max_len")):
        assert encode_batch(**kw) == EINVAL, kw
        assert text in _err(ecg), (kw, _err(ecg))
    assert encode_batch(R=0) == 0 and encode_batch(k=120, m=8, R=0) == 0

    code = ecg.ec_factory(0, ecg.CodingParameters(k=6, m=4))
    tail = (4096, 1, rec, 1, 64, dl, 64, 0, 3, sums, None, rep, None)
    assert L.ecg_usum_ec_batch(None, *tail) == EINVAL and b"ec is NULL" in _err(ecg)
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_HOST, None)
    assert L.ecg_usum_ec_batch(code._h, *tail) == EINVAL and b"ECG_MEM_DEVICE" in _err(ecg)
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, None)
    assert L.ecg_usum_ec_batch(code._h, 4096, 1, rec, 0, 64, dl, 64, 0, 3, sums, None, rep, None) == 0
    assert L.ecg_usum_ec_batch(code._h, 4096, 1, rec, 1, 64, dl, 64, 0, 3, None, None, rep, None) == EINVAL
    assert b"d_sums is NULL" in _err(ecg)


@pytest.mark.parametrize("name", [c["name"] for c in GOLDEN if "matrix" not in c])
def test_classes_without_an_encoding_matrix_are_refused(ecg, usum, name):
    c = next(c for c in GOLDEN if c["name"] == name)
    code = ecg.ec_factory(c["type"], ecg.CodingParameters(**c["params"]))
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, None)
    rec, dl, sums, rep = (ctypes.c_void_p(0x10000 * i) for i in (1, 2, 3, 4))
    assert usum.lib().ecg_usum_ec_batch(code._h, 4096, 1, rec, 1, 64, dl, 64, 0, 3, sums, None, rep,
                                        None) == ecg.ECG_EINVAL
    assert b"usum: the class defines no encoding matrix" in _err(ecg)


# ---- the host form

def _azure():
    c = next(c for c in GOLDEN if c["name"] == "Azure(8,2,2)")
    return c["k"], c["m"], [int(v) for v in c["matrix"]]


def _records(rng, S, k, B, nb, count, longest):
    off = rng.integers(0, B, count)
    ln = np.minimum(rng.integers(0, longest + 1, count), B - off)
    return np.stack([rng.integers(0, S, count), rng.integers(0, k, count), off, ln, rng.integers(0, nb - longest, count)],
                    axis=1).astype(np.int64)


@pytest.mark.parametrize("piece_bytes", [0, 512, 4096])
@pytest.mark.parametrize("which", [1, 2, 3])
def test_expected_answers_the_plain_form(usum, piece_bytes, which):
    k, m, M = _azure()
    S, B, nb = 3, 8 * 1024 + 80, 3000
    rng = np.random.default_rng(piece_bytes + which)
    delta = rng.integers(0, 256, nb, dtype=np.uint8)
    delta[rng.integers(0, nb, 400)] = 0
    recs = _records(rng, S, k, B, nb, 24, 700)                                # overlapping: they simply add
    recs = np.concatenate([recs, [[0, 0, B - 100, 100, 5], [1, k - 1, 0, 0, 0], [S, 0, 0, 4, 0], [0, k, 0, 4, 0],
                                  [0, 0, B, 1, 0], [0, 0, 0, 701, 0], [0, 0, 0, 9, nb - 8], [2, 3, 8100, 172, 40]]])
    up = np.zeros((len(recs), 2), np.int64)
    up[[1, 5], 0] = [4, 2]
    ids = [11, 0, 3, 8, 9, 5, 7]                                              # scrambled, some blocks missing
    src, dst = list(range(k)), list(range(k, k + m))
    table = rng.integers(0, 1 << 32, (S, len(ids), US.pieces(B, piece_bytes)), dtype=np.uint32)
    for report in (None, up):
        want = table.copy()
        want_rep = US.usum(M, src, dst, ids, want, recs, delta, B, 700, piece_bytes, which, report)
        got, rep = usum.expected(M, src, dst, ids, table, recs, delta, B, piece_bytes, which, 700, report)
        assert np.array_equal(rep.astype(np.int64), want_rep)
        assert np.array_equal(got, want) and not np.array_equal(got, table)
    assert want_rep[-8:, 0].tolist() == [0, 0, 1, 2, 3, 4, 5, 0]


@pytest.mark.parametrize("piece_bytes", [0, 1 << 30])
def test_expected_in_a_block_of_2_31_less_1(usum, piece_bytes):
    """Only the tail shift is long: no block is allocated."""
    k, m, M = _azure()
    B = (1 << 31) - 1
    rng = np.random.default_rng(2)
    delta = rng.integers(1, 256, 64, dtype=np.uint8)
    recs = [[0, 2, 5, 33, 7], [0, 7, B - 40, 40, 20], [0, 0, (1 << 30) - 9, 20, 0]]   # the last crosses a piece border
    ids = list(range(k + m))
    src, dst = ids[:k], ids[k:]
    table = rng.integers(0, 1 << 32, (1, k + m, US.pieces(B, piece_bytes)), dtype=np.uint32)
    want = table.copy()
    want_rep = US.usum(M, src, dst, ids, want, recs, delta, B, 64, piece_bytes)
    got, rep = usum.expected(M, src, dst, ids, table, recs, delta, B, piece_bytes, max_len=64)
    assert np.array_equal(got, want) and np.array_equal(rep.astype(np.int64), want_rep)
    assert rep.tolist() == [[0, 33], [0, 40], [0, 20]]


def test_expected_agrees_with_sum_combine(ecg, usum):
    """A block A || X || C whose X becomes X': by ecg_sum_crc32c and ecg_sum_combine, and by the update sum."""
    import ecg_sum
    L = ecg_sum.lib()
    crc = lambda a: L.ecg_sum_crc32c(a.ctypes.data, a.size) & 0xFFFFFFFF
    rng = np.random.default_rng(4)
    B, off, ln = 5000, 1234, 777
    block = rng.integers(0, 256, B, dtype=np.uint8)
    new = block.copy()
    new[off:off + ln] = rng.integers(0, 256, ln, dtype=np.uint8)
    delta = np.ascontiguousarray(block[off:off + ln] ^ new[off:off + ln])
    a, x, c = new[:off].copy(), new[off:off + ln].copy(), new[off + ln:].copy()
    combined = L.ecg_sum_combine(L.ecg_sum_combine(crc(a), crc(x), ln), crc(c), c.size) & 0xFFFFFFFF
    assert combined == crc(new)
    table = np.array([[[crc(block)]]], dtype=np.uint32)
    got, rep = usum.expected([[1]], [0], [1], [0], table, [[0, 0, off, ln, 0]], delta, B)
    assert int(got[0, 0, 0]) == combined and rep.tolist() == [[0, np.count_nonzero(delta)]]


def test_expected_refuses_what_the_device_form_refuses(ecg, usum):
    table = np.zeros((1, 2, 1), np.uint32)
    with pytest.raises(ecg.EcgError):
        usum.expected([[1]], [0], [1], [0, 1], table, [[0, 0, 0, 4, 0]], np.zeros(8, np.uint8), 64, which=0)
    assert b"usum: which = 0" in _err(ecg)
    with pytest.raises(ecg.EcgError):
        usum.expected([[1]], [0], [1], [0, 0], table, [[0, 0, 0, 4, 0]], np.zeros(8, np.uint8), 64)
    assert b"sum_ids names block 0 twice" in _err(ecg)
    L = usum.lib()
    assert L.ecg_usum_expected(1, 1, (ctypes.c_int * 1)(1), (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(1), 64, 1, None,
                               1, 64, None, 8, (ctypes.c_int * 1)(0), 1, 0, 3, None, None, None) == ecg.ECG_EINVAL
    assert b"h_records is NULL" in _err(ecg)


def test_traffic_bytes_equals_the_plain_account(ecg, usum):
    k, m, M = _azure()
    nnz = np.count_nonzero(np.asarray(M).reshape(m, k), axis=0).astype(np.uint8)
    rng = np.random.default_rng(9)
    B = 1 << 20
    recs = _records(rng, 4, k, B, 1 << 30, 50, 70000)
    for P in (0, 512, 4096, 1 << 30):
        for which in (1, 2, 3):
            assert usum.traffic_bytes(nnz, recs, B, P, which) == US.traffic_bytes(nnz, recs, B, P, which)
    one = [[0, 2, 4000, 4096, 0]]                                             # 4 KiB across two 4 KiB pieces
    assert usum.traffic_bytes(nnz, one, B, 4096, 3) == 4096 + 8 * 2 * (1 + int(nnz[2]))
    assert usum.traffic_bytes(nnz, one, B, 0, 1) == 4096 + 8
    assert usum.traffic_bytes(nnz, np.zeros((0, 5), np.int64), B) == 0
    with pytest.raises(ecg.EcgError):
        usum.traffic_bytes(nnz, recs, B, 0, 4)
    with pytest.raises(ecg.EcgError):
        usum.traffic_bytes(nnz, [[0, k, 0, 4, 0]], B)
