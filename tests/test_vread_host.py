"""The verified range read, the parts that need no GPU: libecg_vread.so's exports, every argument refusal with its error
text (each returns before any device is touched) and the host helpers against tests/vread_plain.py and ecg_dread.  Every
test here loads libecg_vread.so.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import dread_plain as DP
import vread_plain as VP

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def vread(ecg):
    import ecg_vread
    ecg_vread.lib()
    return ecg_vread


def _err(ecg):
    return ecg.lib().ecg_last_error()


# ---- the library

def test_header_symbols_exported(vread):
    hdr = open(os.path.join(ROOT, "include", "ecg_vread.h")).read()
    declared = sorted(set(re.findall(r"\b(ecg_vread_\w+)\s*\(", hdr)))
    assert len(declared) == 10
    assert sorted(vread.EXPORTS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", vread.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r" T (ecg_\w+)", out))) == declared
    assert sorted(vread._SIG) == declared
    need = subprocess.run(["readelf", "-d", vread.LIB_PATH], capture_output=True, text=True).stdout
    assert re.findall(r"NEEDED.*\[(libecg[^\]]*)\]", need) == ["libecg.so"]


def test_last_launch_reports_six_fields(vread):
    L = vread.lib()
    assert L.ecg_vread_last_launch(None, 0) == 6
    small = (ctypes.c_int * 5)(*([77] * 5))
    assert L.ecg_vread_last_launch(small, 5) == 6 and list(small) == [77] * 5
    full = (ctypes.c_int * 8)(*([77] * 8))
    assert L.ecg_vread_last_launch(full, 8) == 6 and list(full)[6:] == [77, 77]
    got = vread.last_launch()
    assert list(got) == list(vread.LAST_LAUNCH_FIELDS) and list(got.values()) == list(full)[:6]
    hdr = open(os.path.join(ROOT, "include", "ecg_vread.h")).read()
    assert re.findall(r"v\[(\d)\] (\w+)", hdr) == [(str(i), name) for i, name in enumerate(got)]
    assert L.ecg_vread_counters(None, None) == 0 and set(vread.counters()) == {"launches", "records"}
    assert re.findall(r"^ \*\s+(\d)  \w", hdr, re.M) == [str(i) for i in range(8)]       # the header's eight states
    assert vread.MISMATCH == VP.MISMATCH == 7 and vread.NO_PIECE == VP.NO_PIECE


# ---- arguments (no GPU is touched: every call returns before the first HIP call)

def test_bad_arguments(ecg, vread):
    L, EINVAL = vread.lib(), ecg.ECG_EINVAL
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    H = ints(1, 1, 1, 0, 1, 2, 0, 1)                                                      # 2 x 4
    ids = ints(0, 1, 2, 3)
    dev, lost, exp, rec, out, wk, sm, rep = (ctypes.c_void_p(0x10000 * i) for i in range(1, 9))  # never read
    ok = dict(n=4, r=2, H=H, ids=ids, base=dev, ss=1 << 20, bs=1 << 18, B=4096, S=1, lost=lost, P=512, exp=exp, rec=rec,
              R=1, ml=64, out=out, nb=64, wk=wk, sm=sm, rep=rep)

    def matrix_batch(**kw):
        a = dict(ok, **kw)
        return L.ecg_vread_matrix_batch(a["n"], a["r"], a["H"], a["ids"], a["base"], a["ss"], a["bs"], a["B"], a["S"],
                                        a["lost"], a["P"], a["exp"], a["rec"], a["R"], a["ml"], a["out"], a["nb"],
                                        a["wk"], a["sm"], a["rep"], None)

    wide = ints(*([1] * (9 * 129)))
    wide_ids = ints(*range(129))
    for kw, text in ((dict(n=0), b"n = 0"), (dict(r=0), b"r = 0"), (dict(r=-1), b"r = -1"),
                     (dict(r=9, n=12, H=wide, ids=wide_ids), b"r = 9"),
                     (dict(r=2, n=129, H=wide, ids=wide_ids), b"n = 129"),
                     (dict(H=None), b"H is NULL"), (dict(ids=None), b"src_ids is NULL"),
                     (dict(base=None), b"base is NULL"), (dict(rec=None), b"d_records is NULL"),
                     (dict(out=None), b"d_out is NULL"), (dict(wk=None), b"d_work is NULL"),
                     (dict(rep=None), b"d_report is NULL"), (dict(sm=None), b"d_sums is NULL"),
                     (dict(exp=None), b"d_expected is NULL"),
                     (dict(B=-1), b"B = -1"), (dict(S=-1), b"S = -1"), (dict(R=-1), b"R = -1"),
                     (dict(ml=-1), b"max_len = -1"), (dict(nb=-1), b"out_bytes = -1"),
                     (dict(B=1 << 31, ml=0), b"not below 2^31"), (dict(ml=4097), b"max_len = 4097 exceeds B = 4096"),
                     (dict(rec=ctypes.c_void_p(0x30004)), b"8-byte aligned"),
                     (dict(wk=ctypes.c_void_p(0x50010)), b"32-byte aligned"),
                     (dict(sm=ctypes.c_void_p(0x70002)), b"4-byte aligned"),
                     (dict(ids=ints(0, -1, 2, 3)), b"negative id"),
                     (dict(ids=ints(0, 1, 1, 3)), b"src_ids names block 1 twice"),
                     (dict(P=256), b"piece_bytes = 256"), (dict(P=768), b"piece_bytes = 768"),
                     (dict(P=-512), b"piece_bytes = -512"), (dict(P=1 << 31), b"piece_bytes = 2147483648"),
                     (dict(P=513), b"piece_bytes = 513"),
                     (dict(R=1 << 20, B=1 << 21, ml=1 << 21), b"R * NP is not below 2^31"),     # NP = 4096
                     (dict(R=(1 << 31) - 1, B=1 << 30, ml=1 << 30, P=0), b"2^31 - 1 workgroups")):
        assert matrix_batch(**kw) == EINVAL, kw
        assert _err(ecg).startswith(b"vread: ") and text in _err(ecg), (kw, _err(ecg))
    assert matrix_batch(R=0) == 0 and matrix_batch(R=0, wk=None) == 0                    # no record: a no-op
    assert matrix_batch(R=0, lost=None) == 0                                             # d_lost may be NULL
    assert matrix_batch(r=8, n=128, H=wide, ids=wide_ids, R=0) == 0                      # the largest shape is accepted
    for P in (0, 512, 1 << 30):
        assert matrix_batch(R=0, P=P) == 0

    M = ints(*([1] * (9 * 127)))

    def encode_batch(k=2, m=1, matrix=M, base=dev, B=4096, S=1, f=lost, P=512, e=exp, r=rec, R=1, ml=64, o=out, nb=64,
                     w=wk, s=sm, v=rep):
        return L.ecg_vread_encode_batch(k, m, matrix, base, 1 << 20, 1 << 18, B, S, f, P, e, r, R, ml, o, nb, w, s, v,
                                        None)

    for kw, text in ((dict(k=0), b"k = 0"), (dict(m=0), b"m = 0"), (dict(matrix=None), b"matrix is NULL"),
                     (dict(base=None), b"base is NULL"), (dict(v=None), b"d_report is NULL"), (dict(B=-1), b"B = -1"),
                     (dict(m=9), b"r = 9"), (dict(k=127, m=2), b"n = 129"), (dict(P=100), b"piece_bytes = 100"),
                     (dict(e=None), b"d_expected"), (dict(s=None), b"d_sums"), (dict(r=None), b"d_records"),
                     (dict(o=None), b"d_out"), (dict(w=None), b"d_work"), (dict(ml=4097), b"max_len")):
        assert encode_batch(**kw) == EINVAL, kw
        assert text in _err(ecg), (kw, _err(ecg))
    assert encode_batch(R=0) == 0 and encode_batch(k=120, m=8, R=0) == 0 and encode_batch(R=0, f=None) == 0

    code = ecg.ec_factory(0, ecg.CodingParameters(k=6, m=4))
    tail = (1 << 20, 1 << 16, 4096, 1, lost, 512, exp, rec, 1, 64, out, 64, wk, sm, rep, None)
    assert L.ecg_vread_ec_batch(None, dev, *tail) == EINVAL and b"ec is NULL" in _err(ecg)
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_HOST, None)
    assert L.ecg_vread_ec_batch(code._h, dev, *tail) == EINVAL and b"ECG_MEM_DEVICE" in _err(ecg)
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, None)
    assert L.ecg_vread_ec_batch(code._h, None, *tail) == EINVAL and b"base is NULL" in _err(ecg)
    assert L.ecg_vread_ec_batch(code._h, dev, *(tail[:8] + (0,) + tail[9:])) == 0         # R == 0

    for bad in (-2048, 1, 2047, 3000):
        assert L.ecg_vread_set_span_bytes(bad) == EINVAL and b"span_bytes = %d" % bad in _err(ecg)
    assert L.ecg_vread_set_span_bytes(4096) == 0 and L.ecg_vread_set_span_bytes(0) == 0


# ---- the host helpers

def test_cover_max_pieces_and_work_bytes_equal_the_plain_versions(ecg, vread):
    import ecg_dread
    rng = np.random.default_rng(17)
    for B in (1, 15, 511, 512, 513, 4096, 4097, 4661, 8192, 100000):
        for P in (0, 512, 1024, 2048, 4096, 8192, 1 << 20):
            fixed = [(0, 0), (B, 0), (0, B), (B - 1, 1), (0, 1), (max(0, B - 2), min(2, B))]
            if P and B > P:
                last = (B - 1) // P * P                                          # where the last piece starts
                fixed += [(P - 1, 2), (P - 1, 1), (P, 1), (last - 1, B - last + 1), (last, B - last), (0, P), (1, P)]
            rand = [(int(o), int(rng.integers(0, B - o + 1))) for o in rng.integers(0, B + 1, 12)]
            for off, ln in fixed + rand:
                assert vread.cover(off, ln, P, B) == VP.cover(off, ln, P, B), (off, ln, P, B)
            for ml in sorted({0, 1, min(B, 2), min(B, 511), min(B, 513), min(B, P or 1), min(B, (P or 1) + 1),
                              min(B, (P or 1) + 2), B}):
                assert vread.max_pieces(ml, P, B) == VP.max_pieces(ml, P, B), (ml, P, B)
    assert vread.cover(512, 1, 512, 513) == (1, 1, 1)                            # a last piece of one byte
    assert vread.cover(0, 4661, 8192, 4661) == (0, 1, 4661)                      # P >= B
    assert vread.cover(4660, 1, 0, 4661) == (0, 1, 4661)                         # block sums
    L = vread.lib()
    for args, text in (((0, 1, 100, 64), b"piece_bytes = 100"), ((-1, 1, 512, 64), b"off = -1"),
                       ((0, -1, 512, 64), b"len = -1"), ((60, 5, 512, 64), b"len = 5"), ((0, 0, 512, -1), b"B = -1")):
        assert L.ecg_vread_cover(*args, None, None, None) == ecg.ECG_EINVAL and text in _err(ecg), args
    assert L.ecg_vread_cover(0, 64, 512, 64, None, None, None) == 0
    for args, text in (((1, 100, 64), b"piece_bytes = 100"), ((65, 512, 64), b"max_len = 65"), ((-1, 512, 64), b"max_len")):
        assert L.ecg_vread_max_pieces(*args) == ecg.ECG_EINVAL and text in _err(ecg), args
    for n in (1, 7, 8, 14, 128):
        for R in (0, 1, 5):
            assert vread.work_bytes(R, n) == ecg_dread.work_bytes(R, n)
    for R, n in ((-1, 4), (1, 0), (1, 129)):
        assert L.ecg_vread_work_bytes(R, n) == ecg.ECG_EINVAL and _err(ecg).startswith(b"vread: ")


def test_check_records_agrees_with_dread(ecg, vread):
    import ecg_dread
    n, B, S, ml, nb = 6, 64, 3, 16, 40
    ok = [[0, 0, 0, 5, 0], [0, 1, 5, 4, 5], [1, 0, 0, 5, 9], [0, 2, 20, 0, 0]]
    cases = [ok, ok + [[0, 3, 8, 2, 13]], ok + [[2, 3, 8, 2, 14]], [[0, 0, 4, 4, 10], [1, 0, 0, 16, 0]]]
    for rec in ([-1, 0, 30, 2, 20], [S, 0, 30, 2, 20], [2, n, 30, 2, 20], [2, 0, -1, 2, 20], [2, 0, B - 1, 2, 20],
                [2, 0, 30, ml + 1, 0], [2, 0, 30, 2, -1], [2, 0, 30, 2, nb - 1]):
        cases.append(ok + [rec] + ok)
    rng = np.random.default_rng(3)
    for _ in range(40):
        k = int(rng.integers(1, 9))
        cases.append(np.stack([rng.integers(0, S, k), rng.integers(0, n, k), rng.integers(0, 50, k),
                               rng.integers(0, 12, k), rng.integers(0, 36, k)], axis=1).tolist())
    hits = 0
    for recs in cases:
        want = DP.check_records(recs, n, B, S, ml, nb)
        assert vread.check_records(recs, n, B, S, ml, nb) == want == ecg_dread.check_records(recs, n, B, S, ml, nb)
        if want >= 0:
            assert vread.check_records(recs, n, B, S, ml, nb) == want           # sets this library's error text
            assert _err(ecg).startswith(b"vread: record %d " % want), _err(ecg)
            hits += 1
    assert 10 < hits < len(cases)
    assert vread.check_records(np.zeros((0, 5), np.int64), n, B, S, ml, nb) == -1
    assert vread.lib().ecg_vread_check_records(None, 3, n, B, S, ml, nb) == ecg.ECG_EINVAL
    assert vread.lib().ecg_vread_check_records(None, -1, n, B, S, ml, nb) == ecg.ECG_EINVAL


def test_mismatched_rows(vread):
    recs = [[0, 1, 510, 3, 0], [2, 6, 1090, 10, 3], [1, 2, 0, 2000, 13]]
    rep = [[7, 6, 1, 1], [0, 6, 0, VP.NO_PIECE], [7, 1, 2, 2]]
    assert vread.mismatched_rows(recs, np.array(rep), 512) == VP.mismatched_rows(recs, rep, 512) == [(0, 1), (1, 2), (1, 3)]
    assert vread.mismatched_rows(recs, np.array([[7, 6, 1, 0], [0, 6, 0, -1], [0, 1, 0, -1]]), 0) == [(0, 0)]
