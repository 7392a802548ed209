"""The degraded range read, the parts that need no GPU: libecg_dread.so's exports and code object, every argument
refusal with its error text (each returns before any device is touched), the two host helpers against
tests/dread_plain.py and the fields of the last launch.  Every test here loads libecg_dread.so.
"""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import dread_plain as DP
import test_dread_plain as TDP
import test_kernel_resources as KR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
K_MAX_R = 8                                                # gf_kernels.hpp kMaxMT
OTHERS = ("libecg.so", "libecg_scrub.so", "libecg_locate.so", "libecg_heal.so", "libecg_heal2.so", "libecg_sum.so",
          "libecg_psum.so", "libecg_restore.so", "libecg_update.so", "libecg_usum.so")


@pytest.fixture(scope="module")
def dread(ecg):
    import ecg_dread
    ecg_dread.lib()
    return ecg_dread


def _err(ecg):
    return ecg.lib().ecg_last_error()


# ---- the library

def test_header_symbols_exported(dread):
    hdr = open(os.path.join(ROOT, "include", "ecg_dread.h")).read()
    declared = sorted(set(re.findall(r"\b(ecg_dread_\w+)\s*\(", hdr)))
    assert len(declared) == 8
    assert sorted(dread.EXPORTS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", dread.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r" T (ecg_\w+)", out))) == declared
    assert sorted(dread._SIG) == declared


def test_needs_libecg_only_and_nothing_needs_it(dread):
    lib_dir = os.path.dirname(KR.LIB)
    need = subprocess.run(["readelf", "-d", dread.LIB_PATH], capture_output=True, text=True).stdout
    needed = re.findall(r"NEEDED.*\[(libecg[^\]]*)\]", need)
    assert needed == ["libecg.so"], needed
    for so in OTHERS:
        need = subprocess.run(["readelf", "-d", os.path.join(lib_dir, so)], capture_output=True, text=True).stdout
        assert "NEEDED" in need and "libecg_dread" not in need, so
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(lib_dir, so)], capture_output=True,
                             text=True).stdout
        assert not re.findall(r" T (ecg_dread\w*)", out), so


def test_last_launch_reports_four_fields(dread):
    L = dread.lib()
    assert L.ecg_dread_last_launch(None, 0) == 4
    small = (ctypes.c_int * 3)(*([77] * 3))
    assert L.ecg_dread_last_launch(small, 3) == 4 and list(small) == [77] * 3
    full = (ctypes.c_int * 6)(*([77] * 6))
    assert L.ecg_dread_last_launch(full, 6) == 4 and list(full)[4:] == [77, 77]
    got = dread.last_launch()
    assert list(got) == ["cols_per_wg", "wg_per_record", "R", "max_reads"] == list(dread.LAST_LAUNCH_FIELDS)
    assert list(got.values()) == list(full)[:4] and all(v >= 0 for v in got.values())
    hdr = open(os.path.join(ROOT, "include", "ecg_dread.h")).read()
    assert re.findall(r"v\[(\d)\] (\w+)", hdr) == [(str(i), name) for i, name in enumerate(got)]
    n = [ctypes.c_longlong(-1), ctypes.c_longlong(-1)]
    assert L.ecg_dread_counters(ctypes.byref(n[0]), ctypes.byref(n[1])) == 0 and n[0].value >= 0 and n[1].value >= 0
    assert L.ecg_dread_counters(None, None) == 0
    assert dread.counters() == {"launches": n[0].value, "records": n[1].value}
    assert [dread.ANSWERED, dread.BAD_STRIPE, dread.BAD_COL, dread.BAD_RANGE, dread.TOO_LONG, dread.BAD_OUT,
            dread.UNRECOVERABLE] == list(range(7))
    assert re.findall(r"^ \*\s+(\d)  \w", hdr, re.M) == [str(i) for i in range(7)]       # the header's seven states


def test_work_bytes(ecg, dread):
    for n in (1, 7, 8, 14, 128):
        per = dread.work_bytes(1, n)
        assert per % 32 == 0 and per >= 8 + 4 * n + 32 * n      # state, reads, n block ids, n coefficient tables
        assert dread.work_bytes(5, n) == 5 * per and dread.work_bytes(0, n) == 0
    for R, n in ((-1, 4), (1, 0), (1, 129)):
        assert dread.lib().ecg_dread_work_bytes(R, n) == ecg.ECG_EINVAL and _err(ecg).startswith(b"dread: ")


@pytest.fixture(scope="module")
def meta(dread):
    """Kernel metadata of libecg_dread.so's gfx950 code object, read as tests/test_kernel_resources.py reads
    libecg.so's."""
    saved = KR.LIB
    KR.LIB = dread.LIB_PATH
    try:
        return KR._metadata()
    finally:
        KR.LIB = saved


def test_code_object_is_the_dread_family(meta):
    names = sorted(re.search(r"gf_dread_\w*kernel(ILb[01]E)?", s).group(0) for s in meta)
    assert names == ["gf_dread_kernelILb0E", "gf_dread_kernelILb1E", "gf_dread_plan_kernel"], list(meta)


def test_dread_kernels_use_no_scratch_no_lds(meta):
    bad = {n: f for n, f in meta.items() if f.get("private_segment_fixed_size", 0) or f.get("vgpr_spill_count", 0)
           or f.get("sgpr_spill_count", 0)}
    assert not bad, list(bad)[:5]
    assert all(f.get("group_segment_fixed_size", 0) == 0 for f in meta.values())         # the plan kernel included
    assert all(f["kernarg_segment_size"] <= 4096 for f in meta.values())
    # one accumulator column and a batch of four loads: eight waves per SIMD for the main kernels
    assert max(f["vgpr_count"] for n, f in meta.items() if "plan" not in n) <= 64
    assert max(f["vgpr_count"] for f in meta.values()) <= 128


# ---- arguments (no GPU is touched: every call returns before the first HIP call)

def test_bad_arguments(ecg, dread):
    L, EINVAL = dread.lib(), ecg.ECG_EINVAL
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    H = ints(1, 1, 1, 0, 1, 2, 0, 1)                                                      # 2 x 4
    ids = ints(0, 1, 2, 3)
    dev, lost, rec, out, wk, rep = (ctypes.c_void_p(0x10000 * i) for i in (1, 2, 3, 4, 5, 6))   # never read
    ok = dict(n=4, r=2, H=H, ids=ids, base=dev, ss=4096, bs=1024, B=64, S=1, lost=lost, rec=rec, R=1, ml=64, out=out,
              nb=64, wk=wk, rep=rep)

    def matrix_batch(**kw):
        a = dict(ok, **kw)
        return L.ecg_dread_matrix_batch(a["n"], a["r"], a["H"], a["ids"], a["base"], a["ss"], a["bs"], a["B"], a["S"],
                                        a["lost"], a["rec"], a["R"], a["ml"], a["out"], a["nb"], a["wk"], a["rep"],
                                        None)

    wide = ints(*([1] * (9 * 129)))
    wide_ids = ints(*range(129))
    for kw, text in ((dict(n=0), b"n = 0"), (dict(r=0), b"r = 0"), (dict(r=-1), b"r = -1"),
                     (dict(r=9, n=12, H=wide, ids=wide_ids), b"r = 9"),
                     (dict(r=2, n=129, H=wide, ids=wide_ids), b"n = 129"),
                     (dict(H=None), b"H is NULL"), (dict(ids=None), b"src_ids is NULL"),
                     (dict(base=None), b"base is NULL"), (dict(lost=None), b"d_lost is NULL"),
                     (dict(rec=None), b"d_records is NULL"), (dict(out=None), b"d_out is NULL"),
                     (dict(wk=None), b"d_work is NULL"), (dict(rep=None), b"d_report is NULL"),
                     (dict(B=-1), b"B = -1"), (dict(S=-1), b"S = -1"), (dict(R=-1), b"R = -1"),
                     (dict(ml=-1), b"max_len = -1"), (dict(nb=-1), b"out_bytes = -1"),
                     (dict(B=1 << 31, ml=0), b"not below 2^31"), (dict(ml=65), b"max_len = 65 exceeds B = 64"),
                     (dict(rec=ctypes.c_void_p(0x30004)), b"8-byte aligned"),
                     (dict(wk=ctypes.c_void_p(0x50010)), b"32-byte aligned"),
                     (dict(ids=ints(0, -1, 2, 3)), b"negative id"),
                     (dict(ids=ints(0, 1, 1, 3)), b"src_ids names block 1 twice"),
                     (dict(R=(1 << 31) - 1, B=1 << 20, ml=1 << 20), b"2^31 - 1 workgroups")):
        assert matrix_batch(**kw) == EINVAL, kw
        assert _err(ecg).startswith(b"dread: ") and text in _err(ecg), (kw, _err(ecg))
    assert matrix_batch(R=0) == 0 and matrix_batch(R=0, wk=None) == 0                    # no record: a no-op
    assert matrix_batch(r=8, n=128, H=wide, ids=wide_ids, R=0) == 0                      # the largest shape is accepted

    M = ints(*([1] * (9 * 127)))

    def encode_batch(k=2, m=1, matrix=M, base=dev, B=64, S=1, f=lost, r=rec, R=1, ml=64, o=out, nb=64, w=wk, v=rep):
        return L.ecg_dread_encode_batch(k, m, matrix, base, 4096, 1024, B, S, f, r, R, ml, o, nb, w, v, None)

    for kw, text in ((dict(k=0), b"k = 0"), (dict(m=0), b"m = 0"), (dict(matrix=None), b"matrix is NULL"),
                     (dict(base=None), b"base is NULL"), (dict(v=None), b"d_report is NULL"), (dict(B=-1), b"B = -1"),
                     (dict(S=-1), b"S = -1"), (dict(B=1 << 31), b"2^31"), (dict(m=9), b"r = 9"),
                     (dict(k=127, m=2), b"n = 129"), (dict(k=1 << 30, m=8), b"n = 1073741832"),
                     (dict(f=None), b"d_lost"), (dict(r=None), b"d_records"), (dict(o=None), b"d_out"),
                     (dict(w=None), b"d_work"), (dict(ml=65), b"max_len")):
        assert encode_batch(**kw) == EINVAL, kw
        assert text in _err(ecg), (kw, _err(ecg))
    assert encode_batch(R=0) == 0 and encode_batch(k=120, m=8, R=0) == 0

    code = ecg.ec_factory(0, ecg.CodingParameters(k=6, m=4))
    tail = (4096, 256, 64, 1, lost, rec, 1, 64, out, 64, wk, rep, None)
    assert L.ecg_dread_ec_batch(None, dev, *tail) == EINVAL and b"ec is NULL" in _err(ecg)
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_HOST, None)
    assert L.ecg_dread_ec_batch(code._h, dev, *tail) == EINVAL and b"ECG_MEM_DEVICE" in _err(ecg)
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, None)
    assert L.ecg_dread_ec_batch(code._h, None, *tail) == EINVAL and b"base is NULL" in _err(ecg)
    assert L.ecg_dread_ec_batch(code._h, dev, 4096, 256, 64, 1, lost, rec, 0, 64, out, 64, wk, rep, None) == 0

    flags = (ctypes.c_ubyte * 4)(0, 1, 0, 0)
    c = (ctypes.c_ubyte * 4)()
    for args, text in (((4, 2, None, flags, 1, c, None), b"H is NULL"), ((4, 2, H, None, 1, c, None), b"h_lost is NULL"),
                       ((4, 2, H, flags, 1, None, None), b"c_out is NULL"), ((4, 2, H, flags, 4, c, None), b"col = 4"),
                       ((4, 2, H, flags, -1, c, None), b"col = -1"), ((4, 9, H, flags, 1, c, None), b"r = 9"),
                       ((129, 2, H, flags, 1, c, None), b"n = 129")):
        assert L.ecg_dread_plan(*args) == EINVAL, args
        assert text in _err(ecg), (args, _err(ecg))
    assert L.ecg_dread_plan(4, 2, H, flags, 1, c, None) == 0 and list(c) == [1, 0, 1, 0]   # row 0 without column 3


@pytest.mark.parametrize("name", ["PC(4,2,2,1)", "HPC(4,2,2,1|2,1)", "PC(4,1,4,1)"])
def test_classes_with_more_than_eight_checks_are_refused(ecg, dread, name):
    c = next(c for c in GOLDEN if c["name"] == name)
    code = ecg.ec_factory(c["type"], ecg.CodingParameters(**c["params"]))
    assert code.m > K_MAX_R
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, None)
    dev, lost, rec, out, wk, rep = (ctypes.c_void_p(0x10000 * i) for i in (1, 2, 3, 4, 5, 6))
    assert dread.lib().ecg_dread_ec_batch(code._h, dev, 1 << 20, 4096, 64, 1, lost, rec, 1, 64, out, 64, wk, rep,
                                          None) == ecg.ECG_EINVAL
    assert _err(ecg).startswith(b"dread: r = %d" % code.m) and b"ecg_ec_decode" in _err(ecg)


# ---- the host helpers

@pytest.mark.parametrize("c", TDP.CODES, ids=[c["name"] for c in TDP.CODES])
def test_plan_equals_the_plain_plan(dread, c):
    k, m = c["k"], c["m"]
    n = k + m
    H = DP.check_of(c["matrix"], k, m)
    for E, col in TDP.cases(c):
        lost = np.zeros(n, bool)
        lost[E] = True
        want_state, want_reads, want_c, _ = DP.plan(H, lost, col)
        state, reads, coef = dread.plan(H, lost, col)
        assert (state, reads) == (want_state, want_reads) and coef.tolist() == want_c.tolist(), (E, col)
    lost = np.zeros(n, bool)
    lost[[0, n - 1]] = True
    state, reads, coef = dread.plan(H, lost, 1)                                          # a present column: the copy
    assert (state, reads) == (0, 1) and coef.tolist() == [int(j == 1) for j in range(n)]


def test_plan_on_a_wide_check(dread):
    """n = 128, r = 8 Cauchy: lanes past 64 of the device's plan have their host counterpart here."""
    import heal2_plain as P2
    k, m = 120, 8
    H = DP.check_of(P2.cauchy(m, k), k, m)
    rng = np.random.default_rng(128)
    for t in (1, 8, 9):
        for _ in range(4):
            E = sorted(int(v) for v in rng.choice(k + m, t, replace=False))
            lost = np.zeros(k + m, bool)
            lost[E] = True
            for col in (E[0], E[-1]):
                want_state, want_reads, want_c, _ = DP.plan(H, lost, col)
                state, reads, coef = dread.plan(H, lost, col)
                assert (state, reads) == (want_state, want_reads) and coef.tolist() == want_c.tolist(), (E, col)
                assert state == (0 if t <= 8 else 6) and reads == (k if t <= 8 else 0)


def test_check_records_answers_the_plain_helper(ecg, dread):
    n, B, S, ml, nb = 6, 64, 3, 16, 40
    ok = [[0, 0, 0, 5, 0], [0, 1, 5, 4, 5], [1, 0, 0, 5, 9], [0, 2, 20, 0, 0]]            # touching ranges are legal
    cases = [(ok, b"")]
    for state, rec in ((1, [-1, 0, 30, 2, 20]), (1, [S, 0, 30, 2, 20]), (2, [2, n, 30, 2, 20]), (2, [2, -1, 30, 2, 20]),
                       (3, [2, 0, -1, 2, 20]), (3, [2, 0, 30, -2, 20]), (3, [2, 0, B - 1, 2, 20]),
                       (4, [2, 0, 30, ml + 1, 0]), (5, [2, 0, 30, 2, -1]), (5, [2, 0, 30, 2, nb - 1])):
        cases.append((ok + [rec] + ok, f"state {state}".encode()))
    cases += [(ok + [[0, 3, 8, 2, 13]], b"overlaps an earlier record's out range"),
              (ok + [[2, 3, 8, 2, 14]], b""),                                            # [14,16) touches [9,14)
              (ok + [[0, 0, 0, 5, 20]], b""),                                            # the same bytes twice: legal
              ([[0, 0, 4, 4, 10], [1, 0, 0, 16, 0]], b"record 1 overlaps"),
              ([[0, 0, 0, 16, 8], [1, 0, 0, 1, 0], [2, 0, 4, 4, 20]], b"record 2 overlaps")]
    rng = np.random.default_rng(3)
    for _ in range(40):                                                                  # random sets, mostly conflicting
        k = int(rng.integers(1, 9))
        recs = np.stack([rng.integers(0, S, k), rng.integers(0, n, k), rng.integers(0, 50, k), rng.integers(0, 12, k),
                         rng.integers(0, 36, k)], axis=1)
        cases.append((recs.tolist(), b""))
    hits = 0
    for recs, text in cases:
        want = DP.check_records(recs, n, B, S, ml, nb)
        assert dread.check_records(recs, n, B, S, ml, nb) == want, recs
        hits += want >= 0
        if want >= 0 and text:
            assert _err(ecg).startswith(b"dread: record %d " % want) and text in _err(ecg), (recs, _err(ecg))
    assert 10 < hits < len(cases)
    assert dread.check_records(np.zeros((0, 5), np.int64), n, B, S, ml, nb) == -1
    assert dread.lib().ecg_dread_check_records(None, 3, n, B, S, ml, nb) == ecg.ECG_EINVAL
    assert dread.lib().ecg_dread_check_records(None, -1, n, B, S, ml, nb) == ecg.ECG_EINVAL
