"""Two-block correction, the parts that need no GPU: libecg_heal2.so's exports and code object, every argument
refusal, and the independence tests -- ANY2 needs every 4 columns of the check independent, TARGET2 every 3 -- which
are answered before any device is touched and must agree with tests/heal2_plain.py's plain rank on every golden code.
"""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import heal2_plain as P
import test_kernel_resources as KR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
MIN_R, MAX_R, MAX_N = 3, 8, 32                              # heal2_kernels.hpp kHeal2MinR, kMaxMT, kHeal2MaxN
MODE_INLINE, MODE_STRIDED = 0, 2                           # gf_kernels.hpp enum GfMode


@pytest.fixture(scope="module")
def heal2(ecg):
    import ecg_heal2
    ecg_heal2.lib()
    return ecg_heal2


# ---- the library

def test_header_symbols_exported(heal2):
    hdr = open(os.path.join(ROOT, "include", "ecg_heal2.h")).read()
    declared = sorted(set(re.findall(r"\b(ecg_heal2_\w+)\s*\(", hdr)))
    assert len(declared) == 6
    assert sorted(heal2.EXPORTS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", heal2.LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r" T (ecg_\w+)", out)))
    assert exported == declared
    # the other four libraries need nothing from this one, and it needs only libecg.so
    lib_dir = os.path.dirname(KR.LIB)
    for name in ("libecg.so", "libecg_scrub.so", "libecg_locate.so", "libecg_heal.so"):
        need = subprocess.run(["readelf", "-d", os.path.join(lib_dir, name)], capture_output=True, text=True).stdout
        assert "NEEDED" in need and "libecg_heal2" not in need, name
    need = subprocess.run(["readelf", "-d", heal2.LIB_PATH], capture_output=True, text=True).stdout
    assert re.findall(r"NEEDED.*\[(libecg\w*\.so)\]", need) == ["libecg.so"]


def test_the_other_libraries_keep_their_symbol_sets(heal2):
    lib_dir = os.path.dirname(KR.LIB)
    for name, header in (("libecg_scrub.so", "ecg_scrub.h"), ("libecg_locate.so", "ecg_locate.h"),
                         ("libecg_heal.so", "ecg_heal.h")):
        prefix = header[:-2]
        hdr = open(os.path.join(ROOT, "include", header)).read()
        declared = sorted(set(re.findall(rf"\b({prefix}_\w+)\s*\(", hdr)))
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(lib_dir, name)], capture_output=True,
                             text=True).stdout
        assert sorted(set(re.findall(r" T (ecg_\w+)", out))) == declared, name
    out = subprocess.run(["nm", "-D", "--defined-only", KR.LIB], capture_output=True, text=True).stdout
    assert not re.findall(r" T (ecg_heal2\w*)", out)


def test_last_launch_reports_six_fields(heal2):
    L = heal2.lib()
    assert L.ecg_heal2_last_launch(None, 0) == 6
    small = (ctypes.c_int * 5)(*([77] * 5))
    assert L.ecg_heal2_last_launch(small, 5) == 6 and list(small) == [77] * 5
    full = (ctypes.c_int * 8)(*([77] * 8))
    assert L.ecg_heal2_last_launch(full, 8) == 6 and list(full)[6:] == [77, 77]
    got = heal2.last_launch()
    assert list(got) == ["grid_map", "map_group", "cols_per_wg", "wg_per_stripe", "S", "rtiles"]
    assert list(got.values()) == list(full)[:6] and all(v >= 0 for v in got.values())
    hdr = open(os.path.join(ROOT, "include", "ecg_heal2.h")).read()
    assert re.findall(r"v\[(\d)\] (\w+)", hdr) == [(str(i), name) for i, name in enumerate(got)]


@pytest.fixture(scope="module")
def meta(heal2):
    """Kernel metadata of libecg_heal2.so's gfx950 code object, read as tests/test_kernel_resources.py reads
    libecg.so's."""
    saved = KR.LIB
    KR.LIB = heal2.LIB_PATH
    try:
        return KR._metadata()
    finally:
        KR.LIB = saved


def test_code_object_is_the_heal2_family(meta):
    keys, rest = [], []
    for s in meta:
        v = re.search(r"gf_heal2_kernelILi(\d+)ELi(\d+)EE", s)
        b = re.search(r"gf_heal2_byte_kernelILi(\d+)ELi(\d+)EE", s)
        if v:
            keys.append(("vec",) + tuple(map(int, v.groups())))
        elif b:
            keys.append(("byte",) + tuple(map(int, b.groups())))
        else:
            rest.append(s)
    assert not rest, rest
    want = {(kind, r, mode) for kind in ("vec", "byte") for r in range(MIN_R, MAX_R + 1)
            for mode in (MODE_INLINE, MODE_STRIDED)}
    assert len(keys) == len(set(keys)) == 24
    assert set(keys) == want


def test_heal2_kernels_do_not_spill(meta):
    bad = {n: f for n, f in meta.items() if f.get("private_segment_fixed_size", 0) or f.get("vgpr_spill_count", 0)}
    assert not bad, list(bad)[:5]
    # the counters are three statically indexed registers per lane, not LDS
    assert all(f.get("group_segment_fixed_size", 0) == 0 for f in meta.values())


# ---- arguments (no GPU is touched: every call returns before the first HIP call)

DEV, REP, SEL, TG = (ctypes.c_void_p(0x10000 * i) for i in (1, 2, 3, 4))   # never read


def _matrix_batch(L, H, targets, S, B=64):
    H = np.asarray(H, dtype=np.int64)
    r, n = H.shape
    flat = (ctypes.c_int * (r * n))(*[int(v) for v in H.reshape(-1)])
    ids = (ctypes.c_int * n)(*range(n))
    return L.ecg_heal2_matrix_batch(n, r, flat, ids, DEV, 1 << 16, 1024, B, SEL, targets, S, REP, None)


def test_bad_arguments(ecg, heal2):
    L, EINVAL = heal2.lib(), ecg.ECG_EINVAL
    Hm = np.concatenate([P.cauchy(4, 2), np.eye(4, dtype=np.int64)], axis=1)
    H = (ctypes.c_int * 24)(*[int(v) for v in Hm.reshape(-1)])
    ids = (ctypes.c_int * 6)(*range(6))
    ok = dict(n=6, r=4, H=H, ids=ids, base=DEV, ss=8192, bs=1024, B=64, sel=SEL, tg=TG, S=1, rep=REP)

    def matrix_batch(**kw):
        a = dict(ok, **kw)
        return L.ecg_heal2_matrix_batch(a["n"], a["r"], a["H"], a["ids"], a["base"], a["ss"], a["bs"], a["B"],
                                        a["sel"], a["tg"], a["S"], a["rep"], None)

    for kw in (dict(n=0), dict(r=0), dict(H=None), dict(ids=None), dict(base=None), dict(rep=None), dict(B=-1),
               dict(S=-1), dict(B=1 << 31), dict(B=(1 << 40) + 16), dict(n=-3), dict(r=-1)):
        assert matrix_batch(**kw) == EINVAL, kw
        assert matrix_batch(tg=None, **kw) == EINVAL, kw
    for tgt in (TG, None):                                             # empty: a no-op, in both modes
        assert matrix_batch(S=0, tg=tgt) == 0 and matrix_batch(B=0, tg=tgt) == 0
        assert matrix_batch(S=0, sel=None, tg=tgt) == 0                # a NULL selection is the identity
    # sizes: 3 <= r <= 8, 2 <= n <= 32 (the matrices are read only once the sizes have passed)
    wide = P.cauchy(9, 33, seed=1)
    flat = (ctypes.c_int * wide.size)(*[int(v) for v in wide.reshape(-1)])
    wide_ids = (ctypes.c_int * 33)(*range(33))
    for r, n, word in ((2, 6, b"r = 2"), (9, 12, b"r = 9"), (8, 33, b"n = 33"), (1, 6, b"r = 1"), (4, 1, b"n = 1"),
                       (8, 129, b"n = 129")):
        for tgt in (TG, None):
            assert matrix_batch(r=r, n=n, H=flat, ids=wide_ids, tg=tgt, S=0) == EINVAL, (r, n)
            assert word in ecg.lib().ecg_last_error()
    for r, n in ((8, 32), (3, 32), (3, 2)):                            # the corners are accepted (TARGET2)
        Hc = P.cauchy(r, n, seed=2)
        assert _matrix_batch(L, Hc, TG, 0) == 0, (r, n)
    assert _matrix_batch(L, P.cauchy(8, 32, seed=2), None, 0) == 0     # and the largest shape in ANY2

    M = (ctypes.c_int * (9 * 31))(*[int(v) for v in P.cauchy(9, 31, seed=3).reshape(-1)])

    def encode_batch(k=2, m=4, matrix=M, base=DEV, B=64, S=1, v=REP, ids=SEL, t=TG):
        return L.ecg_heal2_encode_batch(k, m, matrix, base, 8192, 1024, B, ids, t, S, v, None)

    for kw in (dict(k=0), dict(m=0), dict(matrix=None), dict(base=None), dict(v=None), dict(B=-1), dict(S=-1),
               dict(B=1 << 31), dict(m=9), dict(m=2), dict(k=29, m=4), dict(k=1 << 30, m=8), dict(k=127, m=2)):
        assert encode_batch(**kw) == EINVAL, kw
    Mc = P.cauchy(4, 6, seed=4)
    M6 = (ctypes.c_int * 24)(*[int(v) for v in Mc.reshape(-1)])
    for tgt in (TG, None):
        assert encode_batch(k=6, matrix=M6, S=0, t=tgt) == 0 and encode_batch(k=6, matrix=M6, B=0, t=tgt) == 0
        assert encode_batch(k=6, matrix=M6, S=0, ids=None, t=tgt) == 0

    code = ecg.ec_factory(0, ecg.CodingParameters(k=6, m=4))
    assert L.ecg_heal2_ec_batch(None, DEV, 4096, 256, 64, SEL, TG, 1, REP, None) == EINVAL
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_HOST, None)
    assert L.ecg_heal2_ec_batch(code._h, DEV, 4096, 256, 64, SEL, TG, 1, REP, None) == EINVAL      # host handle
    ptrs = (ctypes.c_void_p * 6)(*[0x10000 + 256 * i for i in range(6)])
    cptrs = (ctypes.c_void_p * 4)(*[0x20000 + 256 * i for i in range(4)])
    assert L.ecg_heal2_ec(code._h, ptrs, cptrs, 64, 3, REP) == EINVAL                              # host handle
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, None)
    for args in ((None, 4096, 256, 64, SEL, TG, 1, REP), (DEV, 4096, 256, -1, SEL, TG, 1, REP),
                 (DEV, 4096, 256, 64, SEL, TG, -1, REP), (DEV, 4096, 256, 1 << 31, SEL, TG, 1, REP),
                 (DEV, 4096, 256, 64, SEL, TG, 1, None)):
        assert L.ecg_heal2_ec_batch(code._h, *args, None) == EINVAL, args
    for tgt in (TG, None):
        assert L.ecg_heal2_ec_batch(code._h, DEV, 4096, 256, 64, None, tgt, 0, REP, None) == 0
        assert L.ecg_heal2_ec_batch(code._h, DEV, 4096, 256, 0, SEL, tgt, 3, REP, None) == 0
    assert L.ecg_heal2_ec(code._h, None, cptrs, 64, 3, REP) == EINVAL
    assert L.ecg_heal2_ec(code._h, ptrs, None, 64, 3, REP) == EINVAL
    assert L.ecg_heal2_ec(code._h, ptrs, cptrs, -1, 3, REP) == EINVAL
    assert L.ecg_heal2_ec(code._h, ptrs, cptrs, 64, 3, None) == EINVAL
    assert L.ecg_heal2_ec(code._h, ptrs, cptrs, 64, 10, REP) == EINVAL                             # target == n
    assert L.ecg_heal2_ec(code._h, ptrs, cptrs, 64, -2, REP) == EINVAL
    for target in (-1, 0, 9):
        assert L.ecg_heal2_ec(code._h, ptrs, cptrs, 0, target, REP) == 0
    holed = (ctypes.c_void_p * 6)(*[0x10000, 0x10100, None, 0x10300, 0x10400, 0x10500])
    assert L.ecg_heal2_ec(code._h, holed, cptrs, 64, 3, REP) == EINVAL

    n = [ctypes.c_longlong(-1), ctypes.c_longlong(-1)]
    assert L.ecg_heal2_counters(ctypes.byref(n[0]), ctypes.byref(n[1])) == 0 and n[0].value >= 0 and n[1].value >= 0
    assert L.ecg_heal2_counters(None, None) == 0


# r = 4, every 3 columns independent, columns 0..3 dependent (column 3 = column 0 ^ column 1 ^ column 2)
_C = P.cauchy(4, 3, seed=5)
H_DEP4 = np.concatenate([_C, (_C[:, 0] ^ _C[:, 1] ^ _C[:, 2])[:, None], np.eye(4, dtype=np.int64)[:, :2]], axis=1)
# a dependent triple: column 2 = column 0 ^ 2 * column 1
H_DEP3 = np.array([[1, 1, 1 ^ 2, 1], [1, 2, 1 ^ 4, 4], [1, 4, 1 ^ 8, 16], [1, 8, 1 ^ 16, 64]], dtype=np.int64)


def test_hand_made_checks_are_what_they_claim():
    assert P.independent(H_DEP4, 3) and P.dependent_set(H_DEP4, 4) == (0, 1, 2, 3)
    assert P.independent(H_DEP3, 2) and P.dependent_set(H_DEP3, 3) == (0, 1, 2)


def test_dependent_columns_are_refused(ecg, heal2):
    """A dependent 4-set: ANY2 refused (whatever S_sel), TARGET2 accepted.  A dependent triple, a zero column, r = 3 in
    ANY2: refused, with the columns named.  Nothing is launched."""
    L, EINVAL = heal2.lib(), ecg.ECG_EINVAL
    l0 = heal2.counters()["launches"]
    for S in (1, 0):
        assert _matrix_batch(L, H_DEP4, None, S) == EINVAL
        msg = ecg.lib().ecg_last_error()
        assert b"columns 0, 1, 2 and 3" in msg and b"dependent" in msg and b"ANY2" in msg, msg
    assert _matrix_batch(L, H_DEP4, TG, 0) == 0
    assert _matrix_batch(L, H_DEP4[:, [0, 1, 2, 4, 5]], None, 0) == 0          # without column 3: independent
    assert _matrix_batch(L, H_DEP4[:, ::-1], None, 1) == EINVAL and b"columns 2, 3, 4 and 5" in \
        ecg.lib().ecg_last_error()
    for tgt in (TG, None):
        assert _matrix_batch(L, H_DEP3, tgt, 1) == EINVAL
        assert b"columns 0, 1 and 2" in ecg.lib().ecg_last_error()
    assert b"TARGET2" in ecg.lib().ecg_last_error() or b"ANY2" in ecg.lib().ecg_last_error()
    Hz = np.concatenate([P.cauchy(4, 3, seed=6), np.eye(4, dtype=np.int64)], axis=1)
    assert _matrix_batch(L, Hz, None, 0) == 0 and _matrix_batch(L, Hz, TG, 0) == 0
    Hz[:, 1] = 0
    for tgt in (TG, None):
        assert _matrix_batch(L, Hz, tgt, 0) == EINVAL and b"column 1 of the check matrix is zero" in \
            ecg.lib().ecg_last_error()
    H3 = np.concatenate([P.cauchy(3, 4, seed=7), np.eye(3, dtype=np.int64)], axis=1)
    assert _matrix_batch(L, H3, TG, 0) == 0                                   # r = 3: TARGET2 only
    assert _matrix_batch(L, H3, None, 0) == EINVAL and b"columns 0, 1, 2 and 3" in ecg.lib().ecg_last_error()
    assert _matrix_batch(L, H3[:, :3], None, 0) == 0                          # three blocks: no 4 columns to depend
    assert heal2.counters()["launches"] == l0


# ---- the census: the library's verdict on every golden code equals the plain rank's

def _in_range(c):
    r, n = c["m"], c["k"] + c["m"]
    return MIN_R <= r <= MAX_R and n <= MAX_N


CENSUS = [c for c in GOLDEN if _in_range(c)]


def library_verdicts(ecg, heal2, c):
    """(ANY2 accepted, TARGET2 accepted) by ecg_heal2_ec_batch with S_sel = 0: no device is touched."""
    code = ecg.ec_factory(c["type"], ecg.CodingParameters(**c["params"]))
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, None)
    got = []
    for tgt in (None, TG):
        rc = heal2.lib().ecg_heal2_ec_batch(code._h, DEV, 1 << 20, 4096, 64, None, tgt, 0, REP, None)
        assert rc in (0, ecg.ECG_EINVAL), (c["name"], rc)
        got.append(rc == 0)
    return code, tuple(got)


@pytest.mark.parametrize("c", CENSUS, ids=[c["name"] for c in CENSUS])
def test_census_of_the_golden_codes(ecg, heal2, c):
    code, got = library_verdicts(ecg, heal2, c)
    H = np.asarray(code.check_matrix(), dtype=np.int64)
    assert H.shape == (c["m"], c["k"] + c["m"])
    want = (P.accepts(H, True), P.accepts(H, False))
    print(f"census: {c['name']}: n = {H.shape[1]}, r = {H.shape[0]}, ANY2 {got[0]}, TARGET2 {got[1]}")
    assert got == want, (c["name"], got, want)
    if not got[1]:
        assert not got[0]                                                    # every 4 implies every 3


def test_the_headline_codes_are_accepted_in_any2(ecg, heal2):
    names = {c["name"] for c in CENSUS}
    assert {"RS(10,4)", "RS(6,4)"} <= names and len(CENSUS) >= 4
    for name in ("RS(10,4)", "RS(6,4)"):
        _, got = library_verdicts(ecg, heal2, next(c for c in GOLDEN if c["name"] == name))
        assert got == (True, True), name


@pytest.mark.parametrize("c", [c for c in GOLDEN if not _in_range(c)],
                         ids=[c["name"] for c in GOLDEN if not _in_range(c)])
def test_codes_outside_the_size_limits_are_refused(ecg, heal2, c):
    code = ecg.ec_factory(c["type"], ecg.CodingParameters(**c["params"]))
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, None)
    for tgt in (None, TG):
        assert heal2.lib().ecg_heal2_ec_batch(code._h, DEV, 1 << 20, 4096, 64, None, tgt, 0, REP, None) != 0
    ptrs = (ctypes.c_void_p * code.k)(*[0x10000 + 256 * i for i in range(code.k)])
    cptrs = (ctypes.c_void_p * code.m)(*[0x20000 + 256 * i for i in range(code.m)])
    assert heal2.lib().ecg_heal2_ec(code._h, ptrs, cptrs, 64, 0, REP) != 0
