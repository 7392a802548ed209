"""Corruption localisation, the parts that need no GPU: libecg_locate.so's exports and code object, the argument
checks, the verdict rule, the definition (tests/locate_plain.py) on hand cases, and the census of proportional
columns over the golden RS / ERS / LRC checks that makes a single damaged block nameable.
"""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import gf_plain
import locate_plain as LP
import test_kernel_resources as KR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
MATRIX_CODES = [c for c in GOLDEN if "matrix" in c]       # RS, ERS and the LRC family: H = [matrix | I]
K_MAX_R, K_MAX_N = 8, 128                                  # gf_kernels.hpp kMaxMT, kInlineSrc
MODE_INLINE, MODE_STRIDED = 0, 2                           # gf_kernels.hpp enum GfMode
B = 96


@pytest.fixture(scope="module")
def locate(ecg):
    import ecg_locate
    ecg_locate.lib()
    return ecg_locate


def _golden(name):
    return next(c for c in GOLDEN if c["name"] == name)


def _H(c):
    """[matrix | I] of a golden code, from the oracle's matrix."""
    k, m = c["k"], c["m"]
    return np.concatenate([np.asarray(c["matrix"], dtype=np.int64).reshape(m, k), np.eye(m, dtype=np.int64)], axis=1)


def _stripe(c, seed=1):
    """[k + m][B] uint8 satisfying H: seeded data and gf_plain's product of the golden matrix."""
    k, m = c["k"], c["m"]
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, (k, B), dtype=np.uint8)
    return np.concatenate([data, gf_plain.apply(np.asarray(c["matrix"]).reshape(m, k), data)])


# ---- the library

def test_last_launch_reports_six_fields(locate):
    """The field count without a buffer; a buffer that is too small stays untouched; the binding names the fields in
    the header's order."""
    L = locate.lib()
    assert L.ecg_locate_last_launch(None, 0) == 6
    small = (ctypes.c_int * 5)(*([77] * 5))
    assert L.ecg_locate_last_launch(small, 5) == 6 and list(small) == [77] * 5
    full = (ctypes.c_int * 8)(*([77] * 8))
    assert L.ecg_locate_last_launch(full, 8) == 6 and list(full)[6:] == [77, 77]
    got = locate.last_launch()
    assert list(got) == ["grid_map", "map_group", "cols_per_wg", "wg_per_stripe", "S", "rtiles"]
    assert list(got.values()) == list(full)[:6] and all(v >= 0 for v in got.values())
    hdr = open(os.path.join(ROOT, "include", "ecg_locate.h")).read()
    assert re.findall(r"v\[(\d)\] (\w+)", hdr) == [(str(i), name) for i, name in enumerate(got)]


def test_header_symbols_exported(locate):
    hdr = open(os.path.join(ROOT, "include", "ecg_locate.h")).read()
    declared = sorted(set(re.findall(r"\b(ecg_locate_\w+)\s*\(", hdr)))
    assert len(declared) == 7
    assert sorted(locate.EXPORTS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", locate.LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r" T (ecg_\w+)", out)))
    assert exported == declared
    for status in ("ECG_LOCATE_CLEAN", "ECG_LOCATE_AMBIGUOUS", "ECG_LOCATE_MULTIPLE"):
        value = int(re.search(rf"#define {status} \((-\d+)\)", hdr).group(1))
        assert value == getattr(locate, status[len("ECG_LOCATE_"):]) == getattr(LP, status[len("ECG_LOCATE_"):])
        assert value < -5                                  # apart from the ECG_E* codes
    # libecg.so and libecg_scrub.so need nothing from the locate library
    for so in (KR.LIB, os.path.join(os.path.dirname(KR.LIB), "libecg_scrub.so")):
        need = subprocess.run(["readelf", "-d", so], capture_output=True, text=True).stdout
        assert "NEEDED" in need and "libecg_locate" not in need, so
    need = subprocess.run(["readelf", "-d", locate.LIB_PATH], capture_output=True, text=True).stdout
    assert "libecg.so" in need and "libecg_scrub" not in need


@pytest.fixture(scope="module")
def meta(locate):
    """Kernel metadata of libecg_locate.so's gfx950 code object, read as tests/test_kernel_resources.py reads
    libecg.so's."""
    saved = KR.LIB
    KR.LIB = locate.LIB_PATH
    try:
        return KR._metadata()
    finally:
        KR.LIB = saved


def test_code_object_is_the_locate_family(meta):
    keys, rest = [], []
    for s in meta:
        v = re.search(r"gf_locate_kernelILi(\d+)ELi(\d+)EE", s)
        b = re.search(r"gf_locate_byte_kernelILi(\d+)ELi(\d+)EE", s)
        if v:
            keys.append(("vec",) + tuple(map(int, v.groups())))
        elif b:
            keys.append(("byte",) + tuple(map(int, b.groups())))
        else:
            rest.append(s)
    assert not rest, rest
    want = {(kind, r, mode) for kind in ("vec", "byte") for r in range(1, K_MAX_R + 1)
            for mode in (MODE_INLINE, MODE_STRIDED)}
    assert len(keys) == len(set(keys)) == 32
    assert set(keys) == want
    for name in ("gf_vec_kernel", "gf_byte_kernel", "gf_lat_dword_kernel", "gf_scrub"):
        assert not [s for s in meta if name in s], name


def test_locate_kernels_do_not_spill(meta):
    bad = {n: f for n, f in meta.items() if f.get("private_segment_fixed_size", 0) or f.get("vgpr_spill_count", 0)}
    assert not bad, list(bad)[:5]
    head = {n: f for n, f in meta.items() if re.search(r"gf_locate_kernelILi[1-4]ELi2EE", n)}
    assert len(head) == 4
    assert all(f["sgpr_spill_count"] == 0 for f in head.values()), head
    # the counters are three statically indexed registers per lane, not LDS
    assert all(f.get("group_segment_fixed_size", 0) == 0 for f in meta.values())


# ---- arguments (no GPU is touched: every call returns before the first HIP call)

def test_bad_arguments(ecg, locate):
    L, EINVAL = locate.lib(), ecg.ECG_EINVAL
    H = (ctypes.c_int * 4)(1, 1, 1, 1)
    ids = (ctypes.c_int * 2)(0, 1)
    dev, votes, sel = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000)  # never read
    ok = dict(n=2, r=2, H=H, ids=ids, base=dev, ss=4096, bs=1024, B=64, sel=sel, S=1, votes=votes)

    def matrix_batch(**kw):
        a = dict(ok, **kw)
        return L.ecg_locate_matrix_batch(a["n"], a["r"], a["H"], a["ids"], a["base"], a["ss"], a["bs"], a["B"],
                                         a["sel"], a["S"], a["votes"], None)

    for kw in (dict(n=0), dict(r=0), dict(H=None), dict(ids=None), dict(base=None), dict(votes=None), dict(B=-1),
               dict(S=-1), dict(B=1 << 31), dict(B=(1 << 40) + 16), dict(n=-3), dict(r=-1)):
        assert matrix_batch(**kw) == EINVAL, kw
    assert matrix_batch(S=0) == 0 and matrix_batch(B=0) == 0            # empty: a no-op
    assert matrix_batch(S=0, sel=None) == 0                            # a NULL selection is the identity
    wide = (ctypes.c_int * (9 * 129))(*([1] * (9 * 129)))
    wide_ids = (ctypes.c_int * 129)(*range(129))
    assert matrix_batch(r=9, n=12, H=wide, ids=wide_ids) == EINVAL      # r > 8
    assert b"r = 9" in ecg.lib().ecg_last_error()
    assert matrix_batch(r=2, n=129, H=wide, ids=wide_ids) == EINVAL     # n > 128
    assert b"n = 129" in ecg.lib().ecg_last_error()
    assert matrix_batch(r=8, n=128, H=wide, ids=wide_ids, S=0) == 0     # the largest shape is accepted

    M = (ctypes.c_int * (9 * 127))(*([1] * (9 * 127)))

    def encode_batch(k=2, m=1, matrix=M, base=dev, B=64, S=1, v=votes, ids=sel):
        return L.ecg_locate_encode_batch(k, m, matrix, base, 4096, 1024, B, ids, S, v, None)

    for kw in (dict(k=0), dict(m=0), dict(matrix=None), dict(base=None), dict(v=None), dict(B=-1), dict(S=-1),
               dict(B=1 << 31), dict(m=9), dict(k=127, m=2), dict(k=1 << 30, m=8)):
        assert encode_batch(**kw) == EINVAL, kw
    assert encode_batch(S=0) == 0 and encode_batch(B=0) == 0 and encode_batch(S=0, ids=None) == 0
    assert encode_batch(k=120, m=8, S=0) == 0

    code = ecg.ec_factory(0, ecg.CodingParameters(k=6, m=4))
    assert L.ecg_locate_ec_batch(None, dev, 4096, 256, 64, sel, 1, votes, None) == EINVAL
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_HOST, None)
    assert L.ecg_locate_ec_batch(code._h, dev, 4096, 256, 64, sel, 1, votes, None) == EINVAL      # host handle
    ptrs = (ctypes.c_void_p * 6)(*[0x10000 + 256 * i for i in range(6)])
    cptrs = (ctypes.c_void_p * 4)(*[0x20000 + 256 * i for i in range(4)])
    assert L.ecg_locate_ec(code._h, ptrs, cptrs, 64, votes) == EINVAL                             # host handle
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, None)
    for args in ((None, 4096, 256, 64, sel, 1, votes), (dev, 4096, 256, -1, sel, 1, votes),
                 (dev, 4096, 256, 64, sel, -1, votes), (dev, 4096, 256, 1 << 31, sel, 1, votes),
                 (dev, 4096, 256, 64, sel, 1, None)):
        assert L.ecg_locate_ec_batch(code._h, *args, None) == EINVAL, args
    assert L.ecg_locate_ec_batch(code._h, dev, 4096, 256, 64, None, 0, votes, None) == 0
    assert L.ecg_locate_ec_batch(code._h, dev, 4096, 256, 0, sel, 3, votes, None) == 0
    assert L.ecg_locate_ec(code._h, None, cptrs, 64, votes) == EINVAL
    assert L.ecg_locate_ec(code._h, ptrs, None, 64, votes) == EINVAL
    assert L.ecg_locate_ec(code._h, ptrs, cptrs, -1, votes) == EINVAL
    assert L.ecg_locate_ec(code._h, ptrs, cptrs, 64, None) == EINVAL
    assert L.ecg_locate_ec(code._h, ptrs, cptrs, 0, votes) == 0
    holed = (ctypes.c_void_p * 6)(*[0x10000, 0x10100, None, 0x10300, 0x10400, 0x10500])
    assert L.ecg_locate_ec(code._h, holed, cptrs, 64, votes) == EINVAL

    n = [ctypes.c_longlong(-1), ctypes.c_longlong(-1)]
    assert L.ecg_locate_counters(ctypes.byref(n[0]), ctypes.byref(n[1])) == 0 and n[0].value >= 0 and n[1].value >= 0
    assert L.ecg_locate_counters(None, None) == 0


@pytest.mark.parametrize("name", ["PC(4,2,2,1)", "HPC(4,2,2,1|2,1)", "PC(4,1,4,1)"])
def test_product_codes_with_more_than_eight_checks_are_refused(ecg, locate, name):
    c = _golden(name)
    code = ecg.ec_factory(c["type"], ecg.CodingParameters(**c["params"]))
    assert code.m > K_MAX_R
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, None)
    dev, votes = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)
    assert locate.lib().ecg_locate_ec_batch(code._h, dev, 1 << 20, 4096, 64, None, 1, votes, None) == ecg.ECG_EINVAL
    assert f"r = {code.m}".encode() in ecg.lib().ecg_last_error()
    ptrs = (ctypes.c_void_p * code.k)(*[0x10000 + 256 * i for i in range(code.k)])
    cptrs = (ctypes.c_void_p * code.m)(*[0x20000 + 256 * i for i in range(code.m)])
    assert locate.lib().ecg_locate_ec(code._h, ptrs, cptrs, 64, votes) == ecg.ECG_EINVAL


# ---- verdict

def test_verdict_on_hand_written_votes(ecg, locate):
    n = 5
    cases = [
        ([0, 0, 0, 0, 0, 0, 0], LP.CLEAN, []),
        ([0, 0, 7, 0, 0, 7, 0], 2, [2]),                                  # one block explains all 7
        ([9, 0, 0, 0, 0, 9, 0], 0, [0]),
        ([4, 4, 4, 4, 4, 4, 0], LP.AMBIGUOUS, [0, 1, 2, 3, 4]),           # r = 1: every block explains everything
        ([0, 6, 0, 6, 0, 6, 0], LP.AMBIGUOUS, [1, 3]),
        ([3, 0, 0, 0, 5, 8, 0], LP.MULTIPLE, [0, 4]),                     # two blocks at disjoint positions
        ([0, 0, 0, 0, 0, 3, 3], LP.MULTIPLE, []),                         # nothing explains anything
        ([0, 5, 0, 0, 0, 6, 1], LP.MULTIPLE, [1]),                        # one unexplained position
        ([0, 6, 0, 2, 0, 6, 0], 1, [1, 3]),                               # block 1 explains all, block 3 a few too
        ([0, 0xFFFFFFFF, 0, 0, 0, 0xFFFFFFFF, 0], 1, [1]),                # counters are unsigned
    ]
    for v, status, ids in cases:
        assert locate.verdict(v) == (status, ids), v
        assert LP.verdict(v) == (status, ids), v
    assert locate.verdict(np.array(cases[1][0], dtype=np.int32)) == (2, [2])
    # the C entry point: the count comes back when the buffer is too small, and nothing is written
    L = locate.lib()
    v = (ctypes.c_uint * (n + 2))(3, 0, 0, 0, 5, 8, 0)
    ids = (ctypes.c_int * 2)(-1, -1)
    got = ctypes.c_int(-1)
    assert L.ecg_locate_verdict(n, v, ids, 1, ctypes.byref(got)) == LP.MULTIPLE
    assert got.value == 2 and list(ids) == [-1, -1]
    assert L.ecg_locate_verdict(n, v, ids, 2, ctypes.byref(got)) == LP.MULTIPLE and list(ids) == [0, 4]
    assert L.ecg_locate_verdict(n, v, None, 0, None) == LP.MULTIPLE
    for args in ((0, v, ids, 2, None), (n, None, ids, 2, None), (n, v, ids, -1, None), (n, v, None, 2, None)):
        assert L.ecg_locate_verdict(*args) == ecg.ECG_EINVAL, args


# ---- the definition on hand cases

def test_plain_rs_10_4_names_a_data_block_and_a_parity_block():
    c = _golden("RS(10,4)")
    H, stripe = _H(c), _stripe(c)
    n = 14
    assert not LP.votes(H, stripe).any() and LP.verdict(LP.votes(H, stripe)) == (LP.CLEAN, [])
    for b in (3, 0, 9, 12, 13):                            # data blocks, parity blocks
        bad = stripe.copy()
        bad[b, 40] ^= 0x80
        bad[b, 41] ^= 0x01
        bad[b, B - 1] ^= 0xFF
        v = LP.votes(H, bad)
        want = np.zeros(n + 2, np.int64)
        want[b] = want[n] = 3
        assert np.array_equal(v, want), (b, v)
        assert LP.verdict(v) == (b, [b])


def test_plain_rs_8_1_every_block_ties():
    c = _golden("RS(8,1)")
    H, stripe = _H(c), _stripe(c)
    stripe[5, 17] ^= 0x42
    v = LP.votes(H, stripe)
    assert list(v) == [1] * 9 + [1, 0]
    assert LP.verdict(v) == (LP.AMBIGUOUS, list(range(9)))


def test_plain_two_blocks_at_disjoint_positions():
    c = _golden("RS(10,4)")
    H, stripe = _H(c), _stripe(c)
    stripe[2, 10:14] ^= 0x11
    stripe[11, 50:57] ^= 0x22
    v = LP.votes(H, stripe)
    want = np.zeros(16, np.int64)
    want[2], want[11], want[14] = 4, 7, 11
    assert np.array_equal(v, want), v
    assert LP.verdict(v) == (LP.MULTIPLE, [2, 11])


def test_plain_two_blocks_at_the_same_position_are_unexplained_with_r_4():
    """Any 3 columns of an MDS check with r >= 3 are independent: e1 h1 + e2 h2 is no multiple of a third column,
    nor of h1 or h2."""
    c = _golden("RS(10,4)")
    H, stripe = _H(c), _stripe(c)
    stripe[2, 30] ^= 0x5A
    stripe[7, 30] ^= 0xC3
    v = LP.votes(H, stripe)
    want = np.zeros(16, np.int64)
    want[14] = want[15] = 1
    assert np.array_equal(v, want), v
    assert LP.verdict(v) == (LP.MULTIPLE, [])


def test_plain_zero_column_explains_nothing():
    H = np.array([[1, 0, 3], [2, 0, 1]])
    stripe = np.zeros((3, 8), np.uint8)
    stripe[1, 2] = 9                                       # damage in the block no row covers: invisible
    assert not LP.votes(H, stripe).any()
    stripe[0, 3] = 1
    assert list(LP.votes(H, stripe)) == [1, 0, 0, 1, 0]


# ---- why a single damaged block can be named: no two proportional columns

@pytest.mark.parametrize("c", MATRIX_CODES, ids=[c["name"] for c in MATRIX_CODES])
def test_proportional_column_census(ecg, c):
    H = _H(c)
    pairs, zero = LP.proportional_pairs(H)
    assert zero == 0
    n = c["k"] + c["m"]
    assert pairs == (n * (n - 1) // 2 if c["m"] == 1 else 0), c["name"]
    if c["name"] == "RS(8,1)":
        assert pairs == 36
    # the library's own check matrix is the same one
    code = ecg.ec_factory(c["type"], ecg.CodingParameters(**c["params"]))
    assert np.array_equal(np.asarray(code.check_matrix()), H)


def test_census_covers_the_codes_it_claims():
    assert [c["name"] for c in MATRIX_CODES] == [
        "RS(6,2)", "RS(6,4)", "RS(10,4)", "RS(12,4)", "RS(8,1)", "ERS(8,2|2,0)", "ERS(8,2|2,1)", "Azure(8,2,2)",
        "Azure(12,2,2)", "Azure+1(8,3,2)", "Optimal(8,2,2)", "OptCauchy(8,2,2)", "UniCauchy(8,2,2)"]
