"""Stripe scrubbing, the parts that need no GPU: libecg_scrub.so's exports and code object, the check matrices of
every code class against the oracle's encode and the field's definition (tests/gf_plain.py), the suspects rule,
and argument checking.
"""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import gf_plain
import test_kernel_resources as KR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
B = 96
K_MAX_MT, K_MAX_MT_BIN = 8, 16            # gf_kernels.hpp kMaxMT, kMaxMTBin
MODE_INLINE, MODE_STRIDED = 0, 2          # gf_kernels.hpp enum GfMode: the two modes the check is built for


@pytest.fixture(scope="module")
def scrub(ecg):
    import ecg_scrub
    ecg_scrub.lib()
    return ecg_scrub


# ---- the library

def test_last_launch_reports_six_fields(scrub):
    """The field count without a buffer; a buffer that is too small stays untouched; the binding names the fields in
    the header's order."""
    L = scrub.lib()
    assert L.ecg_scrub_last_launch(None, 0) == 6
    small = (ctypes.c_int * 5)(*([77] * 5))
    assert L.ecg_scrub_last_launch(small, 5) == 6 and list(small) == [77] * 5
    full = (ctypes.c_int * 8)(*([77] * 8))
    assert L.ecg_scrub_last_launch(full, 8) == 6 and list(full)[6:] == [77, 77]
    got = scrub.last_launch()
    assert list(got) == ["grid_map", "map_group", "cols_per_wg", "wg_per_stripe", "S", "rtiles"]
    assert list(got.values()) == list(full)[:6] and all(v >= 0 for v in got.values())
    hdr = open(os.path.join(ROOT, "include", "ecg_scrub.h")).read()
    assert re.findall(r"v\[(\d)\] (\w+)", hdr) == [(str(i), name) for i, name in enumerate(got)]


def test_header_symbols_exported(scrub):
    hdr = open(os.path.join(ROOT, "include", "ecg_scrub.h")).read()
    declared = sorted(set(re.findall(r"\b(ecg_scrub_\w+)\s*\(", hdr)))
    assert len(declared) == 7
    assert sorted(scrub.EXPORTS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", scrub.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (ecg_\w+)", out))
    assert not [s for s in declared if s not in exported]
    # the planning hook lives in libecg.so, and libecg.so needs nothing from the scrub library
    assert "ecg_ec_check_matrix" not in exported
    need = subprocess.run(["readelf", "-d", KR.LIB], capture_output=True, text=True).stdout
    assert "libecg_scrub" not in need


@pytest.fixture(scope="module")
def meta(scrub):
    """Kernel metadata of libecg_scrub.so's gfx950 code object, read as tests/test_kernel_resources.py reads
    libecg.so's."""
    saved = KR.LIB
    KR.LIB = scrub.LIB_PATH
    try:
        return KR._metadata()
    finally:
        KR.LIB = saved


def _enumeration():
    keys = set()
    for kind in ("vec", "byte"):
        for mode in (MODE_INLINE, MODE_STRIDED):
            for b in (0, 1):
                for mt in range(1, (K_MAX_MT_BIN if b else K_MAX_MT) + 1):
                    keys.add((kind, mt, mode, b))
    return keys


def test_code_object_is_the_scrub_family(meta):
    keys, rest = [], []
    for s in meta:
        v = re.search(r"gf_scrub_kernelILi(\d+)ELi(\d+)ELb([01])EE", s)
        b = re.search(r"gf_scrub_byte_kernelILi(\d+)ELi(\d+)ELb([01])EE", s)
        if v:
            keys.append(("vec",) + tuple(map(int, v.groups())))
        elif b:
            keys.append(("byte",) + tuple(map(int, b.groups())))
        else:
            rest.append(s)
    assert not rest, rest
    assert len(keys) == len(set(keys)) == 2 * 2 * (K_MAX_MT + K_MAX_MT_BIN)
    assert set(keys) == _enumeration()
    for name in ("gf_vec_kernel", "gf_byte_kernel", "gf_lat_dword_kernel"):
        assert not [s for s in meta if name in s], name


def test_scrub_kernels_do_not_spill(meta):
    bad = {n: f for n, f in meta.items() if f.get("private_segment_fixed_size", 0) or f.get("vgpr_spill_count", 0)}
    assert not bad, list(bad)[:5]
    head = {n: f for n, f in meta.items() if re.search(r"gf_scrub_kernelILi[1-4]ELi2ELb[01]EE", n)}
    assert len(head) == 8
    assert all(f["sgpr_spill_count"] == 0 for f in head.values()), head


# ---- check matrices

def _encoded_stripe(c):
    """[k + m][B] uint8: seeded data and the oracle's encode of it."""
    from oracle import ec_ref as E
    ec = E.ec_factory(c["type"], E.CodingParameters(**c["params"]))
    rng = np.random.default_rng(len(c["name"]) * 7919 + c["k"] * 31 + c["m"])
    data = [rng.integers(0, 256, B, dtype=np.uint8) for _ in range(ec.k)]
    coding = E.zeros(ec.m, B)
    ec.encode(data, coding, B)
    return np.stack(data + list(coding))


def _facade(ecg, c):
    return ecg.ec_factory(c["type"], ecg.CodingParameters(**c["params"]))


@pytest.mark.parametrize("c", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_check_matrix_against_oracle_encode(ecg, oracle, c):
    ec = _facade(ecg, c)
    k, m = ec.k, ec.m
    H = np.asarray(ec.check_matrix())
    assert H.shape == (m, k + m)
    assert all(H[p, k + p] == 1 for p in range(m))
    stripe = _encoded_stripe(c)
    assert stripe.shape == (k + m, B)
    assert not gf_plain.apply(H, stripe).any(), c["name"]
    for b in range(k + m):
        bad = stripe.copy()
        bad[b, (7 * b + 3) % B] ^= 0x5A
        rows = set(np.flatnonzero(gf_plain.apply(H, bad).any(axis=1)))
        assert rows == set(np.flatnonzero(H[:, b])), (c["name"], b)
        assert rows, (c["name"], b, "a block no check covers")


def test_capi_check_matrix_sizes(ecg):
    ec = _facade(ecg, next(c for c in GOLDEN if c["name"] == "RS(10,4)"))
    L = ecg.lib()
    assert L.ecg_ec_check_matrix(ec._h, None, 0) == 4            # the row count without a buffer
    small = (ctypes.c_int * 8)(*([77] * 8))
    assert L.ecg_ec_check_matrix(ec._h, small, 8) == 4 and list(small) == [77] * 8  # too small: untouched
    assert L.ecg_ec_check_matrix(None, None, 0) == ecg.ECG_EINVAL
    assert L.ecg_ec_check_matrix(ec._h, None, -1) == ecg.ECG_EINVAL
    H = ec.check_matrix()
    M = ec.make_encoding_matrix()
    for p in range(4):
        assert H[p] == M[10 * p:10 * p + 10] + [int(q == p) for q in range(4)]


def test_pc_data_block_sits_in_one_row_check_and_one_column_check(ecg):
    ec = _facade(ecg, next(c for c in GOLDEN if c["name"] == "PC(4,1,4,1)"))
    H = np.asarray(ec.check_matrix())
    rows = list(np.flatnonzero(H[:, 0]))
    # coding order (pc.cpp): k2 * m1 = 4 row parities, then k1 * m2 = 4 column parities, then the global one
    assert len(rows) == 2 and rows[0] < 4 <= rows[1] < 8, rows


# ---- suspects

def _counts(H, stripe):
    return [int(np.count_nonzero(r)) for r in gf_plain.apply(H, stripe)]


def test_suspects(ecg, oracle, scrub):
    rs = next(c for c in GOLDEN if c["name"] == "RS(10,4)")
    H = _facade(ecg, rs).check_matrix()
    stripe = _encoded_stripe(rs)
    assert scrub.suspects(H, _counts(H, stripe)) == []                      # clean
    bad = stripe.copy()
    bad[12, 5] ^= 1
    assert scrub.suspects(H, _counts(H, bad)) == [12]                       # a parity block: itself alone
    bad = stripe.copy()
    bad[3, 40] ^= 0x80
    assert scrub.suspects(H, _counts(H, bad)) == list(range(10))            # a data block: any data block
    assert scrub.suspects(H, [1, 1, 0, 0]) == []                            # rows no single block explains
    pc = next(c for c in GOLDEN if c["name"] == "PC(4,1,4,1)")
    Hp = _facade(ecg, pc).check_matrix()
    sp = _encoded_stripe(pc)
    for b in (0, 6, 15):
        bad = sp.copy()
        bad[b, 11] ^= 0x33
        assert scrub.suspects(Hp, _counts(Hp, bad)) == [b]                  # row x column names the block
    # the C entry point: the count is returned when the buffer is too small, and nothing is written
    L = scrub.lib()
    flat = (ctypes.c_int * 56)(*[v for row in H for v in row])
    cnt = (ctypes.c_uint * 4)(9, 9, 9, 9)
    ids = (ctypes.c_int * 4)(-1, -1, -1, -1)
    assert L.ecg_scrub_suspects(4, 14, flat, cnt, ids, 4) == 10 and list(ids) == [-1] * 4
    assert L.ecg_scrub_suspects(4, 14, flat, cnt, None, 0) == 10


# ---- arguments (no GPU is touched: every call returns before the first HIP call)

def test_bad_arguments(ecg, scrub):
    L, EINVAL = scrub.lib(), ecg.ECG_EINVAL
    H = (ctypes.c_int * 4)(1, 1, 1, 1)
    ids = (ctypes.c_int * 2)(0, 1)
    dev, cnt = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)  # never dereferenced
    ok = dict(k_in=2, r=2, H=H, ids=ids, base=dev, ss=4096, bs=1024, B=64, S=1, cnt=cnt)

    def matrix_batch(**kw):
        a = dict(ok, **kw)
        return L.ecg_scrub_matrix_batch(a["k_in"], a["r"], a["H"], a["ids"], a["base"], a["ss"], a["bs"], a["B"],
                                        a["S"], a["cnt"], None)

    for kw in (dict(k_in=0), dict(r=0), dict(H=None), dict(ids=None), dict(base=None), dict(cnt=None), dict(B=-1),
               dict(S=-1), dict(B=1 << 31), dict(B=(1 << 40) + 16)):
        assert matrix_batch(**kw) == EINVAL, kw
    assert matrix_batch(S=0) == 0 and matrix_batch(B=0) == 0      # empty: a no-op

    M = (ctypes.c_int * 2)(1, 1)

    def encode_batch(k=2, m=1, matrix=M, base=dev, B=64, S=1, counts=cnt):
        return L.ecg_scrub_encode_batch(k, m, matrix, base, 4096, 1024, B, S, counts, None)

    for kw in (dict(k=0), dict(m=0), dict(matrix=None), dict(base=None), dict(counts=None), dict(B=-1), dict(S=-1),
               dict(B=1 << 31)):
        assert encode_batch(**kw) == EINVAL, kw
    assert encode_batch(S=0) == 0 and encode_batch(B=0) == 0

    ec = _facade(ecg, next(c for c in GOLDEN if c["name"] == "RS(6,4)"))
    assert L.ecg_scrub_ec_batch(None, dev, 4096, 256, 64, 1, cnt, None) == EINVAL
    ecg.lib().ecg_ec_set_memory(ec._h, ecg.ECG_MEM_HOST, None)
    assert L.ecg_scrub_ec_batch(ec._h, dev, 4096, 256, 64, 1, cnt, None) == EINVAL       # host handle
    ptrs = (ctypes.c_void_p * 6)(*[0x10000 + 256 * i for i in range(6)])
    cptrs = (ctypes.c_void_p * 4)(*[0x20000 + 256 * i for i in range(4)])
    assert L.ecg_scrub_ec(ec._h, ptrs, cptrs, 64, cnt) == EINVAL                        # host handle
    ecg.lib().ecg_ec_set_memory(ec._h, ecg.ECG_MEM_DEVICE, None)
    for args in ((None, 4096, 256, 64, 1, cnt), (dev, 4096, 256, -1, 1, cnt), (dev, 4096, 256, 64, -1, cnt),
                 (dev, 4096, 256, 1 << 31, 1, cnt), (dev, 4096, 256, 64, 1, None)):
        assert L.ecg_scrub_ec_batch(ec._h, *args, None) == EINVAL, args
    assert L.ecg_scrub_ec_batch(ec._h, dev, 4096, 256, 64, 0, cnt, None) == 0
    assert L.ecg_scrub_ec(ec._h, None, cptrs, 64, cnt) == EINVAL
    assert L.ecg_scrub_ec(ec._h, ptrs, cptrs, -1, cnt) == EINVAL
    assert L.ecg_scrub_ec(ec._h, ptrs, cptrs, 64, None) == EINVAL
    assert L.ecg_scrub_ec(ec._h, ptrs, cptrs, 0, cnt) == 0

    c4 = (ctypes.c_uint * 2)(1, 0)
    assert L.ecg_scrub_suspects(0, 2, H, c4, None, 0) == EINVAL
    assert L.ecg_scrub_suspects(2, 0, H, c4, None, 0) == EINVAL
    assert L.ecg_scrub_suspects(2, 2, None, c4, None, 0) == EINVAL
    assert L.ecg_scrub_suspects(2, 2, H, None, None, 0) == EINVAL
    assert L.ecg_scrub_suspects(2, 2, H, c4, None, -1) == EINVAL
    n = [ctypes.c_longlong(-1), ctypes.c_longlong(-1)]
    assert L.ecg_scrub_counters(ctypes.byref(n[0]), ctypes.byref(n[1])) == 0 and n[0].value >= 0 and n[1].value >= 0
    assert L.ecg_scrub_counters(None, None) == 0


def test_per_stripe_form_is_limited_like_inline_calls(ecg, scrub):
    """k + m above kInlineSrc (128) has no per-stripe form; the strided form has no such limit."""
    ec = ecg.ec_factory(ecg.ECTYPE.RS, ecg.CodingParameters(k=126, m=3))
    ecg.lib().ecg_ec_set_memory(ec._h, ecg.ECG_MEM_DEVICE, None)
    ptrs = (ctypes.c_void_p * 126)(*[0x10000 + 256 * i for i in range(126)])
    cptrs = (ctypes.c_void_p * 3)(*[0x80000 + 256 * i for i in range(3)])
    assert scrub.lib().ecg_scrub_ec(ec._h, ptrs, cptrs, 64, ctypes.c_void_p(0x90000)) == ecg.ECG_EINVAL
