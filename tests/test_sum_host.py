"""Block checksums, the parts that need no GPU: libecg_sum.so's exports and code object, the host functions
ecg_sum_crc32c and ecg_sum_combine against the definition (tests/crc32c_plain.py), and every argument refusal.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import crc32c_plain as CP
import test_kernel_resources as KR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODE_INLINE, MODE_STRIDED = 0, 2                           # sum_kernels.hpp enum SumMode
COPIES = int(re.search(r"constexpr int kSumCopies = (\d+);", open(os.path.join(
    ROOT, "erasure-codes-prototype_amd", "csrc", "sum_kernels.hpp")).read()).group(1))   # table scheme 1
# the row tables (one copy; kSumCopies copies) and one word per wave
LDS_BYTES = {1: 4 * 256 * 4 + 2 * 4, COPIES: COPIES * 4 * 256 * 4 + 2 * 4}


@pytest.fixture(scope="module")
def sums(ecg):
    import ecg_sum
    ecg_sum.lib()
    return ecg_sum


# ---- the library

def test_header_symbols_exported(sums):
    hdr = open(os.path.join(ROOT, "include", "ecg_sum.h")).read()
    declared = sorted(set(re.findall(r"\b(ecg_sum_\w+)\s*\(", hdr)))
    assert len(declared) == 11
    assert sorted(sums.EXPORTS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", sums.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r" T (ecg_\w+)", out))) == declared
    need = subprocess.run(["readelf", "-d", sums.LIB_PATH], capture_output=True, text=True).stdout
    needed = re.findall(r"NEEDED.*\[(libecg[^\]]*)\]", need)
    assert needed == ["libecg.so"], needed
    lib_dir = os.path.dirname(KR.LIB)
    for name in ("libecg.so", "libecg_scrub.so", "libecg_locate.so", "libecg_heal.so", "libecg_heal2.so"):
        need = subprocess.run(["readelf", "-d", os.path.join(lib_dir, name)], capture_output=True, text=True).stdout
        assert "NEEDED" in need and "libecg_sum" not in need, name
    out = subprocess.run(["nm", "-D", "--defined-only", KR.LIB], capture_output=True, text=True).stdout
    assert not re.findall(r" T (ecg_sum\w*)", out)


def test_last_launch_reports_five_fields_of_its_own(sums):
    L = sums.lib()
    assert L.ecg_sum_last_launch(None, 0) == 5
    small = (ctypes.c_int * 4)(*([77] * 4))
    assert L.ecg_sum_last_launch(small, 4) == 5 and list(small) == [77] * 4
    full = (ctypes.c_int * 7)(*([77] * 7))
    assert L.ecg_sum_last_launch(full, 7) == 5 and list(full)[5:] == [77, 77]
    got = sums.last_launch()
    assert list(got) == ["path", "segment_bytes", "segments_per_block", "blocks", "table_scheme"]
    assert list(got.values()) == list(full)[:5] and all(v >= 0 for v in got.values())
    hdr = open(os.path.join(ROOT, "include", "ecg_sum.h")).read()
    assert re.findall(r"v\[(\d)\] (\w+)", hdr) == [(str(i), name) for i, name in enumerate(got)]


@pytest.fixture(scope="module")
def meta(sums):
    """Kernel metadata of libecg_sum.so's gfx950 code object, read as tests/test_kernel_resources.py reads
    libecg.so's."""
    saved = KR.LIB
    KR.LIB = sums.LIB_PATH
    try:
        return KR._metadata()
    finally:
        KR.LIB = saved


def test_code_object_is_the_sum_family(meta):
    keys, rest = [], []
    for s in meta:
        v = re.search(r"crc_sum_kernelILi(\d+)ELi(\d+)EE", s)
        b = re.search(r"crc_sum_byte_kernelILi(\d+)EE", s)
        if v:
            keys.append(("vec%s" % v.group(2), int(v.group(1))))
        elif b:
            keys.append(("byte", int(b.group(1))))
        elif "crc_verify_kernel" in s:
            keys.append(("verify", -1))
        else:
            rest.append(s)
    assert not rest, rest
    want = {(kind, mode) for kind in ("vec1", "vec%d" % COPIES, "byte") for mode in (MODE_INLINE, MODE_STRIDED)}
    want |= {("verify", -1)}
    assert len(keys) == len(set(keys)) == 7 and set(keys) == want
    for name in ("gf_vec_kernel", "gf_byte_kernel", "gf_scrub", "gf_locate", "gf_heal"):
        assert not [s for s in meta if name in s], name


def test_sum_kernels_do_not_spill_and_hold_the_stated_lds(meta):
    bad = {n: f for n, f in meta.items() if f.get("private_segment_fixed_size", 0) or f.get("vgpr_spill_count", 0)
           or f.get("sgpr_spill_count", 0)}
    assert not bad, list(bad)
    for name, f in meta.items():
        vec = re.search(r"crc_sum_kernelILi\d+ELi(\d+)EE", name)
        assert f.get("group_segment_fixed_size", 0) == (LDS_BYTES[int(vec.group(1))] if vec else 0), name
        if vec:
            assert f["vgpr_count"] <= 64, (name, f["vgpr_count"])       # eight waves per SIMD
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert all(f"{v} B" in design for v in LDS_BYTES.values())


# ---- the host functions

def test_crc32c_known_answers(sums):
    for data, want in CP.KNOWN:
        assert sums.crc32c(data) == want, data
        assert sums.lib().ecg_sum_crc32c(ctypes.c_char_p(data), len(data)) == want
    assert sums.lib().ecg_sum_crc32c(None, 0) == 0
    assert sums.crc32c(np.arange(32, dtype=np.uint8)) == 0x46DD794E
    assert sums.crc32c(bytearray(b"123456789")) == 0xE3069283


def test_crc32c_every_short_length_and_random_long_ones(sums):
    rng = np.random.default_rng(131)
    pool = rng.integers(0, 256, 70_000 + 8, dtype=np.uint8)
    for n in range(0, 131):
        for shift in (0, 1, 5):                                        # the 8-byte stride from every alignment
            assert sums.crc32c(pool[shift:shift + n]) == CP.bitwise(pool[shift:shift + n].tobytes()), (n, shift)
    lengths = np.array([int(v) for v in rng.integers(131, 70_001, 7)] + [70_000])
    rows = np.stack([pool[i:i + 70_000] for i in range(len(lengths))])    # one walk of the numpy form for them all
    want = CP.many(rows, lengths)
    for i, n in enumerate(lengths):
        assert sums.crc32c(rows[i, :n]) == int(want[i]), n


def test_combine(sums):
    rng = np.random.default_rng(7)
    a = rng.integers(0, 256, 3000, dtype=np.uint8)
    big = rng.integers(0, 256, (1 << 20) + 53, dtype=np.uint8)
    crc_a = sums.crc32c(a)
    assert crc_a == int(CP.many(a))
    for len_b in (0, 1, 2047, 2048, (1 << 20) + 53):
        b = big[:len_b]
        whole = sums.crc32c(np.concatenate([a, b]))
        assert sums.combine(crc_a, sums.crc32c(b), len_b) == whole, len_b
    for split in (0, 1, 17, 2999, 3000):                               # random splits of one buffer
        assert sums.combine(sums.crc32c(a[:split]), sums.crc32c(a[split:]), 3000 - split) == crc_a, split
    # len_b = 2^31 - 1 by composing two combines: B = B1 || B2 of zeros, whose sums the arithmetic of the definition
    # gives without walking them -- crc32c(0^n) = (0xFFFFFFFF * x^(8n)) ^ 0xFFFFFFFF, here by square and multiply
    # over CP's own bit step
    def mul(p, q):
        out = 0
        for i in range(32):
            if (p >> (31 - i)) & 1:
                out ^= q
            q = CP._step(q)
        return out

    def xpow8(n):
        out, sq = 0x80000000, 0x00800000
        while n:
            if n & 1:
                out = mul(out, sq)
            sq = mul(sq, sq)
            n >>= 1
        return out

    def zeros(n):
        return mul(0xFFFFFFFF, xpow8(n)) ^ 0xFFFFFFFF

    assert zeros(32) == 0x8A9136AA and zeros(1) == 0x527D5351 and zeros(0) == 0
    n1, n2 = (1 << 30) + 12345, (1 << 30) - 12346
    assert n1 + n2 == (1 << 31) - 1
    whole = zeros(3000 + n1 + n2) ^ mul(crc_a ^ zeros(3000), xpow8(n1 + n2))   # crc32c(a || 0^(n1+n2)) by linearity
    step1 = sums.combine(crc_a, zeros(n1), n1)
    assert sums.combine(step1, zeros(n2), n2) == whole
    assert sums.combine(crc_a, zeros(n1 + n2), n1 + n2) == whole
    assert sums.combine(crc_a, sums.combine(zeros(n1), zeros(n2), n2), n1 + n2) == whole
    # pieces of 4 GiB and more: bits 32 and up of len_b.  Against the definition's arithmetic, and against two composed
    # combines of lengths below 2^32
    for big_len in (1 << 32, (1 << 32) + 5, (1 << 33) + (1 << 31) + 7, (1 << 40) + 123456789, (1 << 62) + 1):
        whole = zeros(3000 + big_len) ^ mul(crc_a ^ zeros(3000), xpow8(big_len))
        assert sums.combine(crc_a, zeros(big_len), big_len) == whole, big_len
        h1 = big_len // 2
        h2 = big_len - h1
        if h2 < 1 << 32:
            assert sums.combine(sums.combine(crc_a, zeros(h1), h1), zeros(h2), h2) == whole, big_len
    assert sums.combine(0x12345678, 0, 1 << 32) != 0x12345678                 # not dropped
    assert sums.combine(0x12345678, 0, 1 << 32) == sums.combine(sums.combine(0x12345678, 0, 1 << 31), 0, 1 << 31)
    assert sums.lib().ecg_sum_combine(1, 2, -1) == 0 and b"sum:" in sums.ecg.lib().ecg_last_error()


# ---- arguments (no GPU is touched: every call returns before the first HIP call)

def _refused(ecg, rc, *words):
    assert rc == ecg.ECG_EINVAL
    msg = ecg.lib().ecg_last_error()
    assert msg.startswith(b"sum: ") and len(msg) > 8, msg
    for w in words:
        assert w in msg, (w, msg)


def test_bad_arguments(ecg, sums):
    L = sums.lib()
    ids = (ctypes.c_int * 2)(0, 1)
    dev, out, sel, exp, tg, bad = (ctypes.c_void_p(0x10000 * i) for i in range(1, 7))   # never read
    ok = dict(n=2, ids=ids, base=dev, ss=4096, bs=1024, B=64, sel=sel, S=1, out=out, exp=exp, tg=tg, bad=bad)
    l0 = sums.counters()["launches"]

    def blocks_batch(**kw):
        a = dict(ok, **kw)
        return L.ecg_sum_blocks_batch(a["n"], a["ids"], a["base"], a["ss"], a["bs"], a["B"], a["sel"], a["S"],
                                      a["out"], None)

    def verify_batch(**kw):
        a = dict(ok, **kw)
        return L.ecg_sum_verify_batch(a["n"], a["ids"], a["base"], a["ss"], a["bs"], a["B"], a["sel"], a["S"],
                                      a["exp"], a["out"], a["tg"], a["bad"], None)

    refusals = ((dict(n=0), b"n = 0"), (dict(n=-3), b"n = -3"), (dict(ids=None), b"src_ids"),
                (dict(base=None), b"NULL"), (dict(out=None), b"d_sums"), (dict(B=-1), b"negative"),
                (dict(S=-1), b"negative"), (dict(B=1 << 31), b"2^31"), (dict(B=(1 << 40) + 16), b"2^31"))
    for f in (blocks_batch, verify_batch):
        for kw, word in refusals:
            ecg.lib().ecg_last_error()
            _refused(ecg, f(**kw), word)
        assert f(S=0) == 0 and f(B=0) == 0 and f(S=0, sel=None) == 0        # empty: a no-op
    _refused(ecg, verify_batch(exp=None), b"d_expected")
    _refused(ecg, verify_batch(tg=None), b"d_targets")
    _refused(ecg, verify_batch(bad=None), b"d_bad")
    wide_ids = (ctypes.c_int * 300)(*range(300))
    assert blocks_batch(n=300, ids=wide_ids, S=0) == 0                      # the strided form has no n limit

    code = ecg.ec_factory(0, ecg.CodingParameters(k=6, m=4))
    ptrs = (ctypes.c_void_p * 6)(*[0x10000 + 256 * i for i in range(6)])
    cptrs = (ctypes.c_void_p * 4)(*[0x20000 + 256 * i for i in range(4)])

    def ec_batch(h=code._h, base=dev, B=64, S=1, v=out):
        return L.ecg_sum_ec_batch(h, base, 4096, 256, B, sel, S, v, None)

    def verify_ec_batch(h=code._h, base=dev, B=64, S=1, v=out, e=exp, t=tg, b=bad):
        return L.ecg_sum_verify_ec_batch(h, base, 4096, 256, B, sel, S, e, v, t, b, None)

    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_HOST, None)
    _refused(ecg, ec_batch(), b"ECG_MEM_DEVICE")                             # host handles
    _refused(ecg, verify_ec_batch(), b"ECG_MEM_DEVICE")
    _refused(ecg, L.ecg_sum_ec(code._h, ptrs, cptrs, 64, out), b"ECG_MEM_DEVICE")
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, None)
    for f in (ec_batch, verify_ec_batch):
        _refused(ecg, f(h=None), b"handle")
        _refused(ecg, f(base=None), b"NULL")
        _refused(ecg, f(B=-1), b"negative")
        _refused(ecg, f(S=-1), b"negative")
        _refused(ecg, f(B=1 << 31), b"2^31")
        _refused(ecg, f(v=None), b"d_sums")
        assert f(S=0) == 0 and f(B=0) == 0
    _refused(ecg, verify_ec_batch(e=None), b"d_expected")
    _refused(ecg, verify_ec_batch(t=None), b"d_targets")
    _refused(ecg, verify_ec_batch(b=None), b"d_bad")

    _refused(ecg, L.ecg_sum_ec(None, ptrs, cptrs, 64, out), b"handle")
    _refused(ecg, L.ecg_sum_ec(code._h, None, cptrs, 64, out), b"NULL")
    _refused(ecg, L.ecg_sum_ec(code._h, ptrs, None, 64, out), b"NULL")
    _refused(ecg, L.ecg_sum_ec(code._h, ptrs, cptrs, -1, out), b"negative")
    _refused(ecg, L.ecg_sum_ec(code._h, ptrs, cptrs, 64, None), b"d_sums")
    holed = (ctypes.c_void_p * 6)(*[0x10000, 0x10100, None, 0x10300, 0x10400, 0x10500])
    _refused(ecg, L.ecg_sum_ec(code._h, holed, cptrs, 64, out), b"NULL")
    assert L.ecg_sum_ec(code._h, ptrs, cptrs, 0, out) == 0
    wide = ecg.ec_factory(ecg.ECTYPE.RS, ecg.CodingParameters(k=121, m=8))   # n = 129 block pointers
    ecg.lib().ecg_ec_set_memory(wide._h, ecg.ECG_MEM_DEVICE, None)
    wp = (ctypes.c_void_p * 121)(*[0x10000 + 256 * i for i in range(121)])
    wc = (ctypes.c_void_p * 8)(*[0x40000 + 256 * i for i in range(8)])
    _refused(ecg, L.ecg_sum_ec(wide._h, wp, wc, 64, out), b"n = 129")
    assert L.ecg_sum_ec_batch(wide._h, dev, 1 << 20, 256, 64, sel, 0, out, None) == 0   # the strided form takes it

    n = [ctypes.c_longlong(-1), ctypes.c_longlong(-1)]
    assert L.ecg_sum_counters(ctypes.byref(n[0]), ctypes.byref(n[1])) == 0 and n[0].value >= 0 and n[1].value >= 0
    assert L.ecg_sum_counters(None, None) == 0
    assert sums.counters()["launches"] == l0


def test_a_grid_past_the_launch_limit_is_refused_before_anything_happens(ecg, sums):
    """2^20 stripes x 256 blocks x 2^19 forced 2 KiB segments is far beyond 2^31 - 1 workgroups: ECG_EHIP with the
    reason, the counters and the last-launch record unmoved, no device touched (the pointers are never read)."""
    L = sums.lib()
    ids = (ctypes.c_int * 256)(*range(256))
    dev, out = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)
    c0, l0 = sums.counters(), sums.last_launch()
    try:
        sums.set_segment_bytes(2048)
        rc = L.ecg_sum_blocks_batch(256, ids, dev, 1 << 40, 1 << 30, 1 << 30, None, 1 << 20, out, None)
        assert rc == ecg.ECG_EHIP, rc
        assert b"launch_sum" in ecg.lib().ecg_last_error()
        rc = L.ecg_sum_blocks_batch(256, ids, dev, 1 << 40, (1 << 30) + 1, 1 << 30, None, 1 << 20, out, None)
        assert rc == ecg.ECG_EHIP, rc                                   # the byte path's grid too (unaligned stride)
    finally:
        sums.set_segment_bytes(0)
    assert sums.counters() == c0 and sums.last_launch() == l0


def test_set_table_scheme(ecg, sums):
    L = sums.lib()
    try:
        for good in (0, 1, -1):
            assert L.ecg_sum_set_table_scheme(good) == 0
        for bad in (2, -2, 8):
            _refused(ecg, L.ecg_sum_set_table_scheme(bad), str(bad).encode())
    finally:
        sums.set_table_scheme(-1)


def test_set_segment_bytes(ecg, sums):
    L = sums.lib()
    try:
        for good in (2048, 4096, 6144, 1 << 20, 0):
            assert L.ecg_sum_set_segment_bytes(good) == 0
        for bad in (1, 16, 2047, 2049, 3072, -2048, (1 << 20) + 16, 1 << 31):
            _refused(ecg, L.ecg_sum_set_segment_bytes(bad), str(bad).encode())
        with pytest.raises(ecg.EcgError) as e:
            sums.set_segment_bytes(100)
        assert e.value.code == ecg.ECG_EINVAL
    finally:
        sums.set_segment_bytes(0)
