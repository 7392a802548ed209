"""Piece checksums, the parts that need no GPU: libecg_psum.so's exports and code object, the host function
ecg_psum_fold against the definition (tests/crc32c_plain.py), every argument refusal and the span knob.
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
# 7 tables of 4 x 256 words for P < 2048, all 9 for P >= 2048
LDS_BYTES = {"small": 7 * 4 * 256 * 4, "rows": 9 * 4 * 256 * 4, "byte": 0, "verify": 0}
OTHERS = ("libecg.so", "libecg_scrub.so", "libecg_locate.so", "libecg_heal.so", "libecg_heal2.so", "libecg_sum.so")


@pytest.fixture(scope="module")
def psum(ecg):
    import ecg_psum
    ecg_psum.lib()
    yield ecg_psum
    ecg_psum.set_span_bytes(0)


# ---- the library

def test_header_symbols_exported(psum):
    hdr = open(os.path.join(ROOT, "include", "ecg_psum.h")).read()
    declared = sorted(set(re.findall(r"\b(ecg_psum_\w+)\s*\(", hdr)))
    assert len(declared) == 9
    assert sorted(psum.EXPORTS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", psum.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r" T (ecg_\w+)", out))) == declared
    need = subprocess.run(["readelf", "-d", psum.LIB_PATH], capture_output=True, text=True).stdout
    needed = re.findall(r"NEEDED.*\[(libecg[^\]]*)\]", need)
    assert needed == ["libecg.so"], needed
    lib_dir = os.path.dirname(KR.LIB)
    for name in OTHERS:
        need = subprocess.run(["readelf", "-d", os.path.join(lib_dir, name)], capture_output=True, text=True).stdout
        assert "NEEDED" in need and "libecg_psum" not in need, name
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(lib_dir, name)], capture_output=True,
                             text=True).stdout
        assert not re.findall(r" T (ecg_psum\w*)", out), name


def test_last_launch_reports_five_fields_of_its_own(psum):
    L = psum.lib()
    assert L.ecg_psum_last_launch(None, 0) == 5
    small = (ctypes.c_int * 4)(*([77] * 4))
    assert L.ecg_psum_last_launch(small, 4) == 5 and list(small) == [77] * 4
    full = (ctypes.c_int * 7)(*([77] * 7))
    assert L.ecg_psum_last_launch(full, 7) == 5 and list(full)[5:] == [77, 77]
    got = psum.last_launch()
    assert list(got) == ["path", "piece_bytes", "pieces_per_block", "blocks", "span_bytes"]
    assert list(got.values()) == list(full)[:5] and all(v >= 0 for v in got.values())
    hdr = open(os.path.join(ROOT, "include", "ecg_psum.h")).read()
    assert re.findall(r"v\[(\d)\] (\w+)", hdr) == [(str(i), name) for i, name in enumerate(got)]


@pytest.fixture(scope="module")
def meta(psum):
    """Kernel metadata of libecg_psum.so's gfx950 code object, read as tests/test_kernel_resources.py reads
    libecg.so's."""
    saved = KR.LIB
    KR.LIB = psum.LIB_PATH
    try:
        return KR._metadata()
    finally:
        KR.LIB = saved


def _kind(symbol):
    for kind in ("small", "rows", "byte"):
        m = re.search(r"crc_psum_%s_kernelILi(\d+)EE" % kind, symbol)
        if m:
            return kind, int(m.group(1))
    return ("verify", -1) if "crc_pverify_kernel" in symbol else None


def test_code_object_is_the_psum_family(meta):
    keys = [_kind(s) for s in meta]
    assert None not in keys, [s for s in meta if _kind(s) is None]
    want = {(kind, mode) for kind in ("small", "rows", "byte") for mode in (MODE_INLINE, MODE_STRIDED)}
    want |= {("verify", -1)}
    assert len(keys) == len(set(keys)) == 7 and set(keys) == want
    for name in ("gf_vec_kernel", "gf_byte_kernel", "gf_scrub", "gf_locate", "gf_heal", "crc_sum_", "crc_verify"):
        assert not [s for s in meta if name in s], name


def test_psum_kernels_do_not_spill_and_hold_the_stated_lds(meta):
    bad = {n: f for n, f in meta.items() if f.get("private_segment_fixed_size", 0) or f.get("vgpr_spill_count", 0)
           or f.get("sgpr_spill_count", 0)}
    assert not bad, list(bad)
    for name, f in meta.items():
        kind = _kind(name)[0]
        assert f.get("group_segment_fixed_size", 0) == LDS_BYTES[kind], name
        assert f["vgpr_count"] <= 64, (name, f["vgpr_count"])       # registers never bound the resident waves: LDS does
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert all(f"{v} B" in design for v in LDS_BYTES.values() if v)


# ---- the host function

FOLD_SIZES = (1, 511, 512, 513, 6165, (1 << 20) + 53)
FOLD_PIECES = (512, 4096, 1 << 20)


def _piece_sums(block, P):
    """The plain form's sums of the pieces of one block: one walk of `many` over the full pieces as [B // P][P] rows,
    one over the ragged last piece (no `lengths`: at 2^20 positions its per-step select is what takes the time)."""
    full = block.size // P
    sums = CP.many(block[:full * P].reshape(full, P)) if full else np.zeros(0, np.uint32)
    if full * P < block.size:
        sums = np.append(sums, CP.many(block[full * P:]))
    return sums.astype(np.uint32)


@pytest.mark.parametrize("B", FOLD_SIZES)
def test_fold_of_the_plain_piece_sums_is_the_plain_block_sum(psum, B):
    rng = np.random.default_rng(4000 + B)
    block = rng.integers(0, 256, B, dtype=np.uint8)
    whole = int(CP.many(block))
    for P in FOLD_PIECES:
        sums = _piece_sums(block, P)
        assert sums.shape == (-(-B // P),)
        assert psum.fold(sums, P, B) == whole, (B, P)
        assert psum.fold(sums.view(np.int32), P, B) == whole             # as the int32 a device tensor holds
        if sums.size > 1:
            flipped = sums.copy()
            flipped[0] ^= 1
            assert psum.fold(flipped, P, B) != whole
            assert psum.fold(sums[::-1].copy(), P, B) != whole or np.array_equal(sums, sums[::-1])


def test_fold_refusals(ecg, psum):
    L = psum.lib()
    sums = (ctypes.c_uint * 4)(1, 2, 3, 4)
    assert L.ecg_psum_fold(None, 0, 512, 0) == 0                          # an empty block
    for args, word in (((sums, 3, 512, 2048), b"Q = 3"), ((sums, 4, 500, 2000), b"piece_bytes = 500"),
                       ((sums, 4, 256, 1024), b"piece_bytes = 256"), ((sums, 1, 1 << 31, 5), b"piece_bytes"),
                       ((None, 4, 512, 2048), b"NULL"), ((sums, -1, 512, 2048), b"Q = -1"),
                       ((sums, 4, 512, -5), b"B = -5")):
        ecg.lib().ecg_last_error()
        assert L.ecg_psum_fold(*args) == 0
        msg = ecg.lib().ecg_last_error()
        assert msg.startswith(b"psum: ") and word in msg, (args[1:], msg)
    with pytest.raises(ecg.EcgError):
        psum.fold([1, 2, 3], 512, 2048)
    with pytest.raises(ecg.EcgError):
        psum.fold([1], 768, 100)


# ---- arguments (no GPU is touched: every call returns before the first HIP call)

def _refused(ecg, rc, *words):
    assert rc == ecg.ECG_EINVAL
    msg = ecg.lib().ecg_last_error()
    assert msg.startswith(b"psum: ") and len(msg) > 9, msg
    for w in words:
        assert w in msg, (w, msg)


def test_bad_arguments(ecg, psum):
    L = psum.lib()
    ids = (ctypes.c_int * 2)(0, 1)
    dev, out, sel, exp, tg, bad = (ctypes.c_void_p(0x10000 * i) for i in range(1, 7))   # never read
    ok = dict(n=2, ids=ids, base=dev, ss=4096, bs=1024, B=64, P=512, sel=sel, S=1, out=out, exp=exp, tg=tg, bad=bad)
    c0, l0 = psum.counters(), psum.last_launch()

    def pieces_batch(**kw):
        a = dict(ok, **kw)
        return L.ecg_psum_pieces_batch(a["n"], a["ids"], a["base"], a["ss"], a["bs"], a["B"], a["P"], a["sel"],
                                       a["S"], a["out"], None)

    def verify_batch(**kw):
        a = dict(ok, **kw)
        return L.ecg_psum_verify_batch(a["n"], a["ids"], a["base"], a["ss"], a["bs"], a["B"], a["P"], a["sel"],
                                       a["S"], a["exp"], a["out"], a["tg"], a["bad"], None)

    pieces = [(dict(P=p), b"piece_bytes = %d" % p) for p in (0, -512, 1, 256, 511, 513, 768, 1536, 3 << 10, 1 << 31,
                                                              (1 << 30) + 512, 1 << 40)]
    refusals = [(dict(n=0), b"n = 0"), (dict(n=-3), b"n = -3"), (dict(ids=None), b"src_ids"),
                (dict(base=None), b"NULL"), (dict(out=None), b"d_sums"), (dict(B=-1), b"negative"),
                (dict(S=-1), b"negative"), (dict(B=1 << 31), b"2^31"), (dict(B=(1 << 40) + 16), b"2^31"),
                # S_sel * n * Q output words: 2^20 * 2 * 2^10 = 2^31 is refused, one stripe fewer is not (below)
                (dict(S=1 << 20, B=1 << 19), b"output words"), (dict(S=(1 << 31) - 1, B=1), b"output words")] + pieces
    for f in (pieces_batch, verify_batch):
        for kw, word in refusals:
            ecg.lib().ecg_last_error()
            _refused(ecg, f(**kw), word)
        assert f(S=0) == 0 and f(B=0) == 0 and f(S=0, sel=None) == 0        # empty: a no-op
        for good in (512, 1024, 1 << 20, 1 << 30):
            assert f(S=0, P=good) == 0
        _refused(ecg, f(S=0, P=100), b"piece_bytes")                        # refusals come before the no-op
    _refused(ecg, verify_batch(exp=None), b"d_expected")
    _refused(ecg, verify_batch(tg=None), b"d_targets")
    _refused(ecg, verify_batch(bad=None), b"d_bad")
    wide_ids = (ctypes.c_int * 300)(*range(300))
    assert pieces_batch(n=300, ids=wide_ids, S=0) == 0                      # the strided form has no n limit

    code = ecg.ec_factory(0, ecg.CodingParameters(k=6, m=4))
    ptrs = (ctypes.c_void_p * 6)(*[0x10000 + 256 * i for i in range(6)])
    cptrs = (ctypes.c_void_p * 4)(*[0x20000 + 256 * i for i in range(4)])

    def ec_batch(h=code._h, base=dev, B=64, P=512, S=1, v=out):
        return L.ecg_psum_ec_batch(h, base, 4096, 256, B, P, sel, S, v, None)

    def verify_ec_batch(h=code._h, base=dev, B=64, P=512, S=1, v=out, e=exp, t=tg, b=bad):
        return L.ecg_psum_verify_ec_batch(h, base, 4096, 256, B, P, sel, S, e, v, t, b, None)

    def ec(h=code._h, d=ptrs, c=cptrs, B=64, P=512, v=out):
        return L.ecg_psum_ec(h, d, c, B, P, v)

    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_HOST, None)
    _refused(ecg, ec_batch(), b"ECG_MEM_DEVICE")                             # host handles
    _refused(ecg, verify_ec_batch(), b"ECG_MEM_DEVICE")
    _refused(ecg, ec(), b"ECG_MEM_DEVICE")
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, None)
    for f in (ec_batch, verify_ec_batch):
        _refused(ecg, f(h=None), b"handle")
        _refused(ecg, f(base=None), b"NULL")
        _refused(ecg, f(B=-1), b"negative")
        _refused(ecg, f(S=-1), b"negative")
        _refused(ecg, f(B=1 << 31), b"2^31")
        _refused(ecg, f(v=None), b"d_sums")
        _refused(ecg, f(P=768), b"piece_bytes = 768")
        _refused(ecg, f(S=1 << 20, B=1 << 19), b"output words")
        assert f(S=0) == 0 and f(B=0) == 0
    _refused(ecg, verify_ec_batch(e=None), b"d_expected")
    _refused(ecg, verify_ec_batch(t=None), b"d_targets")
    _refused(ecg, verify_ec_batch(b=None), b"d_bad")

    _refused(ecg, ec(h=None), b"handle")
    _refused(ecg, ec(d=None), b"NULL")
    _refused(ecg, ec(c=None), b"NULL")
    _refused(ecg, ec(B=-1), b"negative")
    _refused(ecg, ec(v=None), b"d_sums")
    _refused(ecg, ec(P=100), b"piece_bytes = 100")
    _refused(ecg, ec(P=1 << 31), b"piece_bytes")
    holed = (ctypes.c_void_p * 6)(*[0x10000, 0x10100, None, 0x10300, 0x10400, 0x10500])
    _refused(ecg, ec(d=holed), b"NULL")
    assert ec(B=0) == 0
    wide = ecg.ec_factory(ecg.ECTYPE.RS, ecg.CodingParameters(k=121, m=8))   # n = 129 block pointers
    ecg.lib().ecg_ec_set_memory(wide._h, ecg.ECG_MEM_DEVICE, None)
    wp = (ctypes.c_void_p * 121)(*[0x10000 + 256 * i for i in range(121)])
    wc = (ctypes.c_void_p * 8)(*[0x40000 + 256 * i for i in range(8)])
    _refused(ecg, L.ecg_psum_ec(wide._h, wp, wc, 64, 512, out), b"n = 129")
    assert L.ecg_psum_ec_batch(wide._h, dev, 1 << 20, 256, 64, 512, sel, 0, out, None) == 0   # the strided form takes it

    n = [ctypes.c_longlong(-1), ctypes.c_longlong(-1)]
    assert L.ecg_psum_counters(ctypes.byref(n[0]), ctypes.byref(n[1])) == 0 and n[0].value >= 0 and n[1].value >= 0
    assert L.ecg_psum_counters(None, None) == 0
    assert psum.counters() == c0 and psum.last_launch() == l0

    import torch
    for bad_piece in (0, 100, 768, 1 << 31):                                 # the binding refuses before it allocates
        with pytest.raises(ecg.EcgError) as e:
            psum.pieces(4096, bad_piece)
        assert e.value.code == ecg.ECG_EINVAL
    assert [psum.pieces(B, 512) for B in (0, 1, 512, 513, 1024)] == [0, 1, 1, 2, 2]
    with pytest.raises(ecg.EcgError):
        psum.heal_rows(torch.zeros((2, 3, 1024), dtype=torch.uint8), torch.zeros((2, 3), dtype=torch.int32), 512)


def test_a_grid_past_the_launch_limit_is_refused_before_anything_happens(ecg, psum):
    """2^11 stripes x 256 blocks x 2^13 forced 2 KiB spans of a 16 MiB block is 2^32 workgroups (and 2^19 x 4 output
    words per stripe stay below 2^31): ECG_EHIP with the reason, the counters and the last-launch record unmoved, no
    device touched (the pointers are never read)."""
    L = psum.lib()
    ids = (ctypes.c_int * 256)(*range(256))
    dev, out = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)
    c0, l0 = psum.counters(), psum.last_launch()
    try:
        psum.set_span_bytes(2048)
        rc = L.ecg_psum_pieces_batch(256, ids, dev, 1 << 40, 1 << 30, 1 << 24, 1 << 23, None, 1 << 11, out, None)
        assert rc == ecg.ECG_EHIP, rc
        assert b"launch_psum" in ecg.lib().ecg_last_error()
        psum.set_span_bytes(0)
        # the byte path's grid too (unaligned stride): 2^11 x 256 x 2^30 / 8 KiB = 2^36 workgroups
        rc = L.ecg_psum_pieces_batch(256, ids, dev, 1 << 40, (1 << 30) + 1, 1 << 30, 1 << 30, None, 1 << 11, out, None)
        assert rc == ecg.ECG_EHIP, rc
    finally:
        psum.set_span_bytes(0)
    assert psum.counters() == c0 and psum.last_launch() == l0


def test_set_span_bytes(ecg, psum):
    L = psum.lib()
    try:
        for good in (2048, 4096, 6144, 1 << 20, 0):
            assert L.ecg_psum_set_span_bytes(good) == 0
        for bad in (1, 16, 512, 2047, 2049, 3072, -2048, (1 << 20) + 16, 1 << 31):
            _refused(ecg, L.ecg_psum_set_span_bytes(bad), str(bad).encode())
        with pytest.raises(ecg.EcgError) as e:
            psum.set_span_bytes(100)
        assert e.value.code == ecg.ECG_EINVAL
    finally:
        psum.set_span_bytes(0)
