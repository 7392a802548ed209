"""In-place correction, the parts that need no GPU: libecg_heal.so's exports and code object, and every argument
refusal -- among them ANY mode over a check with two proportional columns, which is refused before any device is
touched, while TARGET mode over the same check is accepted.
"""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import locate_plain as LP
import test_kernel_resources as KR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
K_MAX_R = 8                                                # gf_kernels.hpp kMaxMT
MODE_INLINE, MODE_STRIDED = 0, 2                           # gf_kernels.hpp enum GfMode


@pytest.fixture(scope="module")
def heal(ecg):
    import ecg_heal
    ecg_heal.lib()
    return ecg_heal


def _golden(name):
    return next(c for c in GOLDEN if c["name"] == name)


# ---- the library

def test_header_symbols_exported(heal):
    hdr = open(os.path.join(ROOT, "include", "ecg_heal.h")).read()
    declared = sorted(set(re.findall(r"\b(ecg_heal_\w+)\s*\(", hdr)))
    assert len(declared) == 6
    assert sorted(heal.EXPORTS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", heal.LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r" T (ecg_\w+)", out)))
    assert exported == declared
    assert "ecg_locate_verdict" in hdr                    # a report is read by the locate's verdict, unchanged
    # the other three libraries need nothing from this one, and it needs only libecg.so
    lib_dir = os.path.dirname(KR.LIB)
    for so in (KR.LIB, os.path.join(lib_dir, "libecg_scrub.so"), os.path.join(lib_dir, "libecg_locate.so")):
        need = subprocess.run(["readelf", "-d", so], capture_output=True, text=True).stdout
        assert "NEEDED" in need and "libecg_heal" not in need, so
    need = subprocess.run(["readelf", "-d", heal.LIB_PATH], capture_output=True, text=True).stdout
    assert "libecg.so" in need and "libecg_scrub" not in need and "libecg_locate" not in need


def test_the_other_libraries_keep_their_symbol_sets(heal):
    lib_dir = os.path.dirname(KR.LIB)
    for name, header in (("libecg_scrub.so", "ecg_scrub.h"), ("libecg_locate.so", "ecg_locate.h")):
        prefix = header[:-2]
        hdr = open(os.path.join(ROOT, "include", header)).read()
        declared = sorted(set(re.findall(rf"\b({prefix}_\w+)\s*\(", hdr)))
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(lib_dir, name)], capture_output=True,
                             text=True).stdout
        assert sorted(set(re.findall(r" T (ecg_\w+)", out))) == declared, name
    out = subprocess.run(["nm", "-D", "--defined-only", KR.LIB], capture_output=True, text=True).stdout
    assert not re.findall(r" T (ecg_heal\w*)", out)


def test_last_launch_reports_six_fields(heal):
    L = heal.lib()
    assert L.ecg_heal_last_launch(None, 0) == 6
    small = (ctypes.c_int * 5)(*([77] * 5))
    assert L.ecg_heal_last_launch(small, 5) == 6 and list(small) == [77] * 5
    full = (ctypes.c_int * 8)(*([77] * 8))
    assert L.ecg_heal_last_launch(full, 8) == 6 and list(full)[6:] == [77, 77]
    got = heal.last_launch()
    assert list(got) == ["grid_map", "map_group", "cols_per_wg", "wg_per_stripe", "S", "rtiles"]
    assert list(got.values()) == list(full)[:6] and all(v >= 0 for v in got.values())
    hdr = open(os.path.join(ROOT, "include", "ecg_heal.h")).read()
    assert re.findall(r"v\[(\d)\] (\w+)", hdr) == [(str(i), name) for i, name in enumerate(got)]


@pytest.fixture(scope="module")
def meta(heal):
    """Kernel metadata of libecg_heal.so's gfx950 code object, read as tests/test_kernel_resources.py reads
    libecg.so's."""
    saved = KR.LIB
    KR.LIB = heal.LIB_PATH
    try:
        return KR._metadata()
    finally:
        KR.LIB = saved


def test_code_object_is_the_heal_family(meta):
    keys, rest = [], []
    for s in meta:
        v = re.search(r"gf_heal_kernelILi(\d+)ELi(\d+)EE", s)
        b = re.search(r"gf_heal_byte_kernelILi(\d+)ELi(\d+)EE", s)
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
    for name in ("gf_vec_kernel", "gf_byte_kernel", "gf_lat_dword_kernel", "gf_scrub", "gf_locate"):
        assert not [s for s in meta if name in s], name


def test_heal_kernels_do_not_spill(meta):
    bad = {n: f for n, f in meta.items() if f.get("private_segment_fixed_size", 0) or f.get("vgpr_spill_count", 0)}
    assert not bad, list(bad)[:5]
    # the counters are three statically indexed registers per lane, not LDS
    assert all(f.get("group_segment_fixed_size", 0) == 0 for f in meta.values())


# ---- arguments (no GPU is touched: every call returns before the first HIP call)

# two proportional columns (column 2 = 3 * column 0 over GF(2^8)), no zero column
H_PROP = np.array([[1, 1, 3, 1], [2, 3, 6, 0]], dtype=np.int64)


def test_hand_made_check_has_two_proportional_columns():
    assert LP.proportional_pairs(H_PROP) == (1, 0)
    assert LP.proportional_pairs(H_PROP[:, [0, 1, 3]]) == (0, 0)


def test_bad_arguments(ecg, heal):
    L, EINVAL = heal.lib(), ecg.ECG_EINVAL
    H = (ctypes.c_int * 4)(1, 1, 1, 2)                                  # columns (1, 1), (1, 2): not proportional
    ids = (ctypes.c_int * 2)(0, 1)
    dev, rep, sel, tg = (ctypes.c_void_p(0x10000 * i) for i in (1, 2, 3, 4))   # never read
    ok = dict(n=2, r=2, H=H, ids=ids, base=dev, ss=4096, bs=1024, B=64, sel=sel, tg=tg, S=1, rep=rep)

    def matrix_batch(**kw):
        a = dict(ok, **kw)
        return L.ecg_heal_matrix_batch(a["n"], a["r"], a["H"], a["ids"], a["base"], a["ss"], a["bs"], a["B"],
                                       a["sel"], a["tg"], a["S"], a["rep"], None)

    for kw in (dict(n=0), dict(r=0), dict(H=None), dict(ids=None), dict(base=None), dict(rep=None), dict(B=-1),
               dict(S=-1), dict(B=1 << 31), dict(B=(1 << 40) + 16), dict(n=-3), dict(r=-1)):
        assert matrix_batch(**kw) == EINVAL, kw
        assert matrix_batch(tg=None, **kw) == EINVAL, kw
    for tgt in (tg, None):                                             # empty: a no-op, in both modes
        assert matrix_batch(S=0, tg=tgt) == 0 and matrix_batch(B=0, tg=tgt) == 0
        assert matrix_batch(S=0, sel=None, tg=tgt) == 0                # a NULL selection is the identity
    wide = (ctypes.c_int * (9 * 129))(*([1] * (9 * 129)))
    wide_ids = (ctypes.c_int * 129)(*range(129))
    assert matrix_batch(r=9, n=12, H=wide, ids=wide_ids) == EINVAL      # r > 8
    assert b"r = 9" in ecg.lib().ecg_last_error()
    assert matrix_batch(r=2, n=129, H=wide, ids=wide_ids) == EINVAL     # n > 128
    assert b"n = 129" in ecg.lib().ecg_last_error()
    assert matrix_batch(r=8, n=128, H=wide, ids=wide_ids, S=0) == 0     # the largest shape is accepted (TARGET)

    M = (ctypes.c_int * (9 * 127))(*([1] * (9 * 127)))

    def encode_batch(k=2, m=1, matrix=M, base=dev, B=64, S=1, v=rep, ids=sel, t=tg):
        return L.ecg_heal_encode_batch(k, m, matrix, base, 4096, 1024, B, ids, t, S, v, None)

    for kw in (dict(k=0), dict(m=0), dict(matrix=None), dict(base=None), dict(v=None), dict(B=-1), dict(S=-1),
               dict(B=1 << 31), dict(m=9), dict(k=127, m=2), dict(k=1 << 30, m=8)):
        assert encode_batch(**kw) == EINVAL, kw
    assert encode_batch(S=0) == 0 and encode_batch(B=0) == 0 and encode_batch(S=0, ids=None) == 0
    assert encode_batch(k=120, m=8, S=0) == 0

    code = ecg.ec_factory(0, ecg.CodingParameters(k=6, m=4))
    assert L.ecg_heal_ec_batch(None, dev, 4096, 256, 64, sel, tg, 1, rep, None) == EINVAL
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_HOST, None)
    assert L.ecg_heal_ec_batch(code._h, dev, 4096, 256, 64, sel, tg, 1, rep, None) == EINVAL      # host handle
    ptrs = (ctypes.c_void_p * 6)(*[0x10000 + 256 * i for i in range(6)])
    cptrs = (ctypes.c_void_p * 4)(*[0x20000 + 256 * i for i in range(4)])
    assert L.ecg_heal_ec(code._h, ptrs, cptrs, 64, 3, rep) == EINVAL                              # host handle
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, None)
    for args in ((None, 4096, 256, 64, sel, tg, 1, rep), (dev, 4096, 256, -1, sel, tg, 1, rep),
                 (dev, 4096, 256, 64, sel, tg, -1, rep), (dev, 4096, 256, 1 << 31, sel, tg, 1, rep),
                 (dev, 4096, 256, 64, sel, tg, 1, None)):
        assert L.ecg_heal_ec_batch(code._h, *args, None) == EINVAL, args
    for tgt in (tg, None):
        assert L.ecg_heal_ec_batch(code._h, dev, 4096, 256, 64, None, tgt, 0, rep, None) == 0
        assert L.ecg_heal_ec_batch(code._h, dev, 4096, 256, 0, sel, tgt, 3, rep, None) == 0
    assert L.ecg_heal_ec(code._h, None, cptrs, 64, 3, rep) == EINVAL
    assert L.ecg_heal_ec(code._h, ptrs, None, 64, 3, rep) == EINVAL
    assert L.ecg_heal_ec(code._h, ptrs, cptrs, -1, 3, rep) == EINVAL
    assert L.ecg_heal_ec(code._h, ptrs, cptrs, 64, 3, None) == EINVAL
    assert L.ecg_heal_ec(code._h, ptrs, cptrs, 64, 10, rep) == EINVAL                             # target == n
    assert L.ecg_heal_ec(code._h, ptrs, cptrs, 64, -2, rep) == EINVAL
    for target in (-1, 0, 9):
        assert L.ecg_heal_ec(code._h, ptrs, cptrs, 0, target, rep) == 0
    holed = (ctypes.c_void_p * 6)(*[0x10000, 0x10100, None, 0x10300, 0x10400, 0x10500])
    assert L.ecg_heal_ec(code._h, holed, cptrs, 64, 3, rep) == EINVAL

    n = [ctypes.c_longlong(-1), ctypes.c_longlong(-1)]
    assert L.ecg_heal_counters(ctypes.byref(n[0]), ctypes.byref(n[1])) == 0 and n[0].value >= 0 and n[1].value >= 0
    assert L.ecg_heal_counters(None, None) == 0


def test_any_mode_is_refused_over_proportional_columns(ecg, heal):
    """ANY over RS(8,1) (r = 1: every pair of columns) and over a hand-made H with one proportional pair: ECG_EINVAL
    with the reason, from every entry point, whatever S_sel; TARGET over the same checks is accepted (S_sel = 0: no
    device is touched)."""
    L, EINVAL = heal.lib(), ecg.ECG_EINVAL
    dev, rep, sel, tg = (ctypes.c_void_p(0x10000 * i) for i in (1, 2, 3, 4))
    l0 = heal.counters()["launches"]

    def matrix_batch(H, targets, S):
        H = np.asarray(H, dtype=np.int64)
        r, n = H.shape
        flat = (ctypes.c_int * (r * n))(*[int(v) for v in H.reshape(-1)])
        ids = (ctypes.c_int * n)(*range(n))
        return L.ecg_heal_matrix_batch(n, r, flat, ids, dev, 1 << 16, 1024, 64, sel, targets, S, rep, None)

    for S in (1, 0):
        assert matrix_batch(H_PROP, None, S) == EINVAL
        msg = ecg.lib().ecg_last_error()
        assert b"columns 0 and 2" in msg and b"proportional" in msg, msg
    assert matrix_batch(H_PROP, tg, 0) == 0                              # TARGET takes it
    assert matrix_batch(H_PROP[:, [0, 1, 3]], None, 0) == 0              # and ANY without the pair
    assert matrix_batch(H_PROP[:, ::-1], None, 1) == EINVAL and b"columns 1 and 3" in ecg.lib().ecg_last_error()
    Hz = H_PROP.copy()
    Hz[:, 2] = 0                                                         # a zero column is proportional to nothing
    assert matrix_batch(Hz, None, 0) == 0
    Hz[:, 0] = 0                                                         # nor are two of them
    assert matrix_batch(Hz, None, 0) == 0
    assert matrix_batch([[1, 2, 3]], None, 1) == EINVAL                  # r = 1, n >= 2
    assert matrix_batch([[1, 2, 3]], tg, 0) == 0
    assert matrix_batch([[7]], None, 0) == 0                             # r = 1, n = 1: nothing to confuse

    c = _golden("RS(8,1)")
    M = (ctypes.c_int * 8)(*[int(v) for v in c["matrix"]])
    assert L.ecg_heal_encode_batch(8, 1, M, dev, 1 << 16, 1024, 64, sel, None, 1, rep, None) == EINVAL
    assert b"proportional" in ecg.lib().ecg_last_error() and b"r = 1" in ecg.lib().ecg_last_error()
    assert L.ecg_heal_encode_batch(8, 1, M, dev, 1 << 16, 1024, 64, sel, tg, 0, rep, None) == 0
    code = ecg.ec_factory(c["type"], ecg.CodingParameters(**c["params"]))
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, None)
    assert L.ecg_heal_ec_batch(code._h, dev, 1 << 16, 1024, 64, sel, None, 1, rep, None) == EINVAL
    assert L.ecg_heal_ec_batch(code._h, dev, 1 << 16, 1024, 64, sel, tg, 0, rep, None) == 0
    ptrs = (ctypes.c_void_p * 8)(*[0x10000 + 256 * i for i in range(8)])
    cptrs = (ctypes.c_void_p * 1)(0x20000)
    assert L.ecg_heal_ec(code._h, ptrs, cptrs, 64, -1, rep) == EINVAL
    assert b"proportional" in ecg.lib().ecg_last_error()
    assert L.ecg_heal_ec(code._h, ptrs, cptrs, 0, 4, rep) == 0
    assert heal.counters()["launches"] == l0


@pytest.mark.parametrize("c", [c for c in GOLDEN if "matrix" in c and c["m"] >= 2],
                         ids=[c["name"] for c in GOLDEN if "matrix" in c and c["m"] >= 2])
def test_any_mode_is_accepted_for_the_golden_checks(ecg, heal, c):
    """tests/test_locate_host.py's census finds no proportional columns among the RS / ERS / LRC checks with r >= 2."""
    code = ecg.ec_factory(c["type"], ecg.CodingParameters(**c["params"]))
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, None)
    dev, rep = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)
    assert heal.lib().ecg_heal_ec_batch(code._h, dev, 1 << 20, 4096, 64, None, None, 0, rep, None) == 0


@pytest.mark.parametrize("name", ["PC(4,2,2,1)", "HPC(4,2,2,1|2,1)", "PC(4,1,4,1)"])
def test_product_codes_with_more_than_eight_checks_are_refused(ecg, heal, name):
    c = _golden(name)
    code = ecg.ec_factory(c["type"], ecg.CodingParameters(**c["params"]))
    assert code.m > K_MAX_R
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, None)
    dev, rep, tg = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000)
    assert heal.lib().ecg_heal_ec_batch(code._h, dev, 1 << 20, 4096, 64, None, tg, 1, rep, None) == ecg.ECG_EINVAL
    assert f"r = {code.m}".encode() in ecg.lib().ecg_last_error()
    ptrs = (ctypes.c_void_p * code.k)(*[0x10000 + 256 * i for i in range(code.k)])
    cptrs = (ctypes.c_void_p * code.m)(*[0x20000 + 256 * i for i in range(code.m)])
    assert heal.lib().ecg_heal_ec(code._h, ptrs, cptrs, 64, 0, rep) == ecg.ECG_EINVAL
