"""Named-block restoration, the parts that need no GPU: libecg_restore.so's exports and code object, every argument
refusal with its error text (each returns before any device is touched), the scratch size and the fields of the last
launch.  Every test here loads libecg_restore.so.
"""
import ctypes
import json
import os
import re
import subprocess

import pytest

import test_kernel_resources as KR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
K_MAX_R = 8                                                # gf_kernels.hpp kMaxMT
MODE_INLINE, MODE_STRIDED = 0, 2                           # gf_kernels.hpp enum GfMode
OTHERS = ("libecg.so", "libecg_scrub.so", "libecg_locate.so", "libecg_heal.so", "libecg_heal2.so", "libecg_sum.so",
          "libecg_psum.so")


@pytest.fixture(scope="module")
def restore(ecg):
    import ecg_restore
    ecg_restore.lib()
    return ecg_restore


def _golden(name):
    return next(c for c in GOLDEN if c["name"] == name)


# ---- the library

def test_header_symbols_exported(restore):
    hdr = open(os.path.join(ROOT, "include", "ecg_restore.h")).read()
    declared = sorted(set(re.findall(r"\b(ecg_restore_\w+)\s*\(", hdr)))
    assert len(declared) == 8
    assert sorted(restore.EXPORTS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", restore.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r" T (ecg_\w+)", out))) == declared
    assert sorted(restore._SIG) == declared


def test_needs_libecg_only_and_nothing_needs_it(restore):
    lib_dir = os.path.dirname(KR.LIB)
    need = subprocess.run(["readelf", "-d", restore.LIB_PATH], capture_output=True, text=True).stdout
    needed = re.findall(r"NEEDED.*\[(libecg[^\]]*)\]", need)
    assert needed == ["libecg.so"], needed
    for so in OTHERS:
        need = subprocess.run(["readelf", "-d", os.path.join(lib_dir, so)], capture_output=True, text=True).stdout
        assert "NEEDED" in need and "libecg_restore" not in need, so
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(lib_dir, so)], capture_output=True,
                             text=True).stdout
        assert not re.findall(r" T (ecg_restore\w*)", out), so


def test_last_launch_reports_six_fields(restore):
    L = restore.lib()
    assert L.ecg_restore_last_launch(None, 0) == 6
    small = (ctypes.c_int * 5)(*([77] * 5))
    assert L.ecg_restore_last_launch(small, 5) == 6 and list(small) == [77] * 5
    full = (ctypes.c_int * 8)(*([77] * 8))
    assert L.ecg_restore_last_launch(full, 8) == 6 and list(full)[6:] == [77, 77]
    got = restore.last_launch()
    assert list(got) == ["grid_map", "map_group", "cols_per_wg", "wg_per_stripe", "S", "rtiles"]
    assert list(got.values()) == list(full)[:6] and all(v >= 0 for v in got.values())
    hdr = open(os.path.join(ROOT, "include", "ecg_restore.h")).read()
    assert re.findall(r"v\[(\d)\] (\w+)", hdr) == [(str(i), name) for i, name in enumerate(got)]


def test_work_bytes(ecg, restore):
    L = restore.lib()
    assert restore.work_bytes(0) == 0
    sizes = [restore.work_bytes(S) for S in (1, 2, 3, 512, 4096, (1 << 31) - 1)]
    assert all(b > a for a, b in zip([0] + sizes, sizes))               # monotone
    assert sizes[0] % 32 == 0 and sizes[1] == 2 * sizes[0] and sizes[-1] == ((1 << 31) - 1) * sizes[0]
    assert L.ecg_restore_work_bytes(-1) < 0
    with pytest.raises(Exception, match="restore.work_bytes"):
        restore.work_bytes(-1)
    assert b"S_sel = -1" in ecg.lib().ecg_last_error()


@pytest.fixture(scope="module")
def meta(restore):
    """Kernel metadata of libecg_restore.so's gfx950 code object, read as tests/test_kernel_resources.py reads
    libecg.so's."""
    saved = KR.LIB
    KR.LIB = restore.LIB_PATH
    try:
        return KR._metadata()
    finally:
        KR.LIB = saved


def test_code_object_is_the_restore_family(meta):
    keys, rest = [], []
    for s in meta:
        v = re.search(r"gf_restore_kernelILi(\d+)ELi(\d+)EE", s)
        b = re.search(r"gf_restore_byte_kernelILi(\d+)ELi(\d+)EE", s)
        if v:
            keys.append(("vec",) + tuple(map(int, v.groups())))
        elif b:
            keys.append(("byte",) + tuple(map(int, b.groups())))
        else:
            rest.append(s)
    assert len(rest) == 2 and [s for s in rest if "gf_restore_plan_kernel" in s] and \
        [s for s in rest if "gf_restore_names_kernel" in s], rest
    want = {(kind, r, mode) for kind in ("vec", "byte") for r in range(1, K_MAX_R + 1)
            for mode in (MODE_INLINE, MODE_STRIDED)}
    assert len(keys) == len(set(keys)) == 32
    assert set(keys) == want
    for name in ("gf_vec_kernel", "gf_byte_kernel", "gf_lat_dword_kernel", "gf_scrub", "gf_locate", "gf_heal"):
        assert not [s for s in meta if name in s], name


def test_restore_kernels_use_no_scratch_no_lds(meta):
    bad = {n: f for n, f in meta.items() if f.get("private_segment_fixed_size", 0) or f.get("vgpr_spill_count", 0)}
    assert not bad, list(bad)[:5]
    # the counters are three statically indexed registers per lane, the plan kernel's matrices packed words: no LDS
    assert all(f.get("group_segment_fixed_size", 0) == 0 for f in meta.values())
    # the descriptor, the INLINE plan included, fits the kernel arguments
    assert all(f["kernarg_segment_size"] <= 4096 for f in meta.values())
    # four waves per SIMD at the least (512 VGPRs / 4), as the heal
    assert max(f["vgpr_count"] for f in meta.values()) <= 128


# ---- arguments (no GPU is touched: every call returns before the first HIP call)

def _err(ecg):
    return ecg.lib().ecg_last_error()


def test_bad_arguments(ecg, restore):
    L, EINVAL = restore.lib(), ecg.ECG_EINVAL
    H = (ctypes.c_int * 4)(1, 1, 1, 2)
    ids = (ctypes.c_int * 2)(0, 1)
    dev, rep, sel, nm, wk = (ctypes.c_void_p(0x10000 * i) for i in (1, 2, 3, 4, 5))   # never read
    ok = dict(n=2, r=2, H=H, ids=ids, base=dev, ss=4096, bs=1024, B=64, sel=sel, nm=nm, S=1, wk=wk, rep=rep)

    def matrix_batch(**kw):
        a = dict(ok, **kw)
        return L.ecg_restore_matrix_batch(a["n"], a["r"], a["H"], a["ids"], a["base"], a["ss"], a["bs"], a["B"],
                                          a["sel"], a["nm"], a["S"], a["wk"], a["rep"], None)

    for kw, text in ((dict(n=0), b"n = 0"), (dict(r=0), b"r = 0"), (dict(n=-3), b"n = -3"), (dict(r=-1), b"r = -1"),
                     (dict(H=None), b"H is NULL"), (dict(ids=None), b"src_ids is NULL"),
                     (dict(base=None), b"base is NULL"), (dict(rep=None), b"d_report is NULL"),
                     (dict(B=-1), b"B = -1"), (dict(S=-1), b"S_sel = -1"), (dict(B=1 << 31), b"not below 2^31"),
                     (dict(B=(1 << 40) + 16), b"not below 2^31"), (dict(nm=None), b"d_named is NULL"),
                     (dict(wk=None), b"d_work is NULL"), (dict(wk=ctypes.c_void_p(0x50010)), b"32-byte aligned")):
        assert matrix_batch(**kw) == EINVAL, kw
        assert _err(ecg).startswith(b"restore: ") and text in _err(ecg), (kw, _err(ecg))
    assert matrix_batch(S=0) == 0 and matrix_batch(B=0) == 0 and matrix_batch(S=0, sel=None) == 0   # empty: a no-op
    assert matrix_batch(S=0, wk=None) == 0                               # no stripes need no scratch
    wide = (ctypes.c_int * (9 * 129))(*([1] * (9 * 129)))
    wide_ids = (ctypes.c_int * 129)(*range(129))
    assert matrix_batch(r=9, n=12, H=wide, ids=wide_ids) == EINVAL      # r > 8
    assert b"restore: r = 9" in _err(ecg)
    assert matrix_batch(r=2, n=129, H=wide, ids=wide_ids) == EINVAL     # n > 128
    assert b"n = 129" in _err(ecg)
    assert matrix_batch(r=8, n=128, H=wide, ids=wide_ids, S=0) == 0     # the largest shape is accepted

    M = (ctypes.c_int * (9 * 127))(*([1] * (9 * 127)))

    def encode_batch(k=2, m=1, matrix=M, base=dev, B=64, S=1, v=rep, ids=sel, f=nm, w=wk):
        return L.ecg_restore_encode_batch(k, m, matrix, base, 4096, 1024, B, ids, f, S, w, v, None)

    for kw, text in ((dict(k=0), b"k = 0"), (dict(m=0), b"m = 0"), (dict(matrix=None), b"matrix is NULL"),
                     (dict(base=None), b"base is NULL"), (dict(v=None), b"d_report is NULL"), (dict(B=-1), b"B = -1"),
                     (dict(S=-1), b"S_sel = -1"), (dict(B=1 << 31), b"2^31"), (dict(m=9), b"r = 9"),
                     (dict(k=127, m=2), b"n = 129"), (dict(k=1 << 30, m=8), b"exceeds"), (dict(f=None), b"d_named"),
                     (dict(w=None), b"d_work")):
        assert encode_batch(**kw) == EINVAL, kw
        assert text in _err(ecg), (kw, _err(ecg))
    assert encode_batch(S=0) == 0 and encode_batch(B=0) == 0 and encode_batch(S=0, ids=None) == 0
    assert encode_batch(k=120, m=8, S=0) == 0

    code = ecg.ec_factory(0, ecg.CodingParameters(k=6, m=4))
    flags = (ctypes.c_ubyte * 10)(0, 1, 0, 0, 0, 0, 0, 1, 0, 0)
    assert L.ecg_restore_ec_batch(None, dev, 4096, 256, 64, sel, nm, 1, wk, rep, None) == EINVAL
    assert b"ec is NULL" in _err(ecg)
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_HOST, None)
    assert L.ecg_restore_ec_batch(code._h, dev, 4096, 256, 64, sel, nm, 1, wk, rep, None) == EINVAL   # host handle
    assert b"ECG_MEM_DEVICE" in _err(ecg)
    ptrs = (ctypes.c_void_p * 6)(*[0x10000 + 256 * i for i in range(6)])
    cptrs = (ctypes.c_void_p * 4)(*[0x20000 + 256 * i for i in range(4)])
    assert L.ecg_restore_ec(code._h, ptrs, cptrs, 64, flags, rep) == EINVAL                            # host handle
    assert b"ECG_MEM_DEVICE" in _err(ecg)
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, None)
    for args, text in (((None, 4096, 256, 64, sel, nm, 1, wk, rep), b"base is NULL"),
                       ((dev, 4096, 256, -1, sel, nm, 1, wk, rep), b"B = -1"),
                       ((dev, 4096, 256, 64, sel, nm, -1, wk, rep), b"S_sel = -1"),
                       ((dev, 4096, 256, 1 << 31, sel, nm, 1, wk, rep), b"2^31"),
                       ((dev, 4096, 256, 64, sel, None, 1, wk, rep), b"d_named"),
                       ((dev, 4096, 256, 64, sel, nm, 1, None, rep), b"d_work"),
                       ((dev, 4096, 256, 64, sel, nm, 1, wk, None), b"d_report")):
        assert L.ecg_restore_ec_batch(code._h, *args, None) == EINVAL, args
        assert text in _err(ecg), (args, _err(ecg))
    assert L.ecg_restore_ec_batch(code._h, dev, 4096, 256, 64, None, nm, 0, wk, rep, None) == 0
    assert L.ecg_restore_ec_batch(code._h, dev, 4096, 256, 0, sel, nm, 3, wk, rep, None) == 0
    holed = (ctypes.c_void_p * 6)(*[0x10000, 0x10100, None, 0x10300, 0x10400, 0x10500])
    for args, text in (((None, cptrs, 64, flags, rep), b"pointer array is NULL"),
                       ((ptrs, None, 64, flags, rep), b"pointer array is NULL"),
                       ((ptrs, cptrs, -1, flags, rep), b"block_size = -1"),
                       ((ptrs, cptrs, 64, None, rep), b"h_named is NULL"),
                       ((ptrs, cptrs, 64, flags, None), b"d_report is NULL"),
                       ((holed, cptrs, 64, flags, rep), b"a block pointer is NULL")):
        assert L.ecg_restore_ec(code._h, *args) == EINVAL, args
        assert text in _err(ecg), (args, _err(ecg))
    assert L.ecg_restore_ec(None, ptrs, cptrs, 64, flags, rep) == EINVAL
    assert L.ecg_restore_ec(code._h, ptrs, cptrs, 0, flags, rep) == 0

    sums, exp, named, count = (ctypes.c_void_p(0x10000 * i) for i in (6, 7, 8, 9))
    for args, text in (((0, 1, sums, exp, 1, named, count), b"n = 0"), ((2, -1, sums, exp, 1, named, count), b"Q = -1"),
                       ((2, 1, sums, exp, -1, named, count), b"S_sel = -1"),
                       ((2, 1, None, exp, 1, named, count), b"d_sums is NULL"),
                       ((2, 1, sums, None, 1, named, count), b"d_expected is NULL"),
                       ((2, 1, sums, exp, 1, None, count), b"d_named is NULL"),
                       ((2, 1, sums, exp, 1, named, None), b"d_count is NULL")):
        assert L.ecg_restore_names_from_sums(*args, None) == EINVAL, args
        assert text in _err(ecg), (args, _err(ecg))
    assert L.ecg_restore_names_from_sums(2, 0, sums, exp, 1, named, count, None) == 0
    assert L.ecg_restore_names_from_sums(2, 4, sums, exp, 0, named, count, None) == 0

    n = [ctypes.c_longlong(-1), ctypes.c_longlong(-1)]
    assert L.ecg_restore_counters(ctypes.byref(n[0]), ctypes.byref(n[1])) == 0 and n[0].value >= 0 and n[1].value >= 0
    assert L.ecg_restore_counters(None, None) == 0
    assert restore.counters() == {"launches": n[0].value, "bytes": n[1].value}


@pytest.mark.parametrize("name", ["PC(4,2,2,1)", "HPC(4,2,2,1|2,1)", "PC(4,1,4,1)"])
def test_product_codes_with_more_than_eight_checks_are_refused(ecg, restore, name):
    c = _golden(name)
    code = ecg.ec_factory(c["type"], ecg.CodingParameters(**c["params"]))
    assert code.m > K_MAX_R
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, None)
    dev, rep, nm, wk = (ctypes.c_void_p(0x10000 * i) for i in (1, 2, 3, 4))
    L = restore.lib()
    assert L.ecg_restore_ec_batch(code._h, dev, 1 << 20, 4096, 64, None, nm, 1, wk, rep, None) == ecg.ECG_EINVAL
    assert f"restore: r = {code.m}".encode() in _err(ecg)
    ptrs = (ctypes.c_void_p * code.k)(*[0x10000 + 256 * i for i in range(code.k)])
    cptrs = (ctypes.c_void_p * code.m)(*[0x20000 + 256 * i for i in range(code.m)])
    flags = (ctypes.c_ubyte * (code.k + code.m))()
    assert L.ecg_restore_ec(code._h, ptrs, cptrs, 64, flags, rep) == ecg.ECG_EINVAL
