"""The region-product kernel instantiations libecg.so is built with, and the sweep that launches each of them
(helper of tests/test_kernel_enumeration.py and tests/test_gpu_kernel_matrix.py; imports nothing of the project).

A KEY names one instantiation, in the form ecg.launch_histogram() reports:
    ("vec", MODE, BIN, NT, MT)        gf_vec_kernel<MT, MODE, NT, BIN>
    ("byte", MODE, BIN, MT)           gf_byte_kernel<MT, MODE, BIN>
    ("lat", BIN, MT, KB, EAGER)       gf_lat_dword_kernel<MT, BIN, KB, EAGER>
A CASE is one public call, its shape, and the keys its launches must land on, predicted here from the
dispatcher's rules (engine.cpp launch_one / run_strided / run_ptr_batch, gf_kernels.hip launch_gf) and checked
against the histogram when the case runs.
"""
from collections import namedtuple

import numpy as np

# ---- the dispatcher's constants, mirrored (source: erasure-codes-prototype_amd/csrc/)
MODE_INLINE, MODE_PTRS, MODE_STRIDED, MODE_INLINE_LAT = 0, 1, 2, 3  # gf_kernels.hpp:28-35 enum GfMode
K_MAX_MT = 8                      # gf_kernels.hpp:39 kMaxMT: rows per GENERAL row tile
K_MAX_MT_BIN = 16                 # gf_kernels.hpp:40 kMaxMTBin: rows per BINARY row tile
LAT_BUCKETS = (4, 6, 8, 10, 12, 16)  # gf_kernels.hip pick_lat_k: input-count buckets of the latency kernel
LAT_MAX_SRC = 16                  # gf_kernels.hpp:46 kLatMaxSrc
LAT_EAGER_BYTES = 16 << 10        # gf_kernels.hpp:47 kLatEagerBytes: EAGER form up to this block size
NT_POLICIES = (0, 1, 2, 3)        # gf_kernels.hip pick_vec: switch (nt & 3)
WIDE_BIN_NT = 3                   # gf_kernels.hip gen_pick: `if constexpr (BIN && NT == 3)` builds MT 9..16;
                                  # launch_gf: `nt = a.MT > kMaxMT ? 3 : ...`
BYTE_MODES = (MODE_INLINE, MODE_PTRS, MODE_STRIDED)  # gf_kernels.hip launch_gf: INLINE_LAT tails run pick_byte<INLINE>
LAT_DWORD_DEFAULT = 1 << 20       # gf_host.cpp init_options: ECG_OPT_LAT_DWORD_BYTES
# kernels of the code object outside the enumeration
OTHER_KERNELS = ("gf_call_worker_kernel", "fill_splitmix_kernel")


def enumeration():
    """Every key the library is built with, from the constants above."""
    keys = set()
    for b in (0, 1):
        for mt in range(1, (K_MAX_MT_BIN if b else K_MAX_MT) + 1):
            for mode in (MODE_INLINE, MODE_PTRS, MODE_STRIDED, MODE_INLINE_LAT):
                for nt in NT_POLICIES if mt <= K_MAX_MT else (WIDE_BIN_NT,):
                    keys.add(("vec", mode, b, nt, mt))
            for mode in BYTE_MODES:
                keys.add(("byte", mode, b, mt))
            if mt <= K_MAX_MT:  # launch_gf: the latency kernel takes one row tile of at most kMaxMT rows
                for kb in LAT_BUCKETS:
                    for eager in (0, 1):
                        keys.add(("lat", b, mt, kb, eager))
    return keys


# ---- cases
# form: "strided" ecg.matrix_apply_batch over S = 3 stripes; "ptrs" three scattered ecg.dev_matrix_encode calls in
# one ecg.batch() scope; "dev" one ecg.dev_matrix_encode; "host" one ecg.jerasure_matrix_encode on numpy blocks.
# lat: the ECG_OPT_LAT_DWORD_BYTES the case sets; nt / cpw: ECG_OPT_NT / ECG_OPT_COLS_PER_WG; shift: bytes the
# arenas' bases are moved off 16-byte alignment.
Case = namedtuple("Case", "form binary m k B nt cpw lat shift seed")
S_STRIDED = 3


def tile(binary, m):
    mt = min(m, K_MAX_MT_BIN if binary else K_MAX_MT)  # program_cache.cpp program_set: ps->MT, ps->rtiles
    return mt, (m + mt - 1) // mt


def lat_bucket(k):
    return next(kb for kb in LAT_BUCKETS if k <= kb)


def matrix(c):
    """The case's coefficient matrix [m][k].  GENERAL: seeded random bytes with a value >= 2, then a 1, then a 0
    forced in as far as the size allows, and no all-zero row (ecg_dev_matrix_encode drops such rows, as Jerasure
    leaves their blocks alone).  BINARY: dense seeded 0/1 (three ones in four) with no empty row or column, so
    ECG_OPT_ROW_SPLIT -- which needs every column used by exactly one row -- cannot split it."""
    rng = np.random.default_rng(c.seed)
    if c.binary:
        M = (rng.random((c.m, c.k)) < 0.75).astype(np.int64)
        for p in range(c.m):
            if not M[p].any():
                M[p, p % c.k] = 1
        for j in range(c.k):
            if not M[:, j].any():
                M[j % c.m, j] = 1
        if c.k >= 16 and c.m >= 2:  # a column used twice: never separable
            M[0, 0] = M[1, 0] = 1
        return M
    M = rng.integers(0, 256, (c.m, c.k), dtype=np.int64)
    flat = M.reshape(-1)
    flat[0] = 2 + int(flat[0]) % 254
    if flat.size >= 2:
        flat[-1] = 1
    if c.k >= 3:
        M[0, 1] = 0
    for p in range(c.m):
        if not M[p].any():
            M[p, 0] = 7
    return M


def live_rows(c, M):
    """Rows the call writes: the pointer-call forms drop all-zero rows (matrix.cpp plan_matrix_encode)."""
    if c.form == "strided":
        return list(range(c.m))
    return [p for p in range(c.m) if M[p].any()]


def _route(c, M):
    """(binary, mt, rtiles, vec_bytes, mode, lat) of the case's launch_gf call, by the dispatcher's rules; lat: the
    call runs the latency kernel."""
    M = matrix(c) if M is None else M
    rows = live_rows(c, M)
    binary = int(all(int(v) <= 1 for p in rows for v in M[p]))  # matrix.cpp op_is_binary
    mt, rtiles = tile(binary, len(rows))
    aligned = c.shift % 16 == 0 or c.form == "host"  # host blocks are staged at a 256-byte pitch (run_host)
    vec_bytes = (c.B & ~15) if aligned else 0
    if c.form == "strided":
        mode = MODE_STRIDED
    elif c.form == "ptrs":
        mode = MODE_PTRS
    elif c.form == "host":
        mode = MODE_INLINE_LAT  # host_tier.cpp run_host: launch_one(..., latency = true)
    else:  # engine.cpp launch_one: lat = B <= ECG_OPT_LAT_DWORD_BYTES && k <= kLatMaxSrc
        mode = MODE_INLINE_LAT if c.B <= c.lat and c.k <= LAT_MAX_SRC else MODE_INLINE
    lat = (mode == MODE_INLINE_LAT and vec_bytes == c.B and c.B <= c.lat and c.k <= LAT_MAX_SRC and rtiles == 1 and
           mt <= K_MAX_MT)  # gf_kernels.hip launch_gf
    return binary, mt, rtiles, vec_bytes, mode, lat


def expected_keys(c, M=None):
    """{key: launches} of the case, by the dispatcher's rules."""
    binary, mt, rtiles, vec_bytes, mode, lat = _route(c, M)
    keys = {}
    if lat:
        keys[("lat", binary, mt, lat_bucket(c.k), int(c.B <= LAT_EAGER_BYTES))] = 1
        return keys
    if vec_bytes > 0:
        keys[("vec", mode, binary, WIDE_BIN_NT if mt > K_MAX_MT else c.nt, mt)] = 1
    if vec_bytes < c.B:
        keys[("byte", MODE_INLINE if mode == MODE_INLINE_LAT else mode, binary, mt)] = 1
    return keys


def expected_report(c, M=None):
    """{mode, rtiles, kernel} of ecg.last_launch() after the case's call (include/ecg.h ecg_last_launch): the mode
    the call was launched in (an INLINE_LAT call's byte kernel still reports mode 3), its row tiles, and kernel 2 for
    the latency kernel, 0 when a vector launch ran, 1 for the byte kernel alone."""
    _, _, rtiles, vec_bytes, mode, lat = _route(c, M)
    return {"mode": mode, "rtiles": rtiles, "kernel": 2 if lat else 0 if vec_bytes > 0 else 1}


B_MAIN = 4693   # two full 2 KiB workgroup chunks, a partial third of 37 columns, a 5-byte tail
B_BYTES = 5     # a byte-only block
B_LAT_EAGER, B_LAT_PLAIN = 1040, 16400  # EAGER with a partial last workgroup; non-eager
K_LB4 = (1, 2, 3, 4, 7, 9)   # load-batch 4 tiles: BINARY, GENERAL MT <= 4 (gf_kernels.hip kLoadBatch, kGenLB)
K_LB2 = (1, 2, 3, 5)         # load-batch 2 tiles: GENERAL MT >= 5 (kGenWideLB)
K_LAT_VEC = (1, 5, 8, 9, 16)  # gf_vec_kernel's INLINE_LAT blocks: k <= 8, k <= 16
K_LAT = (1, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16)  # both edges of every latency bucket
M_MULTI = {0: (9, 12, 17), 1: (17, 20, 32)}  # several row tiles with a short last one


def _case(form, binary, m, k, B, nt=3, cpw=0, lat=LAT_DWORD_DEFAULT, shift=0):
    seed =(m * 1000003 + k * 10007 + B * 101 + nt * 13 + shift * 7 + binary * 3 + len(form)) & 0x7FFFFFFF
    return Case(form, binary, m, k, B, nt, cpw, lat, shift, seed)


def vec_group(path, binary, m):
    """The cases of one (path, flavour, m): path "strided", "ptrs", "inline" (a device call with the latency
    threshold at 0) or "inline_lat" (a device call under the default threshold, B not a multiple of 16)."""
    form = path if path in ("strided", "ptrs") else "dev"
    lat = 0 if path == "inline" else LAT_DWORD_DEFAULT
    mt, _ = tile(binary, m)
    lb2 = not binary and mt >= 5
    ks = K_LAT_VEC if path == "inline_lat" else K_LB2 if lb2 else K_LB4
    k1 = 5 if lb2 or path == "inline_lat" else 7
    out = [_case(form, binary, m, k, B_MAIN, lat=lat) for k in ks]          # the full k list at NT 3
    if mt <= K_MAX_MT:
        out += [_case(form, binary, m, k1, B_MAIN, nt=nt, lat=lat) for nt in (0, 1, 2)]
    out.append(_case(form, binary, m, k1, B_BYTES, lat=lat))                 # byte-only block
    out.append(_case(form, binary, m, k1, B_MAIN, lat=lat, shift=1))         # whole block through the byte kernel
    return out


def cols_per_wg_cases():
    """One shape per mode with ECG_OPT_COLS_PER_WG = 1024."""
    return [_case("strided", 0, 4, 7, B_MAIN, cpw=1024), _case("ptrs", 1, 3, 7, B_MAIN, cpw=1024),
            _case("dev", 0, 2, 7, B_MAIN, cpw=1024, lat=0), _case("dev", 1, 5, 9, B_MAIN, cpw=1024)]


def lat_group(binary, m):
    """The latency kernel's buckets for one (flavour, MT): device calls, both EAGER forms."""
    return [_case("dev", binary, m, k, B) for k in K_LAT for B in (B_LAT_EAGER, B_LAT_PLAIN)]


def host_cases():
    """Host-tier calls (zero-copy staging, completion flags): the latency kernel; with the threshold at 0 the
    flagged INLINE_LAT form of gf_vec_kernel, which no device call reaches without a byte tail; k = 17 runs that
    kernel's load-batch loop (neither its k <= 8 nor its k <= 16 block); m > 8 GENERAL is two row tiles."""
    out = []
    for binary in (0, 1):
        out += [_case("host", binary, 4, 6, B_LAT_EAGER), _case("host", binary, 2, 10, B_LAT_PLAIN)]
        for m in (1, 4, 8):
            out += [_case("host", binary, m, k, B_LAT_EAGER, lat=0) for k in (5, 16, 17)]
        out.append(_case("host", binary, 12, 9, B_LAT_EAGER))
        out.append(_case("host", binary, 3, 6, B_MAIN))
    return out


VEC_PATHS = ("strided", "ptrs", "inline", "inline_lat")


def vec_groups():
    """[(path, flavour, m)] of the sweep's vector / byte cases."""
    out = []
    for path in VEC_PATHS:
        for binary in (0, 1):
            for m in range(1, (K_MAX_MT_BIN if binary else K_MAX_MT) + 1):
                out.append((path, binary, m))
            for m in M_MULTI[binary]:
                out.append((path, binary, m))
    return out


def lat_groups():
    return [(binary, m) for binary in (0, 1) for m in range(1, K_MAX_MT + 1)]


def all_cases():
    out = []
    for g in vec_groups():
        out += vec_group(*g)
    for g in lat_groups():
        out += lat_group(*g)
    return out + cols_per_wg_cases() + host_cases()


def declared_keys():
    keys = set()
    for c in all_cases():
        keys |= set(expected_keys(c))
    return keys | FIELD_PASS_KEYS


# The exhaustive field pass (tests/test_gpu_kernel_matrix.py): 1 -> 8 GENERAL ops whose coefficients walk 0..255
# and a 16 -> 16 op holding every coefficient, on the 16-byte path, the byte path and the latency path.
FIELD_B = 4096
FIELD_PASS_KEYS = {
    ("vec", MODE_STRIDED, 0, 3, 8), ("byte", MODE_STRIDED, 0, 8),
    ("lat", 0, 8, 4, 1), ("lat", 0, 7, 4, 1),   # the pointer call drops the all-zero row of coefficient 0
    ("vec", MODE_INLINE_LAT, 0, 3, 8),          # 16 -> 16 is two row tiles: not the latency kernel's
}

# Instantiations no public call reaches, each with the routing line that makes it so.
UNREACHABLE = {}
