"""Stripe scrubbing on the GPU: every gf_scrub_kernel / gf_scrub_byte_kernel tile of libecg_scrub.so against the
field's definition (tests/gf_plain.py), planted single bytes at the chunk, column and tail edges, the byte path,
the overwrite rule, the ErasureCode facade over oracle-encoded stripes, and the batch-scope flush.

Shapes are the smallest at which the kernels can go wrong: B = 4693 (gf_kernel_cases.B_MAIN: two full 2 KiB
workgroup chunks, a partial third, a 5-byte tail), B = 5 (byte path only), S = 3 strided stripes with 64-byte
bands of 0xC3 around every block and a block the check does not name.  Expected counts never come from the
library's own encode.

A check H = [C | I] over consecutive blocks (every encode) folds only C through the coefficient tables and XORs
the stored blocks in; any other H goes through the tables whole.  The sweep runs both forms on every tile.

INLINE (pointers in the kernel arguments) is reached through ecg_scrub.ec, whose matrix is the handle's own: RS(k, r)
gives GENERAL [C | I] tiles of r = 2..8 rows (one-row Vandermonde codes are all ones, so GENERAL MT = 1 has no INLINE
call), RS(k, 1) and HVPC(k1, 1, k2, 1) the BINARY ones; product codes, whose column checks read row parities, give
general checks: BINARY PC(k1, 1, k2, 1) from 3 rows, GENERAL PC(k1, 2, 1, 1) from 6.

Wide checks run k = 33 and k = 128 table columns, STRIDED on the widest tiles and INLINE on RS(120, 8).  The launch
geometries (workgroup -> chunk maps, column-loop lengths) are tests/test_gpu_check_geometry.py's.
"""
import ctypes
import json
import os

import numpy as np
import pytest

import check_geometry_cases as G
import gf_kernel_cases as C
import gf_plain

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
GUARD, BAND = 64, 0xC3
S3 = 3
K_SWEEP = (1, 2, 3, 4, 5, 7, 9, 14)   # every load-batch branch and remainder (batches of 4 and 2)
R_GENERAL = tuple(range(1, 9)) + (9, 17)
R_BINARY = tuple(range(1, 17)) + (17,)
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return torch


@pytest.fixture(scope="module")
def scrub(ecg):
    import ecg_scrub
    ecg_scrub.lib()
    return ecg_scrub


def _pitch(B):
    return (GUARD + B + GUARD + 15) & ~15  # every block 16-byte aligned in an aligned arena


def _arena(rng, S, slots, B, blocks=None):
    """[S][slots][pitch] host image: bands of 0xC3, random (or given) block bytes."""
    img = np.full((S, slots, _pitch(B)), BAND, np.uint8)
    img[:, :, GUARD:GUARD + B] = rng.integers(0, 256, (S, slots, B), dtype=np.uint8) if blocks is None else blocks
    return img


def _to_dev(torch, img, shift=0):
    flat = torch.empty(img.size + 16, dtype=torch.uint8, device="cuda")
    view = flat[shift:shift + img.size]
    view.copy_(torch.from_numpy(img.reshape(-1)))
    return view.view(img.shape)


def _blocks(d, B):
    return d[:, :, GUARD:GUARD + B]


def _want(H, img, src, B):
    """counts[s][p] by the definition: nonzero bytes of XOR_j H[p][j] * block src[j]."""
    return np.array([[np.count_nonzero(row) for row in gf_plain.apply(H, img[s, src, GUARD:GUARD + B])]
                     for s in range(img.shape[0])], dtype=np.int64)


def _planned_bytes(H, src, S, B, strided):
    """What the library declares it reads (scrub.cpp make_check, scrub_kernels.hip launch_scrub): every row tile
    reads all table columns; when H = [C | I] (unit columns last, over consecutive blocks in the strided form) only
    C goes through the tables and each stored block of the identity part is read once."""
    r, n = H.shape
    kg = n - r
    ident = kg >= 1 and np.array_equal(H[:, kg:], np.eye(r, dtype=np.int64)) and (
        not strided or all(src[kg + q] == src[kg] + q for q in range(r)))
    cols = kg if ident else n
    mt = min(r, C.K_MAX_MT_BIN if H[:, :cols].max() <= 1 else C.K_MAX_MT)
    return S * B * (((r + mt - 1) // mt) * cols + (r if ident else 0)), ident


def _check_call(torch, scrub, img, d, B, shift, H, src, call, strided=True, ident=None):
    """Run `call`, compare its counts with the definition, the arena with what was uploaded, and the counters
    with the declared launches and bytes."""
    H = np.asarray(H, dtype=np.int64)
    S = img.shape[0]
    nbytes, is_ident = _planned_bytes(H, src, S, B, strided)
    assert ident is None or ident == is_ident
    c0 = scrub.counters()
    got = call()
    torch.cuda.synchronize()
    c1 = scrub.counters()
    assert got.dtype == torch.int32 and tuple(got.shape) == (S, H.shape[0])
    want = _want(H, img, src, B)
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want), (H.shape, B, shift, got.cpu().numpy(), want)
    assert np.array_equal(d.cpu().numpy(), img), "the check wrote to its inputs"
    vec = (B & ~15) if shift % 16 == 0 else 0
    assert c1["launches"] - c0["launches"] == (vec > 0) + (vec < B)
    assert c1["bytes"] - c0["bytes"] == nbytes
    return want


def _sweep_matrix(binary, r, k):
    return C.matrix(C._case("strided", binary, r, k, C.B_MAIN))


def _strided_case(torch, scrub, binary, r, k, B, shift=0):
    H = _sweep_matrix(binary, r, k)
    rng = np.random.default_rng(1000 * r + 10 * k + binary + B)
    img = _arena(rng, S3, k + 1, B)
    d = _to_dev(torch, img, shift)
    src = [k - j for j in range(k)]  # slot 0 is not named
    # a one-row matrix that ends in a 1 (gf_kernel_cases.matrix puts one there) IS [C | I]; no other case here is
    want = _check_call(torch, scrub, img, d, B, shift, H, src, lambda: scrub.matrix_batch(H, src, _blocks(d, B)),
                       ident=None if r == 1 else False)
    if B >= 256:
        assert (want > 0.9 * B).all()  # random inputs: nearly every syndrome byte is nonzero


def _encode_shaped_case(torch, scrub, binary, r, k, B, shift=0):
    """H = [C | I] over consecutive blocks: C through the tables, the stored blocks XORed in (the identity path)."""
    H = np.concatenate([_sweep_matrix(binary, r, k), np.eye(r, dtype=np.int64)], axis=1)
    rng = np.random.default_rng(2000 * r + 10 * k + binary + B)
    img = _arena(rng, S3, k + r + 1, B)
    d = _to_dev(torch, img, shift)
    src = list(range(1, k + r + 1))  # slot 0 is not named
    _check_call(torch, scrub, img, d, B, shift, H, src, lambda: scrub.matrix_batch(H, src, _blocks(d, B)), ident=True)


def _inline_codes(ecg, binary, r):
    """Handles whose check has r rows of the wanted flavour: [C | I] checks (RS, HVPC: the identity path) and
    product codes, whose column checks over the row parities make H a general matrix."""
    F, P = ecg.ec_factory, ecg.CodingParameters
    out = []
    if binary:
        if r == 1:
            out.append((F(ecg.ECTYPE.RS, P(k=5, m=1)), True))
        else:
            k1 = (r + 1) // 2
            out.append((F(ecg.ECTYPE.HV_PC, P(k1=k1, m1=1, k2=r - k1, m2=1)), True))
        if r >= 3:
            k1 = r // 2
            out.append((F(ecg.ECTYPE.PC, P(k1=k1, m1=1, k2=r - 1 - k1, m2=1)), False))
    else:
        if r >= 2:
            out.append((F(ecg.ECTYPE.RS, P(k=3 + r % 5, m=r)), True))
        if r >= 6:
            out.append((F(ecg.ECTYPE.PC, P(k1=r - 4, m1=2, k2=1, m2=1)), False))
    return out


def _inline_case(torch, ecg, scrub, binary, r):
    for code, ident in _inline_codes(ecg, binary, r):
        k, m = code.k, code.m
        assert m == r
        H = np.asarray(code.check_matrix(), dtype=np.int64)
        assert int(H.max() <= 1) == binary
        for B in (C.B_MAIN, C.B_BYTES):
            rng = np.random.default_rng(77 * r + binary + B)
            img = _arena(rng, 1, k + m + 1, B)
            d = _to_dev(torch, img)
            blocks = [d[0, 1 + b, GUARD:GUARD + B] for b in range(k + m)]
            _check_call(torch, scrub, img, d, B, 0, H, list(range(1, k + m + 1)),
                        lambda: scrub.ec(code, blocks[:k], blocks[k:], B), strided=False, ident=ident)


_SWEEP = [(0, r) for r in R_GENERAL] + [(1, r) for r in R_BINARY]


@gpu
@pytest.mark.parametrize("binary,r", _SWEEP, ids=[f"{'bin' if b else 'gen'}-r{r}" for b, r in _SWEEP])
def test_tile_sweep(ecg, torch_cuda, scrub, binary, r):
    for k in K_SWEEP:
        _strided_case(torch_cuda, scrub, binary, r, k, C.B_MAIN)
    _strided_case(torch_cuda, scrub, binary, r, 7, C.B_BYTES)
    for k in (1, 4, 7):
        _encode_shaped_case(torch_cuda, scrub, binary, r, k, C.B_MAIN)
    _encode_shaped_case(torch_cuda, scrub, binary, r, 5, C.B_BYTES)
    _inline_case(torch_cuda, ecg, scrub, binary, r)


# ---- planted single bytes

RS64 = next(c for c in GOLDEN if c["name"] == "RS(6,4)")
POSITIONS = (0, 15, 16, 2047, 2048, 4687, 4688, 4692)  # column, chunk and tail edges of B_MAIN


def _consistent_rs64(S, B, seed):
    """[S][k + m][B] stripes whose parity is gf_plain's product of the golden RS(6,4) matrix with random data."""
    k, m = 6, 4
    M = np.asarray(RS64["matrix"], dtype=np.int64).reshape(m, k)
    rng = np.random.default_rng(seed)
    out = np.zeros((S, k + m, B), np.uint8)
    for s in range(S):
        out[s, :k] = rng.integers(0, 256, (k, B), dtype=np.uint8)
        out[s, k:] = gf_plain.apply(M, out[s, :k])
    return M, out


def _planted(torch, scrub, shift):
    k, m, B = 6, 4, C.B_MAIN
    assert B == 4693 and POSITIONS[-1] == B - 1 and POSITIONS[-3] == (B & ~15) - 1
    M, stripes = _consistent_rs64(S3, B, 64)
    img = _arena(None, S3, k + m + 1, B, blocks=np.concatenate([np.zeros((S3, 1, B), np.uint8), stripes], axis=1))
    d = _to_dev(torch, img, shift)
    view = d[:, 1:, GUARD:GUARD + B]  # slot 0 is not named
    flat = [int(v) for v in M.reshape(-1)]
    assert not scrub.encode_batch(k, m, flat, view).cpu().numpy().any()  # clean
    for block, rows in ((2, [p for p in range(m) if M[p, 2]]), (k + 1, [1])):
        assert block >= k or len(rows) == m  # a Vandermonde column has no zero: the field has no zero divisors
        for pos in POSITIONS:
            d[1, 1 + block, GUARD + pos] ^= 0x21
            got = scrub.encode_batch(k, m, flat, view).cpu().numpy()
            d[1, 1 + block, GUARD + pos] ^= 0x21
            want = np.zeros((S3, m), np.int32)
            want[1, rows] = 1
            assert np.array_equal(got, want), (block, pos, got)
    assert np.array_equal(d.cpu().numpy(), img)


@gpu
def test_planted_single_bytes(torch_cuda, scrub):
    _planted(torch_cuda, scrub, 0)


@gpu
def test_unaligned_base_runs_the_byte_kernel(torch_cuda, scrub):
    """The arena shifted by one byte: no block is 16-byte aligned, one byte-kernel launch covers everything."""
    _planted(torch_cuda, scrub, 1)
    for binary, r, k in ((0, 4, 7), (0, 9, 3), (1, 17, 5)):
        _strided_case(torch_cuda, scrub, binary, r, k, C.B_MAIN, shift=1)
        _encode_shaped_case(torch_cuda, scrub, binary, r, k, C.B_MAIN, shift=1)


@gpu
def test_counts_are_overwritten_not_accumulated(torch_cuda, scrub):
    torch = torch_cuda
    k, m, B = 6, 4, C.B_MAIN
    M, stripes = _consistent_rs64(S3, B, 65)
    flat = [int(v) for v in M.reshape(-1)]
    d = torch.from_numpy(stripes).cuda()
    out = torch.full((S3, m), -1, dtype=torch.int32, device="cuda")  # 0xFFFFFFFF
    assert scrub.encode_batch(k, m, flat, d, out=out) is out
    assert not out.cpu().numpy().any()
    noisy = stripes.copy()
    noisy[:, 3] = np.random.default_rng(5).integers(0, 256, (S3, B), dtype=np.uint8)
    H = np.concatenate([M, np.eye(m, dtype=np.int64)], axis=1)
    want = np.array([[np.count_nonzero(r) for r in gf_plain.apply(H, noisy[s])] for s in range(S3)])
    d.copy_(torch.from_numpy(noisy))
    for _ in range(2):
        scrub.encode_batch(k, m, flat, d, out=out)
        assert np.array_equal(out.cpu().numpy(), want)


# ---- wide checks: as many table columns as an INLINE launch has pointers (kInlineSrc = 128), and one past a batch

WIDE_K = (33, 128)


@gpu
@pytest.mark.parametrize("k", WIDE_K, ids=[f"k{k}" for k in WIDE_K])
def test_wide_checks_strided(torch_cuda, scrub, k):
    """k columns through the tables (a general H) and [C | I] with k + r <= 128 blocks, on the widest GENERAL and
    BINARY tiles."""
    for binary, r in ((0, 8), (1, 16)):
        _strided_case(torch_cuda, scrub, binary, r, k, C.B_MAIN)
        _encode_shaped_case(torch_cuda, scrub, binary, r, min(k, 128 - r), C.B_MAIN)


@gpu
def test_wide_check_inline(ecg, torch_cuda, scrub):
    """ecg_scrub.ec on RS(120, 8): 128 block pointers in the kernel arguments."""
    torch = torch_cuda
    code = ecg.ec_factory(ecg.ECTYPE.RS, ecg.CodingParameters(k=120, m=8))
    k, m, B = code.k, code.m, C.B_MAIN
    H = np.asarray(code.check_matrix(), dtype=np.int64)
    assert H.shape == (8, 128)
    img = _arena(np.random.default_rng(120), 1, k + m + 1, B)
    d = _to_dev(torch, img)
    blocks = [d[0, 1 + b, GUARD:GUARD + B] for b in range(k + m)]
    _check_call(torch, scrub, img, d, B, 0, H, list(range(1, k + m + 1)),
                lambda: scrub.ec(code, blocks[:k], blocks[k:], B), strided=False, ident=True)
    # a stripe that satisfies the check, damaged by the wide locate plan: sparse counts, every block's column
    stripes = G.consistent(gf_plain.apply, H[:, :k], 1, B, 428)
    G.apply_plan(stripes, [(0, b, pos, val) for s, b, pos, val in G.wide_plan(k + m, m) if s == 2])
    img = _arena(None, 1, k + m + 1, B, blocks=np.concatenate([np.zeros((1, 1, B), np.uint8), stripes], axis=1))
    d = _to_dev(torch, img)
    blocks = [d[0, 1 + b, GUARD:GUARD + B] for b in range(k + m)]
    want = _check_call(torch, scrub, img, d, B, 0, H, list(range(1, k + m + 1)),
                       lambda: scrub.ec(code, blocks[:k], blocks[k:], B), strided=False, ident=True)
    assert (want > 0).all() and (want < 500).all()


# ---- an all-zero matrix row: encode_check leaves its H row and its parity column zero

@gpu
def test_all_zero_matrix_row(torch_cuda, scrub):
    """encode_batch with row 1 of the RS(6,4) matrix zeroed: row 1 checks nothing, so its count stays zero and damage
    in parity block k + 1 is invisible; damage elsewhere is counted as by the definition over that H."""
    torch = torch_cuda
    k, m, B = 6, 4, C.B_MAIN
    M = np.asarray(RS64["matrix"], dtype=np.int64).reshape(m, k).copy()
    M[1] = 0
    rng = np.random.default_rng(69)
    stripes = np.zeros((S3, k + m, B), np.uint8)
    for s in range(S3):
        stripes[s, :k] = rng.integers(0, 256, (k, B), dtype=np.uint8)
        stripes[s, k:] = gf_plain.apply(M, stripes[s, :k])
    assert not stripes[:, k + 1].any()
    H = np.concatenate([M, np.eye(m, dtype=np.int64)], axis=1)
    H[1, k + 1] = 0
    for i, p in enumerate(POSITIONS):
        stripes[1, k + 1, p] ^= 0x10 + i                            # stripe 1: the unchecked block only
        stripes[2, (0, 5, k + m - 1)[i % 3], p] ^= 0x21 + i         # stripe 2: data blocks and a checked parity
    stripes[2, k + 1, 100:140] ^= 0x5A                              # and the unchecked one
    img = _arena(None, S3, k + m, B, blocks=stripes)
    d = _to_dev(torch, img)
    flat = [int(v) for v in M.reshape(-1)]
    want = _check_call(torch, scrub, img, d, B, 0, H, list(range(k + m)),
                       lambda: scrub.encode_batch(k, m, flat, _blocks(d, B)), ident=False)
    assert not want[0].any() and not want[1].any() and not want[:, 1].any()
    assert [int(v) for v in want[2]] == [6, 0, 6, 8]               # 3 + 3 data bytes; parity 9 adds 2 to its own row


# ---- the ErasureCode facade

@gpu
@pytest.mark.parametrize("c", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_facade(ecg, oracle, torch_cuda, scrub, c):
    """Stripe 0 as the oracle encoded it, stripe 1 + b with one byte range of block b corrupted: ec_batch reports
    zero, then exactly H's column support with the definition's counts; ec over one stripe's pointers agrees."""
    from oracle import ec_ref as E
    torch = torch_cuda
    B = C.B_MAIN
    ref = E.ec_factory(c["type"], E.CodingParameters(**c["params"]))
    code = ecg.ec_factory(c["type"], ecg.CodingParameters(**c["params"]))
    k, m = code.k, code.m
    n = k + m
    rng = np.random.default_rng(k * 100 + m)
    data = [rng.integers(0, 256, B, dtype=np.uint8) for _ in range(k)]
    coding = E.zeros(m, B)
    ref.encode(data, coding, B)
    clean = np.stack(data + list(coding))
    stripes = np.repeat(clean[None], n + 1, axis=0)
    for b in range(n):
        lo = (37 * b) % (B - 40)
        stripes[1 + b, b, lo:lo + 40] ^= rng.integers(1, 256, 40, dtype=np.uint8)
        stripes[1 + b, b, B - 1] ^= 0x01  # and the last tail byte
    H = np.asarray(code.check_matrix(), dtype=np.int64)
    want = np.array([[np.count_nonzero(r) for r in gf_plain.apply(H, stripes[s])] for s in range(n + 1)])
    assert not want[0].any()
    for b in range(n):
        assert set(np.flatnonzero(want[1 + b])) == set(np.flatnonzero(H[:, b])) != set()
    d = torch.from_numpy(stripes).cuda()
    got = scrub.ec_batch(code, d).cpu().numpy()
    assert np.array_equal(got, want), c["name"]
    for s in (0, 1, n):
        one = scrub.ec(code, [d[s, j] for j in range(k)], [d[s, k + j] for j in range(m)], B).cpu().numpy()
        assert np.array_equal(one[0], want[s]), (c["name"], s)
    assert scrub.suspects(H, got[0]) == []
    assert k + m - 1 in scrub.suspects(H, got[n])
    assert np.array_equal(d.cpu().numpy(), stripes)
    # a host-memory handle has no scrub: ECG_EINVAL, nothing launched
    ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_HOST, None)
    cnt = torch.zeros((n + 1, m), dtype=torch.int32, device="cuda")
    l0 = scrub.counters()["launches"]
    assert scrub.lib().ecg_scrub_ec_batch(code._h, d.data_ptr(), d.stride(0), d.stride(1), B, n + 1, cnt.data_ptr(),
                                          None) == ecg.ECG_EINVAL
    dp = (ctypes.c_void_p * k)(*[d[0, j].data_ptr() for j in range(k)])
    cp = (ctypes.c_void_p * m)(*[d[0, k + j].data_ptr() for j in range(m)])
    assert scrub.lib().ecg_scrub_ec(code._h, dp, cp, B, cnt.data_ptr()) == ecg.ECG_EINVAL
    assert scrub.counters()["launches"] == l0


@gpu
def test_scrub_flushes_the_batch_scope(ecg, torch_cuda, scrub):
    """A dev_matrix_encode recorded in a batch scope, then a scrub of the same blocks inside the scope: the scrub
    flushes the scope first, so it checks the encode's result (zero), not the stale parity."""
    torch = torch_cuda
    k, m, B = 6, 4, C.B_MAIN
    M, stripes = _consistent_rs64(1, B, 66)
    flat = [int(v) for v in M.reshape(-1)]
    want_parity = stripes[0, k:].copy()
    stripes[0, k:] = 0xA5  # stale
    d = torch.from_numpy(stripes).cuda()
    assert scrub.encode_batch(k, m, flat, d).cpu().numpy().all()  # stale parity fails every row
    with ecg.batch():
        ecg.dev_matrix_encode(k, m, flat, [d[0, j] for j in range(k)], [d[0, k + j] for j in range(m)], B)
        counts = scrub.encode_batch(k, m, flat, d)
    torch.cuda.synchronize()
    assert not counts.cpu().numpy().any()
    assert np.array_equal(d[0, k:].cpu().numpy(), want_parity)
