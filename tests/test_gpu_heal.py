"""In-place correction on the GPU: every gf_heal_kernel / gf_heal_byte_kernel of libecg_heal.so against the
definition (tests/heal_plain.py), which tries every error value for every candidate block instead of the kernels'
pivot-row ratio test and pivot division.

Every case uploads an arena, runs one call and compares THE WHOLE ARENA with the definition's image -- guard bands,
the block the check does not name and the stripes the call does not select included -- the report exactly, and
`counters()` with the declared launches and bytes.

Shapes are the locate's (tests/test_gpu_locate.py, whose arena helpers and damage plan this module uses): B = 4693
(two full 2 KiB workgroup chunks, a partial third, a 5-byte tail), B = 5 (byte path only), S = 3 strided stripes with
64-byte bands of 0xC3 around every block and a block the check does not name.  Stripes that satisfy their check are
built with tests/gf_plain.py (or the oracle's encode), never with the library's own encode.

ANY mode is refused over proportional columns, so the sweep's random matrices are nudged until no two columns of
[C | I] are proportional (`_distinct`), and the wide cases replace the one column of check_geometry_cases.wide_matrix
that is a multiple of a unit column.
"""
import json
import os

import numpy as np
import pytest

import check_geometry_cases as G
import gf_kernel_cases as C
import gf_plain
import heal_plain as HP
import locate_plain as LP
import test_gpu_locate as TL

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
MATRIX_CODES = [c for c in GOLDEN if "matrix" in c]   # RS, ERS and the LRC family
GUARD, BAND, S3 = TL.GUARD, TL.BAND, TL.S3
K_SWEEP = (1, 2, 3, 4, 5, 7, 9, 14)   # every load-batch branch and remainder (batches of 4 and 2)
B_MAIN, B_BYTES = C.B_MAIN, C.B_BYTES
POSITIONS = (0, 15, 16, 2047, 2048, B_MAIN - 6, B_MAIN - 1)   # column, chunk and tail edges of B_MAIN
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return torch


@pytest.fixture(scope="module")
def heal(ecg):
    import ecg_heal
    ecg_heal.lib()
    return ecg_heal


@pytest.fixture(scope="module")
def locate(ecg):
    import ecg_locate
    ecg_locate.lib()
    return ecg_locate


@pytest.fixture(scope="module")
def scrub(ecg):
    import ecg_scrub
    ecg_scrub.lib()
    return ecg_scrub


# ---- one call against the definition

def _expect(img, B, H, src, rows, targets):
    """(arena image after the call, [len(rows)][n + 2] reports) by the definition: heal_plain over the blocks `src`
    of every stripe in `rows`, target targets[i] for rows[i] (None: ANY)."""
    want = img.copy()
    reports = []
    for i, s in enumerate(rows):
        out, rep = HP.heal(H, img[s][src, GUARD:GUARD + B], None if targets is None else targets[i])
        want[s][src, GUARD:GUARD + B] = out
        reports.append(rep)
    return want, np.stack(reports)


def _ints(torch, values):
    return None if values is None else torch.tensor([int(v) for v in values], dtype=torch.int32, device="cuda")


def _run(torch, heal, img, d, B, shift, H, src, call, sel=None, targets=None):
    """Upload img into d, run `call`, compare the report, the whole arena and the counters with the definition.
    Returns (report, expected image), both numpy."""
    H = np.asarray(H, dtype=np.int64)
    n = H.shape[1]
    rows = list(range(img.shape[0])) if sel is None else list(sel)
    assert len(set(rows)) == len(rows)                              # the ids of a call must be distinct
    want, reports = _expect(img, B, H, src, rows, targets)
    d.copy_(torch.from_numpy(img).to(d.device))
    c0 = heal.counters()
    got = call()
    torch.cuda.synchronize()
    c1 = heal.counters()
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(rows), n + 2)
    g = got.cpu().numpy().astype(np.int64)
    assert np.array_equal(g, reports), (H.shape, B, shift, sel, targets, g, reports)
    assert (g[:, :n].sum(axis=1) + g[:, n + 1] == g[:, n]).all()
    after = d.cpu().numpy()
    if not np.array_equal(after, want):
        diff = np.argwhere(after != want)
        raise AssertionError((H.shape, B, shift, sel, targets, len(diff), diff[:8].tolist()))
    vec = (B & ~15) if shift % 16 == 0 else 0
    assert c1["launches"] - c0["launches"] == (vec > 0) + (vec < B)
    assert c1["bytes"] - c0["bytes"] == len(rows) * B * n
    return g, want


def _distinct(Cm):
    """Cm with its last row nudged, column by column, until no two nonzero columns of [Cm | I] are proportional."""
    Cm = Cm.copy()
    r, k = Cm.shape
    H = np.concatenate([Cm, np.eye(r, dtype=np.int64)], axis=1)
    e = np.arange(1, 256)

    def clash(j):
        if not H[:, j].any():
            return False
        multiples = gf_plain.TABLE[H[:, j]][:, e]
        others = [b for b in range(k + r) if b != j and (b < j or b >= k)]
        return any((multiples == H[:, b][:, None]).all(axis=0).any() for b in others)

    for j in range(k):
        for t in range(256 * r):
            if not clash(j):
                break
            row = r - 1 - t % r                              # the last row first: a column's leading zeros stay
            H[row, j] = (H[row, j] + 1) % 256
        assert not clash(j)
    return H[:, :k].copy()


def _strided_case(torch, heal, r, k, B, shift=0, sels=(None,), zero_col=False):
    """One random C (r x k): H = [C | I] over blocks 1.., then the same check with its columns reversed (a general
    H).  TARGET names column 0 for stripe 0, the last column (an identity block of [C | I]) for stripe 1 and a middle
    one for stripe 2; ANY from r = 2.  zero_col: column 0 of C is zeroed, its block is damaged (stripe 1) and named
    as stripe 1's target: nothing is written."""
    Cm = C.matrix(C._case("strided", 0, r, k, B_MAIN))
    if zero_col:
        Cm[:, 0] = 0
    if r >= 2:
        Cm = _distinct(Cm)
    stripes = TL._consistent(Cm, S3, B, 1000 * r + 10 * k + B)
    TL._damage(stripes, 7 * r + k)
    n = k + r
    blocks = np.concatenate([np.full((S3, 1, B), 0x77, np.uint8), stripes], axis=1)   # slot 0 is not named
    img = TL._arena(blocks)
    d = TL._to_dev(torch, img, shift)
    view = d[:, :, GUARD:GUARD + B]
    H = np.concatenate([Cm, np.eye(r, dtype=np.int64)], axis=1)
    src = list(range(1, n + 1))
    for Hx, srcx, zero_at in ((H, src, 0), (H[:, ::-1].copy(), src[::-1], n - 1)):
        if r >= 2:
            assert LP.proportional_pairs(Hx)[0] == 0
        per_stripe = [0, zero_at if zero_col else n - 1, n // 2]
        for ids in sels:
            rows = list(range(S3)) if ids is None else list(ids)
            for targets in ([per_stripe[s] for s in rows],) + ((None,) if r >= 2 else ()):
                g, _ = _run(torch, heal, img, d, B, shift, Hx, srcx,
                            lambda: heal.matrix_batch(Hx, srcx, view, stripe_ids=_ints(torch, ids),
                                                      targets=_ints(torch, targets)), sel=ids, targets=targets)
                assert not g[rows.index(0)].any()                    # the clean stripe's row is all zero
                assert g[rows.index(2), n] > 0
                if zero_col:
                    assert not g[:, zero_at].any()


@gpu
@pytest.mark.parametrize("r", range(1, 9), ids=[f"r{r}" for r in range(1, 9)])
def test_every_r_strided(torch_cuda, heal, r):
    for k in K_SWEEP:
        _strided_case(torch_cuda, heal, r, k, B_MAIN)
    _strided_case(torch_cuda, heal, r, 7, B_BYTES)
    _strided_case(torch_cuda, heal, r, 5, B_MAIN, zero_col=True)
    _strided_case(torch_cuda, heal, r, 3, B_MAIN, sels=([2, 0],))


@gpu
@pytest.mark.parametrize("r", range(1, 9), ids=[f"r{r}" for r in range(1, 9)])
def test_every_r_inline(ecg, torch_cuda, heal, r):
    """ecg_heal.ec over RS(k, r)'s own [C | I] check: the INLINE kernels of every R, both paths, TARGET (the first
    block, the last identity block) and ANY."""
    torch = torch_cuda
    code = ecg.ec_factory(ecg.ECTYPE.RS, ecg.CodingParameters(k=3 + r % 5, m=r))
    k, n = code.k, code.k + code.m
    H = np.asarray(code.check_matrix(), dtype=np.int64)
    assert np.array_equal(H[:, k:], np.eye(r, dtype=np.int64))
    for B in (B_MAIN, B_BYTES):
        stripes = TL._consistent(H[:, :k], 3, B, 77 * r + B)
        TL._damage(stripes, 5 * r + B)
        for s in range(3):
            img = TL._arena(np.concatenate([np.full((1, 1, B), 0x77, np.uint8), stripes[s:s + 1]], axis=1))
            d = TL._to_dev(torch, img)
            blocks = [d[0, 1 + b, GUARD:GUARD + B] for b in range(n)]
            for target in (0, n - 1) + ((heal.ANY,) if r >= 2 else ()):
                _run(torch, heal, img, d, B, 0, H, list(range(1, n + 1)),
                     lambda: heal.ec(code, blocks[:k], blocks[k:], B, target=target),
                     targets=None if target == heal.ANY else [target])


# ---- edges: single bytes, two bytes of a dword, two blocks of a column

RS64 = next(c for c in GOLDEN if c["name"] == "RS(6,4)")
RS104 = next(c for c in GOLDEN if c["name"] == "RS(10,4)")


def _code(c, S, B, seed):
    k, m = c["k"], c["m"]
    M = np.asarray(c["matrix"], dtype=np.int64).reshape(m, k)
    return M, [int(v) for v in M.reshape(-1)], np.concatenate([M, np.eye(m, dtype=np.int64)], axis=1), \
        TL._consistent(M, S, B, seed)


def _encode_case(torch, heal, c, stripes, original=None, sel=None, targets=None, shift=0):
    """stripes [S][n][B] (damaged) inside an arena whose slot 0 the check does not name, through encode_batch.
    original: if given, the stripes the selected rows must come back to.  Returns (report, image after, arena)."""
    k, m = c["k"], c["m"]
    n = k + m
    S, _, B = stripes.shape
    flat = [int(v) for v in c["matrix"]]
    H = np.concatenate([np.asarray(flat, dtype=np.int64).reshape(m, k), np.eye(m, dtype=np.int64)], axis=1)
    img = TL._arena(np.concatenate([np.zeros((S, 1, B), np.uint8), stripes], axis=1))
    d = TL._to_dev(torch, img, shift)
    view = d[:, 1:, GUARD:GUARD + B]
    g, want = _run(torch, heal, img, d, B, shift, H, list(range(1, n + 1)),
                   lambda: heal.encode_batch(k, m, flat, view, stripe_ids=_ints(torch, sel),
                                             targets=_ints(torch, targets)), sel=sel, targets=targets)
    if original is not None:
        rows = list(range(S)) if sel is None else list(sel)
        assert np.array_equal(want[rows][:, 1:, GUARD:GUARD + B], original[rows])
    return g, want, (img, d, view)


def _planted(torch, heal, shift):
    k, m, B = 6, 4, B_MAIN
    n = k + m
    assert B == 4693 and POSITIONS[-2] == (B & ~15) - 1
    _, _, _, original = _code(RS64, S3, B, 64)
    i = 0
    for block in (0, 4, n - 1):                        # the first, a middle and the last block: an identity block
        for pos in POSITIONS:
            stripes = original.copy()
            stripes[1, block, pos] ^= 0x21 + i
            targets = None if i % 2 == 0 else [-1, block, block]
            g, _, _ = _encode_case(torch, heal, RS64, stripes, original=original, targets=targets, shift=shift)
            want = np.zeros((S3, n + 2), np.int64)
            want[1, block] = want[1, n] = 1
            assert np.array_equal(g, want), (block, pos, g)
            i += 1


@gpu
def test_planted_single_bytes(torch_cuda, heal):
    _planted(torch_cuda, heal, 0)


@gpu
def test_unaligned_base_runs_the_byte_kernel(torch_cuda, heal):
    """The arena shifted by one byte: no block is 16-byte aligned, one byte-kernel launch covers everything (_run
    counts the launches)."""
    _planted(torch_cuda, heal, 1)
    for r, k in ((1, 4), (4, 7), (8, 3)):
        _strided_case(torch_cuda, heal, r, k, B_MAIN, shift=1, sels=(None, [2, 0]))


@gpu
def test_two_bytes_of_one_dword_and_two_blocks_of_one_column(torch_cuda, heal):
    """Two bytes of one dword of one block with different error values (the byte mask keeps the other two), and two
    different blocks damaged at different bytes of the same 16-byte column (one lane stores twice), in the vector
    part, across its last column and in the tail."""
    _, _, _, original = _code(RS64, S3, B_MAIN, 71)
    stripes = original.copy()
    stripes[1, 2, 33] ^= 0x01
    stripes[1, 2, 35] ^= 0xFE                          # same dword, another value; bytes 32 and 34 intact
    stripes[1, 7, 4672 + 1] ^= 0x80                    # the last full column of the vector part
    stripes[1, 7, 4672 + 2] ^= 0x7F
    stripes[2, 0, 2048 + 3] ^= 0x11                    # two blocks, one column, different bytes
    stripes[2, 9, 2048 + 12] ^= 0x22
    stripes[2, 3, 4688] ^= 0x33                        # and in the 5-byte tail: the byte kernel
    stripes[2, 6, 4692] ^= 0x44
    g, _, _ = _encode_case(torch_cuda, heal, RS64, stripes, original=original)
    assert [int(v) for v in g[1, [2, 7, 10, 11]]] == [2, 2, 4, 0]
    assert [int(v) for v in g[2, [0, 9, 3, 6, 10, 11]]] == [1, 1, 1, 1, 4, 0]
    g, want, _ = _encode_case(torch_cuda, heal, RS64, stripes, targets=[0, 2, 9])
    assert g[1, 2] == 2 and g[1, 11] == 2 and g[2, 9] == 1 and g[2, 11] == 3
    assert np.array_equal(want[1, 1 + 7, GUARD:GUARD + B_MAIN], stripes[1, 7])     # block 7 stays damaged


# ---- more damaged blocks than r; two blocks at one position

def _six_blocks(B, seed):
    _, _, _, original = _code(RS104, S3, B, seed)
    stripes = original.copy()
    rng = np.random.default_rng(seed)
    blocks = (0, 2, 5, 9, 11, 13)
    spots = (0, 700, 2040, 2900, 4000, B - 30)         # disjoint runs of 30: a chunk edge, the tail
    for b, lo in zip(blocks, spots):
        stripes[1, b, lo:lo + 30] ^= rng.integers(1, 256, 30, dtype=np.uint8)
        stripes[2, b, lo + 40:lo + 45] ^= rng.integers(1, 256, 5, dtype=np.uint8) if lo + 45 <= B else 0
    return original, stripes, blocks


@gpu
def test_six_damaged_blocks_of_rs_10_4_at_disjoint_positions(torch_cuda, heal):
    """Six erasures are beyond an RS(10,4) decode; ANY restores them all, TARGET only the named block's positions."""
    original, stripes, blocks = _six_blocks(B_MAIN, 72)
    g, _, _ = _encode_case(torch_cuda, heal, RS104, stripes, original=original)
    assert [int(v) for v in g[1, list(blocks)]] == [30] * 6 and g[1, 14] == 180 and g[1, 15] == 0
    g, want, _ = _encode_case(torch_cuda, heal, RS104, stripes, targets=[3, 5, 11])
    assert g[1, 5] == 30 and g[1, 14] == 180 and g[1, 15] == 150 and g[1, :14].sum() == 30
    fixed = stripes.copy()
    fixed[1, 5], fixed[2, 11] = original[1, 5], original[2, 11]
    assert np.array_equal(want[:, 1:, GUARD:GUARD + B_MAIN], fixed)


@gpu
def test_two_blocks_at_one_position(torch_cuda, heal):
    """r = 4 (MDS): untouched and counted.  r = 2: whatever the definition does (a third block may be written)."""
    _, _, _, original = _code(RS104, S3, B_MAIN, 73)
    stripes = original.copy()
    for pos in (5, 2047, 4690):
        stripes[1, 2, pos] ^= 0x5A
        stripes[1, 7, pos] ^= 0xC3
    g, want, _ = _encode_case(torch_cuda, heal, RS104, stripes)
    assert not g[1, :14].any() and g[1, 14] == g[1, 15] == 3
    assert np.array_equal(want[:, 1:, GUARD:GUARD + B_MAIN], stripes)
    rs62 = next(c for c in GOLDEN if c["name"] == "RS(6,2)")
    _, _, _, original = _code(rs62, S3, B_MAIN, 74)
    stripes = original.copy()
    rng = np.random.default_rng(74)
    for pos in (5, 100, 2047, 2048, 3000, 4687, 4690):
        stripes[1, 1, pos] ^= rng.integers(1, 256, dtype=np.uint8)
        stripes[1, 6, pos] ^= rng.integers(1, 256, dtype=np.uint8)
        stripes[2, 0, pos] ^= rng.integers(1, 256, dtype=np.uint8)
        stripes[2, 3, pos] ^= rng.integers(1, 256, dtype=np.uint8)
    g, _, _ = _encode_case(torch_cuda, heal, rs62, stripes)
    assert g[1, 8] == g[2, 8] == 7


# ---- targets

@gpu
def test_target_with_the_wrong_block_and_out_of_range(torch_cuda, heal):
    _, _, _, original = _code(RS64, S3, B_MAIN, 75)
    stripes = original.copy()
    TL._damage(stripes, 75)
    stripes[0, 4, 10:50] ^= 0x3C                                     # stripe 0 too
    n = 10
    for targets in ([5, 3, 2], [-1, n, -7], [n + 100, -(1 << 31), (1 << 31) - 1]):
        if targets[0] == 5:                                          # the wrong blocks: nothing of theirs is explained
            votes = np.stack([LP.votes(np.concatenate([np.asarray(RS64["matrix"]).reshape(4, 6),
                                                       np.eye(4, dtype=np.int64)], axis=1), stripes[s])
                              for s in range(S3)])
            assert votes[0, 5] == 0 and votes[1, 3] == 0 and votes[2, 2] == 0
        g, want, _ = _encode_case(torch_cuda, heal, RS64, stripes, targets=targets)
        assert np.array_equal(want[:, 1:, GUARD:GUARD + B_MAIN], stripes)          # bit-identical
        assert not g[:, :n].any() and (g[:, n] > 0).all() and np.array_equal(g[:, n + 1], g[:, n])


@gpu
def test_target_on_rs_8_1(ecg, torch_cuda, heal):
    """r = 1: ANY is refused, TARGET restores the block the caller names."""
    rs81 = next(c for c in GOLDEN if c["name"] == "RS(8,1)")
    _, flat, _, original = _code(rs81, S3, B_MAIN, 76)
    stripes = original.copy()
    rng = np.random.default_rng(76)
    stripes[0, 8, 4600:] ^= rng.integers(1, 256, B_MAIN - 4600, dtype=np.uint8)      # the parity, into the tail
    stripes[1, 0, 0:70] ^= rng.integers(1, 256, 70, dtype=np.uint8)
    stripes[2, 5] = rng.integers(0, 256, B_MAIN, dtype=np.uint8)                     # a whole block
    g, _, (_, d, view) = _encode_case(torch_cuda, heal, rs81, stripes, original=original, targets=[8, 0, 5])
    assert g[0, 8] == B_MAIN - 4600 and g[1, 0] == 70 and g[2, 5] > 0.98 * B_MAIN and not g[:, 10].any()
    with pytest.raises(ecg.EcgError) as e:
        heal.encode_batch(8, 1, flat, view)
    assert e.value.code == ecg.ECG_EINVAL and b"proportional" in ecg.lib().ecg_last_error()


@gpu
def test_whole_block_garbage_target(torch_cuda, heal):
    _, _, _, original = _code(RS64, S3, B_MAIN, 77)
    stripes = original.copy()
    rng = np.random.default_rng(77)
    stripes[1, 3] = rng.integers(0, 256, B_MAIN, dtype=np.uint8)     # a data block
    stripes[2, 8] = rng.integers(0, 256, B_MAIN, dtype=np.uint8)     # a parity block
    g, _, _ = _encode_case(torch_cuda, heal, RS64, stripes, original=original, targets=[0, 3, 8])
    assert not g[0].any() and g[1, 3] == g[1, 10] > 0.98 * B_MAIN and g[2, 8] == g[2, 10] > 0.98 * B_MAIN
    g, _, _ = _encode_case(torch_cuda, heal, RS64, stripes, original=original)       # and ANY
    assert g[1, 3] == g[1, 10] and g[2, 8] == g[2, 10] and not g[:, 11].any()


# ---- selections, idempotence, batch scope

@gpu
def test_selections(torch_cuda, heal):
    """[2, 0] with stripe 1 damaged too: it stays damaged, byte for byte (_run compares the whole arena); [1] alone; a
    NULL selection heals them all."""
    _, _, _, original = _code(RS64, S3, B_MAIN, 78)
    stripes = original.copy()
    TL._damage(stripes, 78)
    stripes[0, 9, 2040:2060] ^= 0x99
    for sel, targets in (([2, 0], None), ([2, 0], [5, 9]), ([1], None), ([1], [0])):
        g, want, _ = _encode_case(torch_cuda, heal, RS64, stripes, sel=sel, targets=targets)
        for s in set(range(S3)) - set(sel):
            assert np.array_equal(want[s, 1:, GUARD:GUARD + B_MAIN], stripes[s]) and not \
                np.array_equal(stripes[s], original[s])
    g, want, _ = _encode_case(torch_cuda, heal, RS64, stripes)
    assert np.array_equal(want[[0, 1], 1:, GUARD:GUARD + B_MAIN], original[[0, 1]])
    assert g[2, 11] == 1                               # stripe 2: two blocks at one position stay


@gpu
def test_idempotence_and_report_overwritten(torch_cuda, heal):
    torch = torch_cuda
    _, flat, _, original = _code(RS64, S3, B_MAIN, 79)
    stripes = original.copy()
    stripes[1, 2, 100:2300] ^= 0x42
    stripes[2, 9, B_MAIN - 3:] ^= 0x17
    g, want, (img, d, view) = _encode_case(torch, heal, RS64, stripes, original=original)
    assert g[1, 2] == 2200 and g[2, 9] == 3
    out = torch.full((S3, 12), -1, dtype=torch.int32, device="cuda")     # 0xFFFFFFFF
    assert heal.encode_batch(6, 4, flat, view, out=out) is out
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()                                   # a second call reports all zeros
    assert np.array_equal(d.cpu().numpy(), want)                         # and leaves the arena unchanged


@gpu
def test_prefilled_out_is_zeroed_before_the_kernels(torch_cuda, heal):
    """RS(6,4), S = 2, B = 48 + 5 (a vector and a byte launch): the report written into an `out` prefilled with a
    nonzero pattern equals the report of a call without `out` over the same damage, so the zeroing of the report still
    precedes both kernels on the stream."""
    torch = torch_cuda
    B = 48 + 5
    _, flat, _, original = _code(RS64, 2, B, 80)
    stripes = original.copy()
    stripes[0, 1, 3] ^= 0x5A
    stripes[0, 7, 20:40] ^= 0x11
    stripes[1, 0, 46:50] ^= 0x07                                         # across the end of the vector path
    stripes[1, 9, B - 2:] ^= 0x33
    g, want, (img, d, view) = _encode_case(torch, heal, RS64, stripes, original=original)
    assert g[0, 1] == 1 and g[0, 7] == 20 and g[1, 0] == 4 and g[1, 9] == 2
    d.copy_(torch.from_numpy(img).to(d.device))                          # damaged again
    out = torch.full((2, 12), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    c0 = heal.counters()
    assert heal.encode_batch(6, 4, flat, view, out=out) is out
    torch.cuda.synchronize()
    assert heal.counters()["launches"] - c0["launches"] == 2             # the vector and the byte kernel
    assert np.array_equal(out.cpu().numpy().astype(np.int64), g)
    assert np.array_equal(d.cpu().numpy(), want)


@gpu
def test_heal_flushes_the_batch_scope(ecg, torch_cuda, heal):
    """A dev_matrix_encode recorded in a batch scope, then a heal of the same blocks inside the scope: the heal
    flushes the scope first, so it sees the encode's parity (nothing to correct), not the stale one."""
    torch = torch_cuda
    k, m, B = 6, 4, B_MAIN
    _, flat, _, stripes = _code(RS64, 1, B, 80)
    want = stripes.copy()
    stripes[0, k:] = 0xA5  # stale
    d = torch.from_numpy(stripes).cuda()
    with ecg.batch():
        ecg.dev_matrix_encode(k, m, flat, [d[0, j] for j in range(k)], [d[0, k + j] for j in range(m)], B)
        report = heal.encode_batch(k, m, flat, d)
    torch.cuda.synchronize()
    assert not report.cpu().numpy().any()
    assert np.array_equal(d.cpu().numpy(), want)


# ---- the ErasureCode facade: INLINE through ec, STRIDED through ec_batch

@gpu
@pytest.mark.parametrize("c", MATRIX_CODES, ids=[c["name"] for c in MATRIX_CODES])
def test_facade(ecg, oracle, torch_cuda, heal, c):
    """Stripes as the oracle encoded them, stripe 1 + b with a byte range and the last byte of block b damaged.
    ec over one stripe's pointers (INLINE) restores it in ANY mode (refused for RS(8,1): TARGET there) and in TARGET
    mode; ec_batch over all of them agrees with the definition."""
    from oracle import ec_ref as E
    torch = torch_cuda
    B = B_MAIN
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
    src = list(range(n))
    # INLINE: one stripe at a time, a clean one and a few damaged ones (a data block, the last parity block)
    for s in (0, 1, k, n):
        img = TL._arena(stripes[s:s + 1])
        d = TL._to_dev(torch, img)
        blocks = [d[0, b, GUARD:GUARD + B] for b in range(n)]
        for target in ([heal.ANY] if m >= 2 else []) + [max(s - 1, 0)]:
            g, want = _run(torch, heal, img, d, B, 0, H, src,
                           lambda: heal.ec(code, blocks[:k], blocks[k:], B, target=target),
                           targets=None if target == heal.ANY else [target])
            assert np.array_equal(want[0, :, GUARD:GUARD + B], clean), (c["name"], s, target)
            assert g[0, n] == (41 if s else 0) and g[0, n + 1] == 0
    if m == 1:
        with pytest.raises(ecg.EcgError) as e:
            heal.ec(code, blocks[:k], blocks[k:], B)
        assert e.value.code == ecg.ECG_EINVAL
    # STRIDED: all n + 1 stripes at once
    img = TL._arena(stripes)
    d = TL._to_dev(torch, img)
    view = d[:, :, GUARD:GUARD + B]
    targets = [-1] + list(range(n))
    for tg in ([None] if m >= 2 else []) + [targets]:
        g, want = _run(torch, heal, img, d, B, 0, H, src,
                       lambda: heal.ec_batch(code, view, targets=_ints(torch, tg)), targets=tg)
        assert np.array_equal(want[:, :, GUARD:GUARD + B], np.repeat(clean[None], n + 1, axis=0)), c["name"]
    sel = [n, 1]
    _run(torch, heal, img, d, B, 0, H, src,
         lambda: heal.ec_batch(code, view, stripe_ids=_ints(torch, sel), targets=_ints(torch, [n - 1, 0])),
         sel=sel, targets=[n - 1, 0])


@gpu
@pytest.mark.parametrize("name", ["PC(4,2,2,1)", "PC(4,1,4,1)"])
def test_larger_codes_are_refused(ecg, torch_cuda, heal, name):
    """r > 8 (PC(4,1,4,1) has r = 9): ECG_EINVAL with the reason, nothing launched, nothing written."""
    torch = torch_cuda
    c = next(g for g in GOLDEN if g["name"] == name)
    code = ecg.ec_factory(c["type"], ecg.CodingParameters(**c["params"]))
    assert code.m > 8
    n = code.k + code.m
    d = torch.full((2, n, 64), 0x5A, dtype=torch.uint8, device="cuda")
    l0 = heal.counters()["launches"]
    with pytest.raises(ecg.EcgError) as e:
        heal.ec_batch(code, d, targets=_ints(torch, [0, 1]))
    assert e.value.code == ecg.ECG_EINVAL and f"r = {code.m}".encode() in ecg.lib().ecg_last_error()
    with pytest.raises(ecg.EcgError) as e:
        heal.ec(code, [d[0, j] for j in range(code.k)], [d[0, code.k + j] for j in range(code.m)], 64, target=0)
    assert e.value.code == ecg.ECG_EINVAL
    assert heal.counters()["launches"] == l0 and bool((d == 0x5A).all())


# ---- wide checks: n + 2 counters in three registers per lane, pivot rows eight per word, r x n ratio tables and
# 1 x n pivot inverses, 128 pointers in the kernel arguments

def _wide_matrix(n, r):
    """check_geometry_cases.wide_matrix, except that its column n - r - 2 -- zero down to its last row, hence a
    multiple of the unit column of row r - 1, which ANY mode refuses -- starts one row higher: pivot row r - 2, still
    in a high word of the packed pivots."""
    Cm = G.wide_matrix(n, r).copy()
    Cm[r - 2, n - r - 2] = 1 + n % 255
    H = np.concatenate([Cm, np.eye(r, dtype=np.int64)], axis=1)
    assert LP.proportional_pairs(H) == (0, 0)
    return Cm, H


@gpu
@pytest.mark.parametrize("n", (64, 128))
def test_wide_checks(torch_cuda, heal, n):
    """wide_plan: stripe 1 with every block damaged inside one wave, stripe 2 with every block damaged all over (and
    a few positions where blocks 0 and n - 1 are both damaged: left and counted).  ANY over [C | I] and over the same
    check with its columns reversed; TARGET 0 and n - 1."""
    torch = torch_cuda
    r, B = 8, B_MAIN
    Cm, H = _wide_matrix(n, r)
    original = G.consistent(gf_plain.apply, Cm, S3, B, 5000 + 10 * n + r)
    stripes = original.copy()
    G.apply_plan(stripes, G.wide_plan(n, r))
    img = TL._arena(np.concatenate([np.full((S3, 1, B), 0x77, np.uint8), stripes], axis=1))   # slot 0 is not named
    d = TL._to_dev(torch, img)
    view = d[:, :, GUARD:GUARD + B]
    src = list(range(1, n + 1))
    g, want = _run(torch, heal, img, d, B, 0, H, src, lambda: heal.matrix_batch(H, src, view))
    assert not g[0].any() and (g[1:, :n] > 0).all() and g[1, n + 1] == 0 and g[2, n + 1] == G.WIDE_DOUBLES
    assert np.array_equal(want[:2, 1:, GUARD:GUARD + B], original[:2])             # stripe 1 comes back whole
    assert np.count_nonzero(want[2, 1:, GUARD:GUARD + B] != original[2]) == 2 * G.WIDE_DOUBLES
    Hr, srcr = H[:, ::-1].copy(), src[::-1]
    gr, _ = _run(torch, heal, img, d, B, 0, Hr, srcr, lambda: heal.matrix_batch(Hr, srcr, view))
    assert np.array_equal(gr[:, :n], g[:, n - 1::-1][:, :n]) and np.array_equal(gr[:, n:], g[:, n:])
    for targets in ([0, 0, n - 1], [n - 1, n - 1, 0]):
        gt, _ = _run(torch, heal, img, d, B, 0, H, src,
                     lambda: heal.matrix_batch(H, src, view, targets=_ints(torch, targets)), targets=targets)
        assert gt[1, targets[1]] == G.block_count(targets[1]) and gt[1, :n].sum() == gt[1, targets[1]]


@gpu
def test_wide_check_through_the_byte_kernel(torch_cuda, heal):
    torch = torch_cuda
    n, r, B = 128, 8, B_MAIN
    Cm, H = _wide_matrix(n, r)
    stripes = G.consistent(gf_plain.apply, Cm, S3, B, 5000 + 10 * n + r)
    G.apply_plan(stripes, G.wide_plan(n, r))
    img = TL._arena(np.concatenate([np.full((S3, 1, B), 0x77, np.uint8), stripes], axis=1))
    d = TL._to_dev(torch, img, 1)
    view = d[:, :, GUARD:GUARD + B]
    src = list(range(1, n + 1))
    _run(torch, heal, img, d, B, 1, H, src, lambda: heal.matrix_batch(H, src, view))


@gpu
def test_wide_inline(ecg, torch_cuda, heal):
    """ecg_heal.ec over RS(120, 8)'s 128 block pointers in the kernel arguments."""
    torch = torch_cuda
    k, m = G.WIDE_INLINE[0]
    code = ecg.ec_factory(ecg.ECTYPE.RS, ecg.CodingParameters(k=k, m=m))
    n, B = k + m, B_MAIN
    H = np.asarray(code.check_matrix(), dtype=np.int64)
    original = G.consistent(gf_plain.apply, H[:, :k], S3, B, 300 + n)
    stripes = original.copy()
    G.apply_plan(stripes, G.wide_plan(n, m, seed=1))
    for s in (1, 2):
        img = TL._arena(np.concatenate([np.full((1, 1, B), 0x77, np.uint8), stripes[s:s + 1]], axis=1))
        d = TL._to_dev(torch, img)
        blocks = [d[0, 1 + b, GUARD:GUARD + B] for b in range(n)]
        g, want = _run(torch, heal, img, d, B, 0, H, list(range(1, n + 1)),
                       lambda: heal.ec(code, blocks[:k], blocks[k:], B))
        assert (g[0, :n] > 0).all()
        if s == 1:
            assert np.array_equal(want[0, 1:, GUARD:GUARD + B], original[1])


@gpu
def test_n_129_is_refused(ecg, torch_cuda, heal):
    """RS(121, 8) has n = 129 > 128: ECG_EINVAL from both forms, nothing launched."""
    torch = torch_cuda
    k, m = G.WIDE_REFUSED
    code = ecg.ec_factory(ecg.ECTYPE.RS, ecg.CodingParameters(k=k, m=m))
    d = torch.zeros((2, k + m, 64), dtype=torch.uint8, device="cuda")
    l0 = heal.counters()["launches"]
    with pytest.raises(ecg.EcgError) as e:
        heal.ec(code, [d[0, j] for j in range(k)], [d[0, k + j] for j in range(m)], 64)
    assert e.value.code == ecg.ECG_EINVAL and b"n = 129" in ecg.lib().ecg_last_error()
    with pytest.raises(ecg.EcgError) as e:
        heal.ec_batch(code, d)
    assert e.value.code == ecg.ECG_EINVAL
    assert heal.counters()["launches"] == l0


# ---- scrub -> dirty -> heal -> re-scrub, and scrub -> locate -> targets_from_votes -> heal

def _store(seed):
    k, m, S, B = 10, 4, 8, B_MAIN
    M = [int(v) for v in RS104["matrix"]]
    original = TL._consistent(np.asarray(M, dtype=np.int64).reshape(m, k), S, B, seed)
    damaged = original.copy()
    rng = np.random.default_rng(11)
    damaged[2, 3, 100:2300] = rng.integers(0, 256, 2200, dtype=np.uint8)      # a data block, across a chunk edge
    damaged[5, 7, [0, 2048, B - 1]] ^= np.array([1, 0x80, 0xFF], np.uint8)    # a data block, single bytes
    damaged[6, 12, B - 40:] ^= 0x3C                                           # a parity block, into the tail
    return k, m, M, original, damaged


@gpu
def test_end_to_end_any(torch_cuda, scrub, locate, heal):
    torch = torch_cuda
    k, m, M, original, damaged = _store(104)
    damaged[6, 1, 300:310] ^= 0x55                                            # stripe 6: a second block elsewhere
    d = torch.from_numpy(damaged).cuda()
    sel = locate.dirty(scrub.encode_batch(k, m, M, d))
    assert sel.cpu().tolist() == [2, 5, 6]
    votes = locate.encode_batch(k, m, M, d, stripe_ids=sel).cpu().numpy()     # the dry run
    report = heal.encode_batch(k, m, M, d, stripe_ids=sel).cpu().numpy()
    assert np.array_equal(report, votes)
    assert [locate.verdict(row) for row in report] == [(3, [3]), (7, [7]), (LP.MULTIPLE, [1, 12])]
    assert np.array_equal(d.cpu().numpy(), original)
    again = scrub.encode_batch(k, m, M, d)
    assert not again.cpu().numpy().any() and locate.dirty(again).numel() == 0


@gpu
def test_end_to_end_target(torch_cuda, scrub, locate, heal):
    torch = torch_cuda
    k, m, M, original, damaged = _store(105)
    d = torch.from_numpy(damaged).cuda()
    sel = locate.dirty(scrub.encode_batch(k, m, M, d))
    assert sel.cpu().tolist() == [2, 5, 6]
    votes = locate.encode_batch(k, m, M, d, stripe_ids=sel)
    targets = heal.targets_from_votes(votes)
    assert targets.dtype == torch.int32 and targets.is_cuda and targets.cpu().tolist() == [3, 7, 12]
    assert np.array_equal(targets.cpu().numpy(), HP.targets_from_votes(votes.cpu().numpy()))
    report = heal.encode_batch(k, m, M, d, stripe_ids=sel, targets=targets).cpu().numpy()
    assert np.array_equal(report, votes.cpu().numpy())
    assert np.array_equal(d.cpu().numpy(), original)
    assert not scrub.encode_batch(k, m, M, d).cpu().numpy().any()


@gpu
def test_targets_from_votes(torch_cuda, heal):
    torch = torch_cuda
    votes = np.array([[0, 0, 0, 0, 0], [0, 4, 0, 4, 0], [2, 2, 0, 2, 0], [1, 0, 2, 3, 0], [0, 3, 0, 4, 1],
                      [0, 0, 0, 2, 2], [0, -1, 0, -1, 0], [0, 0, 9, 9, 0]], dtype=np.int32)
    got = heal.targets_from_votes(torch.from_numpy(votes).cuda())
    assert got.dtype == torch.int32 and got.is_contiguous()
    assert got.cpu().tolist() == list(HP.targets_from_votes(votes)) == [-1, 1, -1, -1, -1, -1, 1, 2]
