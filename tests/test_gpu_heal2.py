"""Two-block correction on the GPU: every gf_heal2_kernel / gf_heal2_byte_kernel of libecg_heal2.so against the
definition (tests/heal2_plain.py), which tries every block with every error value and looks the rest of the syndrome up
among all multiples of all columns, instead of the kernels' pivot rows, minors and predicted syndromes.

Every case uploads an arena, runs one call and compares THE WHOLE ARENA with the definition's image -- guard bands,
the block the check does not name and the stripes the call does not select included -- the report exactly, and
`counters()` with the declared launches and bytes.

Shapes are the heal's (tests/test_gpu_heal.py, tests/test_gpu_locate.py, whose arena helpers this module uses):
B = 4693 (two full 2 KiB workgroup chunks, a partial third, a 5-byte tail), B = 5 (byte path only), S = 3 strided
stripes with 64-byte bands of 0xC3 around every block and a block the check does not name.  MDS checks are [C | I] with
C a Cauchy matrix (heal2_plain.cauchy), whose k-wise independence heal2_plain.heal2 verifies by plain rank before
every use; stripes that satisfy a check are built with tests/gf_plain.py (or the oracle's encode), never with the
library's own encode.
"""
import json
import os

import numpy as np
import pytest

import gf_kernel_cases as C
import gf_plain
import heal2_plain as P
import test_gpu_locate as TL

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
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
def heal2(ecg):
    import ecg_heal2
    ecg_heal2.lib()
    return ecg_heal2


@pytest.fixture(scope="module")
def heal(ecg):
    import ecg_heal
    ecg_heal.lib()
    return ecg_heal


# ---- one call against the definition

def _expect(img, B, H, src, rows, targets):
    """(arena image after the call, [len(rows)][n + 3] reports) by the definition: heal2_plain over the blocks `src`
    of every stripe in `rows`, target targets[i] for rows[i] (None: ANY2)."""
    want = img.copy()
    reports = []
    for i, s in enumerate(rows):
        out, rep = P.heal2(H, img[s][src, GUARD:GUARD + B], None if targets is None else targets[i])
        want[s][src, GUARD:GUARD + B] = out
        reports.append(rep)
    return want, np.stack(reports)


def _ints(torch, values):
    return None if values is None else torch.tensor([int(v) for v in values], dtype=torch.int32, device="cuda")


def _run(torch, heal2, img, d, B, shift, H, src, call, sel=None, targets=None):
    """Upload img into d, run `call`, compare the report, the whole arena and the counters with the definition.
    Returns (report, expected image), both numpy."""
    H = np.asarray(H, dtype=np.int64)
    n = H.shape[1]
    rows = list(range(img.shape[0])) if sel is None else list(sel)
    assert len(set(rows)) == len(rows)                              # the ids of a call must be distinct
    want, reports = _expect(img, B, H, src, rows, targets)
    d.copy_(torch.from_numpy(img).to(d.device))
    c0 = heal2.counters()
    got = call()
    torch.cuda.synchronize()
    c1 = heal2.counters()
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(rows), n + 3)
    g = got.cpu().numpy().astype(np.int64)
    assert np.array_equal(g, reports), (H.shape, B, shift, sel, targets, g, reports)
    assert (g[:, :n].sum(axis=1) - g[:, n + 2] + g[:, n + 1] == g[:, n]).all()
    after = d.cpu().numpy()
    if not np.array_equal(after, want):
        diff = np.argwhere(after != want)
        raise AssertionError((H.shape, B, shift, sel, targets, len(diff), diff[:8].tolist()))
    vec = (B & ~15) if shift % 16 == 0 else 0
    assert c1["launches"] - c0["launches"] == (vec > 0) + (vec < B)
    assert c1["bytes"] - c0["bytes"] == len(rows) * B * n
    return g, want


def _mds(r, k, seed=0):
    Cm = P.cauchy(r, k, seed)
    return Cm, np.concatenate([Cm, np.eye(r, dtype=np.int64)], axis=1)


def _plant_pairs(stripes, seed):
    """On top of test_gpu_locate._damage (stripe 1: single bytes at the edges in three blocks; stripe 2: blocks 0 and
    n - 1 at one position, a run, a tail byte): pairs of (0, n // 2) next to stripe 1's singles, and a short run of
    pairs of (n // 2, n - 1) in stripe 2.  Works for any block size."""
    S, n, B = stripes.shape
    rng = np.random.default_rng(seed)
    spots = (1, 17, 2046, 2049, B - 2) if B >= 64 else (B - 1,)
    for p in spots:
        stripes[1, 0, p] ^= rng.integers(1, 256, dtype=np.uint8)
        stripes[1, n // 2, p] ^= rng.integers(1, 256, dtype=np.uint8)
    lo = 40 if B >= 64 else 0
    hi = min(lo + 5, B)
    stripes[2, n // 2, lo:hi] ^= rng.integers(1, 256, hi - lo, dtype=np.uint8)
    stripes[2, n - 1, lo:hi] ^= rng.integers(1, 256, hi - lo, dtype=np.uint8)


def _strided_case(torch, heal2, r, k, B, shift=0, sels=(None,)):
    """H = [C | I] over blocks 1.. with C an r x k Cauchy matrix, then the same check with its columns reversed (a
    general H, every column through the tables).  TARGET2 names block 0 for stripe 0, the middle block for stripe 1
    and the last (an identity block of [C | I]) for stripe 2; ANY2 from r = 4."""
    Cm, H = _mds(r, k, seed=100 * r + k)
    stripes = TL._consistent(Cm, S3, B, 1000 * r + 10 * k + B)
    TL._damage(stripes, 7 * r + k)
    _plant_pairs(stripes, 11 * r + k)
    n = k + r
    blocks = np.concatenate([np.full((S3, 1, B), 0x77, np.uint8), stripes], axis=1)   # slot 0 is not named
    img = TL._arena(blocks)
    d = TL._to_dev(torch, img, shift)
    view = d[:, :, GUARD:GUARD + B]
    src = list(range(1, n + 1))
    for Hx, srcx, flip in ((H, src, False), (H[:, ::-1].copy(), src[::-1], True)):
        per_stripe = [0, n // 2, n - 1]
        if flip:
            per_stripe = [n - 1 - t for t in per_stripe]
        for ids in sels:
            rows = list(range(S3)) if ids is None else list(ids)
            for targets in ([per_stripe[s] for s in rows],) + ((None,) if r >= 4 else ()):
                g, _ = _run(torch, heal2, img, d, B, shift, Hx, srcx,
                            lambda: heal2.matrix_batch(Hx, srcx, view, stripe_ids=_ints(torch, ids),
                                                       targets=_ints(torch, targets)), sel=ids, targets=targets)
                assert not g[rows.index(0)].any()                    # the clean stripe's row is all zero
                assert g[rows.index(2), n + 2] > 0                   # pairs were corrected
                if 1 in rows:
                    assert g[rows.index(1), n + 2] > 0 and g[rows.index(1), n + 1] == 0


@gpu
@pytest.mark.parametrize("r", range(3, 9), ids=[f"r{r}" for r in range(3, 9)])
def test_every_r_strided(torch_cuda, heal2, r):
    for k in K_SWEEP:
        _strided_case(torch_cuda, heal2, r, k, B_MAIN)
    _strided_case(torch_cuda, heal2, r, 7, B_BYTES)
    _strided_case(torch_cuda, heal2, r, 3, B_MAIN, sels=([2, 0],))


@gpu
@pytest.mark.parametrize("r", range(3, 9), ids=[f"r{r}" for r in range(3, 9)])
def test_every_r_inline(ecg, torch_cuda, heal2, r):
    """ecg_heal2.ec over RS(k, r)'s own [C | I] check: the INLINE kernels of every R, both paths, TARGET2 (the first
    block, the last identity block) and ANY2 (r >= 4)."""
    torch = torch_cuda
    code = ecg.ec_factory(ecg.ECTYPE.RS, ecg.CodingParameters(k=3 + r % 5, m=r))
    k, n = code.k, code.k + code.m
    H = np.asarray(code.check_matrix(), dtype=np.int64)
    assert np.array_equal(H[:, k:], np.eye(r, dtype=np.int64))
    for B in (B_MAIN, B_BYTES):
        stripes = TL._consistent(H[:, :k], 3, B, 77 * r + B)
        TL._damage(stripes, 5 * r + B)
        _plant_pairs(stripes, 3 * r + B)
        for s in (1, 2):
            img = TL._arena(np.concatenate([np.full((1, 1, B), 0x77, np.uint8), stripes[s:s + 1]], axis=1))
            d = TL._to_dev(torch, img)
            blocks = [d[0, 1 + b, GUARD:GUARD + B] for b in range(n)]
            for target in (0, n - 1) + ((heal2.ANY,) if r >= 4 else ()):
                g, _ = _run(torch, heal2, img, d, B, 0, H, list(range(1, n + 1)),
                            lambda: heal2.ec(code, blocks[:k], blocks[k:], B, target=target),
                            targets=None if target == heal2.ANY else [target])
                assert target != heal2.ANY or B != B_MAIN or g[0, n + 2] > 0


# ---- planted pairs

RS64 = next(c for c in GOLDEN if c["name"] == "RS(6,4)")
RS104 = next(c for c in GOLDEN if c["name"] == "RS(10,4)")


def _code(c, S, B, seed):
    k, m = c["k"], c["m"]
    M = np.asarray(c["matrix"], dtype=np.int64).reshape(m, k)
    return TL._consistent(M, S, B, seed)


def _encode_case(torch, heal2, c, stripes, original=None, sel=None, targets=None, shift=0):
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
    g, want = _run(torch, heal2, img, d, B, shift, H, list(range(1, n + 1)),
                   lambda: heal2.encode_batch(k, m, flat, view, stripe_ids=_ints(torch, sel),
                                              targets=_ints(torch, targets)), sel=sel, targets=targets)
    if original is not None:
        rows = list(range(S)) if sel is None else list(sel)
        assert np.array_equal(want[rows][:, 1:, GUARD:GUARD + B], original[rows])
    return g, want, (img, d, view, flat)


PAIR_KINDS = ((0, 4), (2, 7), (6, 9))   # RS(6,4): (first, middle) table blocks, (table, identity), (identity, identity)


def _pairs_at_the_edges(torch, heal2, shift):
    """Stripe s holds pairs of PAIR_KINDS[s] at the column, chunk and tail edges.  ANY2, then TARGET2 naming either
    block of the stripe's pair, then a block outside it: nothing of the pair is touched."""
    n, B = 10, B_MAIN
    assert B == 4693 and POSITIONS[-2] == (B & ~15) - 1
    original = _code(RS64, S3, B, 64)
    stripes = original.copy()
    rng = np.random.default_rng(64)
    for s, (a, b) in enumerate(PAIR_KINDS):
        for pos in POSITIONS:
            stripes[s, a, pos] ^= rng.integers(1, 256, dtype=np.uint8)
            stripes[s, b, pos] ^= rng.integers(1, 256, dtype=np.uint8)
    want = np.zeros((S3, n + 3), np.int64)
    for s, (a, b) in enumerate(PAIR_KINDS):
        want[s, [a, b, n, n + 2]] = len(POSITIONS)
    for targets in (None, [a for a, _ in PAIR_KINDS], [b for _, b in PAIR_KINDS]):
        g, _, _ = _encode_case(torch, heal2, RS64, stripes, original=original, targets=targets, shift=shift)
        assert np.array_equal(g, want), (targets, g)
    g, after, _ = _encode_case(torch, heal2, RS64, stripes, targets=[1, 1, 1], shift=shift)
    assert np.array_equal(after[:, 1:, GUARD:GUARD + B], stripes) and (g[:, n + 1] == len(POSITIONS)).all()


@gpu
def test_pairs_at_the_edges(torch_cuda, heal2):
    _pairs_at_the_edges(torch_cuda, heal2, 0)


@gpu
def test_unaligned_base_runs_the_byte_kernel(torch_cuda, heal2):
    """The arena shifted by one byte: no block is 16-byte aligned, one byte-kernel launch covers everything (_run
    counts the launches)."""
    _pairs_at_the_edges(torch_cuda, heal2, 1)
    for r, k in ((3, 4), (4, 7), (8, 3)):
        _strided_case(torch_cuda, heal2, r, k, B_MAIN, shift=1, sels=(None, [2, 0]))


@gpu
def test_two_corrections_of_one_column(torch_cuda, heal2):
    """Two different pairs that share a block inside one 16-byte column, and inside one dword: the lane corrects the
    shared block's 16 bytes twice, the second time on top of the first.  Then a pair next to singles in one column.  In
    the vector part, in its last column and in the tail (the byte kernel)."""
    n = 10
    original = _code(RS64, S3, B_MAIN, 71)
    stripes = original.copy()
    stripes[1, [2, 5], 32] ^= np.array([0x01, 0xFE], np.uint8)        # {2, 5} at byte 0 of column 2
    stripes[1, [2, 8], 37] ^= np.array([0x80, 0x7F], np.uint8)        # {2, 8} at byte 5: block 2 twice
    stripes[1, [2, 0], 33] ^= np.array([0x11, 0x22], np.uint8)        # {0, 2} in the dword of byte 32: three times
    stripes[1, [7, 9], 4672 + 1] ^= np.array([3, 4], np.uint8)        # the last full column of the vector part
    stripes[1, [7, 3], 4672 + 2] ^= np.array([5, 6], np.uint8)
    stripes[1, [6, 1], 4688] ^= np.array([7, 8], np.uint8)            # the 5-byte tail
    stripes[1, [6, 4], 4690] ^= np.array([9, 10], np.uint8)
    stripes[2, 3, 2048 + 48] ^= 0x33                                  # a single in block 3 ...
    stripes[2, [3, 8], 2048 + 49] ^= np.array([0x44, 0x55], np.uint8) # ... next to a pair that holds block 3 ...
    stripes[2, 6, 2048 + 50] ^= 0x66                                  # ... and a single elsewhere
    stripes[2, 8, 2048 + 63] ^= 0x77                                  # and one in the pair's other block
    g, _, _ = _encode_case(torch_cuda, heal2, RS64, stripes, original=original)
    assert [int(v) for v in g[1, [2, 5, 8, 0, 7, 9, 3, 6, 1, 4]]] == [3, 1, 1, 1, 2, 1, 1, 2, 1, 1]
    assert [int(v) for v in g[1, n:]] == [7, 0, 7]
    assert [int(v) for v in g[2, [3, 8, 6]]] == [2, 2, 1] and [int(v) for v in g[2, n:]] == [4, 0, 1]
    g, after, _ = _encode_case(torch_cuda, heal2, RS64, stripes, targets=[0, 2, 3])
    assert [int(v) for v in g[1, n:]] == [7, 4, 3] and [int(v) for v in g[2, n:]] == [4, 0, 1]
    assert np.array_equal(after[2, 1:, GUARD:GUARD + B_MAIN], original[2])


# ---- one garbage block plus a run; three blocks at one position

@gpu
@pytest.mark.parametrize("r", (3, 4))
def test_garbage_block_plus_a_run(torch_cuda, heal2, r):
    """TARGET2: block g is garbage and named, another block has a run inside it.  With the wrong block named the
    single-block positions still come back, the overlap is what the definition says (r = 4: untouched and counted)."""
    torch = torch_cuda
    k, B = 6, B_MAIN
    n = k + r
    Cm, H = _mds(r, k, seed=40 + r)
    original = TL._consistent(Cm, S3, B, 400 + r)
    stripes = original.copy()
    rng = np.random.default_rng(41 + r)
    plan = ((1, 2, n - 1, 1900, 2300), (2, n - 2, 0, B - 300, B))         # stripe, garbage, run block, run
    for s, gb, rb, lo, hi in plan:
        stripes[s, gb] = rng.integers(0, 256, B, dtype=np.uint8)
        stripes[s, rb, lo:hi] ^= rng.integers(1, 256, hi - lo, dtype=np.uint8)
    img = TL._arena(np.concatenate([np.full((S3, 1, B), 0x77, np.uint8), stripes], axis=1))
    d = TL._to_dev(torch, img)
    view = d[:, :, GUARD:GUARD + B]
    src = list(range(1, n + 1))
    targets = [0, 2, n - 2]
    g, after = _run(torch, heal2, img, d, B, 0, H, src,
                    lambda: heal2.matrix_batch(H, src, view, targets=_ints(torch, targets)), targets=targets)
    assert np.array_equal(after[:, 1:, GUARD:GUARD + B], original)
    for s, gb, rb, lo, hi in plan:
        overlap = np.count_nonzero(stripes[s, gb, lo:hi] != original[s, gb, lo:hi])
        assert g[s, n + 2] == overlap > 250 and g[s, rb] == hi - lo and g[s, n + 1] == 0
    wrong = [0, 3, 1]
    g, after = _run(torch, heal2, img, d, B, 0, H, src,
                    lambda: heal2.matrix_batch(H, src, view, targets=_ints(torch, wrong)), targets=wrong)
    if r == 4:
        for s, gb, rb, lo, hi in plan:
            overlap = np.count_nonzero(stripes[s, gb, lo:hi] != original[s, gb, lo:hi])
            assert g[s, n + 1] == overlap and g[s, n + 2] == 0
            fixed = original[s].copy()
            fixed[[gb, rb], lo:hi] = stripes[s][[gb, rb], lo:hi]
            both = (stripes[s, gb, lo:hi] != original[s, gb, lo:hi])
            fixed[rb, lo:hi][~both] = original[s, rb, lo:hi][~both]
            assert np.array_equal(after[s, 1:, GUARD:GUARD + B], fixed)


@gpu
def test_three_blocks_at_one_position_with_r5(torch_cuda, heal2):
    torch = torch_cuda
    r, k, B = 5, 6, B_MAIN
    n = k + r
    Cm, H = _mds(r, k, seed=50)
    original = TL._consistent(Cm, S3, B, 500)
    stripes = original.copy()
    for i, pos in enumerate((5, 2047, 2048, 4687, 4690)):
        stripes[1, [1, 4, n - 1], pos] ^= np.array([0x5A, 0xC3, 1 + i], np.uint8)
    stripes[1, [0, 9], 100] ^= np.array([1, 2], np.uint8)                  # and one pair that does come back
    img = TL._arena(np.concatenate([np.full((S3, 1, B), 0x77, np.uint8), stripes], axis=1))
    d = TL._to_dev(torch, img)
    view = d[:, :, GUARD:GUARD + B]
    src = list(range(1, n + 1))
    g, after = _run(torch, heal2, img, d, B, 0, H, src, lambda: heal2.matrix_batch(H, src, view))
    assert [int(v) for v in g[1, n:]] == [6, 5, 1] and g[1, :n].sum() == 2
    for targets in ([0, 4, 0], [0, 0, 0]):
        g, _ = _run(torch, heal2, img, d, B, 0, H, src,
                    lambda: heal2.matrix_batch(H, src, view, targets=_ints(torch, targets)), targets=targets)
        assert g[1, n + 1] == (6 if targets[1] == 4 else 5)


# ---- targets, idempotence, the heal's behaviour, batch scope

@gpu
def test_out_of_range_targets(torch_cuda, heal2):
    original = _code(RS64, S3, B_MAIN, 75)
    stripes = original.copy()
    TL._damage(stripes, 75)
    _plant_pairs(stripes, 75)
    stripes[0, 4, 10:50] ^= 0x3C                                     # stripe 0 too
    n = 10
    for targets in ([-1, n, -7], [n + 100, -(1 << 31), (1 << 31) - 1]):
        g, after, _ = _encode_case(torch_cuda, heal2, RS64, stripes, targets=targets)
        assert np.array_equal(after[:, 1:, GUARD:GUARD + B_MAIN], stripes)          # bit-identical
        assert not g[:, :n].any() and (g[:, n] > 0).all() and np.array_equal(g[:, n + 1], g[:, n])
        assert not g[:, n + 2].any()


@gpu
def test_idempotence_and_report_overwritten(torch_cuda, heal2):
    torch = torch_cuda
    original = _code(RS64, S3, B_MAIN, 79)
    stripes = original.copy()
    stripes[1, 2, 100:2300] ^= 0x42
    stripes[1, 7, 2000:2100] ^= 0x24
    stripes[2, 9, B_MAIN - 3:] ^= 0x17
    stripes[2, 0, B_MAIN - 2:] ^= 0x71
    g, want, (img, d, view, flat) = _encode_case(torch, heal2, RS64, stripes, original=original)
    assert g[1, 2] == 2200 and g[1, 7] == 100 and g[1, 12] == 100 and g[2, 9] == 3 and g[2, 12] == 2
    out = torch.full((S3, 13), -1, dtype=torch.int32, device="cuda")     # 0xFFFFFFFF
    assert heal2.encode_batch(6, 4, flat, view, out=out) is out
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()                                   # a second call reports all zeros
    assert np.array_equal(d.cpu().numpy(), want)                         # and leaves the arena unchanged


@gpu
def test_singles_only_is_the_heal(torch_cuda, heal, heal2):
    """Where no position needs a pair, the bytes and the first n + 2 counters are ecg_heal's ANY result on a copy."""
    torch = torch_cuda
    n = 14
    original = _code(RS104, S3, B_MAIN, 72)
    stripes = original.copy()
    rng = np.random.default_rng(72)
    for b, lo in zip((0, 2, 5, 9, 11, 13), (0, 700, 2040, 2900, 4000, B_MAIN - 30)):
        stripes[1, b, lo:lo + 30] ^= rng.integers(1, 256, 30, dtype=np.uint8)
        stripes[2, b, lo + 40:lo + 45] ^= rng.integers(1, 256, 5, dtype=np.uint8) if lo + 45 <= B_MAIN else 0
    g2, want, (img, d, view, flat) = _encode_case(torch, heal2, RS104, stripes, original=original)
    assert not g2[:, n + 2].any() and g2[1, n] == 180
    d.copy_(torch.from_numpy(img).to(d.device))
    g1 = heal.encode_batch(10, 4, flat, view).cpu().numpy().astype(np.int64)
    assert np.array_equal(g1, g2[:, :n + 2])
    assert np.array_equal(d.cpu().numpy(), want)


@gpu
def test_heal2_flushes_the_batch_scope(ecg, torch_cuda, heal2):
    """A dev_matrix_encode recorded in a batch scope, then a heal2 of the same blocks inside the scope: the call
    flushes the scope first, so it sees the encode's parity (nothing to correct), not the stale one."""
    torch = torch_cuda
    k, m, B = 6, 4, B_MAIN
    flat = [int(v) for v in RS64["matrix"]]
    stripes = _code(RS64, 1, B, 80)
    want = stripes.copy()
    stripes[0, k:] = 0xA5  # stale
    d = torch.from_numpy(stripes).cuda()
    with ecg.batch():
        ecg.dev_matrix_encode(k, m, flat, [d[0, j] for j in range(k)], [d[0, k + j] for j in range(m)], B)
        report = heal2.encode_batch(k, m, flat, d)
    torch.cuda.synchronize()
    assert not report.cpu().numpy().any()
    assert np.array_equal(d.cpu().numpy(), want)


# ---- the wide check: n = 32, r = 8: 496 pairs, n + 3 = 35 counters

@gpu
def test_wide_check(torch_cuda, heal2):
    """Every block damaged alone somewhere, pairs over the first, middle and last blocks, and four blocks at one
    position (untouched): counters in every part of the first register and report[n .. n + 2] are all hit.  ANY2 and
    TARGET2, [C | I] and reversed."""
    torch = torch_cuda
    n, r, B = 32, 8, B_MAIN
    Cm, H = _mds(r, n - r, seed=32)
    original = TL._consistent(Cm, S3, B, 3200)
    stripes = original.copy()
    rng = np.random.default_rng(32)
    for b in range(n):
        stripes[1, b, 64 + 3 * b] ^= rng.integers(1, 256, dtype=np.uint8)         # inside one wave
        stripes[2, b, (149 * b) % B] ^= rng.integers(1, 256, dtype=np.uint8)      # all over
    pairs = ((0, 31), (0, 1), (15, 16), (30, 31), (7, 24), (23, 24))
    for i, (a, b) in enumerate(pairs):
        for s, pos in ((1, 1024 + 5 * i), (2, (2047, 2048, 4687, 4688, 4692, 16)[i])):
            stripes[s, [a, b], pos] ^= rng.integers(1, 256, 2, dtype=np.uint8)
    stripes[2, [3, 9, 20, 29], 3000] ^= np.array([1, 2, 3, 4], np.uint8)
    img = TL._arena(np.concatenate([np.full((S3, 1, B), 0x77, np.uint8), stripes], axis=1))
    d = TL._to_dev(torch, img)
    view = d[:, :, GUARD:GUARD + B]
    src = list(range(1, n + 1))
    g, after = _run(torch, heal2, img, d, B, 0, H, src, lambda: heal2.matrix_batch(H, src, view))
    assert not g[0].any() and (g[1:, :n] > 0).all()
    assert [int(v) for v in g[1, n:]] == [38, 0, 6] and [int(v) for v in g[2, n:]] == [39, 1, 6]
    assert np.array_equal(after[:2, 1:, GUARD:GUARD + B], original[:2])
    Hr, srcr = H[:, ::-1].copy(), src[::-1]
    gr, _ = _run(torch, heal2, img, d, B, 0, Hr, srcr, lambda: heal2.matrix_batch(Hr, srcr, view))
    assert np.array_equal(gr[:, :n], g[:, n - 1::-1][:, :n]) and np.array_equal(gr[:, n:], g[:, n:])
    targets = [0, 31, 24]
    gt, _ = _run(torch, heal2, img, d, B, 0, H, src,
                 lambda: heal2.matrix_batch(H, src, view, targets=_ints(torch, targets)), targets=targets)
    assert [int(v) for v in gt[1, n:]] == [38, 4, 2] and [int(v) for v in gt[2, n:]] == [39, 5, 2]


@gpu
def test_n_33_is_refused(ecg, torch_cuda, heal2):
    """RS(25, 8) has n = 33 > 32: ECG_EINVAL from both forms, nothing launched, nothing written."""
    torch = torch_cuda
    k, m = 25, 8
    code = ecg.ec_factory(ecg.ECTYPE.RS, ecg.CodingParameters(k=k, m=m))
    d = torch.full((2, k + m, 64), 0x5A, dtype=torch.uint8, device="cuda")
    l0 = heal2.counters()["launches"]
    with pytest.raises(ecg.EcgError) as e:
        heal2.ec(code, [d[0, j] for j in range(k)], [d[0, k + j] for j in range(m)], 64)
    assert e.value.code == ecg.ECG_EINVAL and b"n = 33" in ecg.lib().ecg_last_error()
    with pytest.raises(ecg.EcgError) as e:
        heal2.ec_batch(code, d, targets=_ints(torch, [0, 1]))
    assert e.value.code == ecg.ECG_EINVAL
    assert heal2.counters()["launches"] == l0 and bool((d == 0x5A).all())


# ---- scrub -> dirty -> heal2 -> re-scrub

@gpu
def test_end_to_end(ecg, oracle, torch_cuda, heal2):
    """RS(10,4) stripes as the oracle encoded them; two blocks damaged at overlapping runs (and a third elsewhere):
    scrub -> dirty -> heal2 in ANY2 -> re-scrub clean, and the bytes are the originals."""
    import ecg_locate
    import ecg_scrub
    from oracle import ec_ref as E
    torch = torch_cuda
    c = RS104
    k, m, S, B = 10, 4, 8, B_MAIN
    ref = E.ec_factory(c["type"], E.CodingParameters(**c["params"]))
    code = ecg.ec_factory(c["type"], ecg.CodingParameters(**c["params"]))
    rng = np.random.default_rng(104)
    original = np.zeros((S, k + m, B), np.uint8)
    for s in range(S):
        data = [rng.integers(0, 256, B, dtype=np.uint8) for _ in range(k)]
        coding = E.zeros(m, B)
        ref.encode(data, coding, B)
        original[s] = np.stack(data + list(coding))
    damaged = original.copy()
    damaged[2, 3, 100:2300] = rng.integers(0, 256, 2200, dtype=np.uint8)      # a data block, across a chunk edge
    damaged[2, 12, 2000:2500] ^= rng.integers(1, 256, 500, dtype=np.uint8)    # a parity block, overlapping it
    damaged[5, 7, B - 40:] ^= 0x3C                                            # into the tail ...
    damaged[5, 0, B - 20:] ^= 0xC3                                            # ... with another block on top
    damaged[6, 1, 300:310] ^= 0x55
    d = torch.from_numpy(damaged).cuda()
    sel = ecg_locate.dirty(ecg_scrub.ec_batch(code, d))
    assert sel.cpu().tolist() == [2, 5, 6]
    report = heal2.ec_batch(code, d, stripe_ids=sel).cpu().numpy()
    assert report[0, 16] > 250 and report[1, 16] == 20 and report[2, 16] == 0 and not report[:, 15].any()
    assert np.array_equal(d.cpu().numpy(), original)
    again = ecg_scrub.ec_batch(code, d)
    assert not again.cpu().numpy().any() and ecg_locate.dirty(again).numel() == 0
