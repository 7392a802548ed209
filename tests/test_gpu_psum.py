"""Piece checksums on the GPU: every crc_psum_small / crc_psum_rows / crc_psum_byte kernel of libecg_psum.so and the
verify's compare against the definition (tests/crc32c_plain.py, which shares no table with the product), and the
bridge from a piece verify to the heal.

Every case uploads an arena -- blocks inside 64-byte bands of 0xC3, a pitch with a gap, slots the call does not name --
runs one call, compares ALL its sums with the definition, the whole arena with its image before the call, `counters()`
with the declared launches and bytes, and `last_launch()` with the geometry the case is meant to reach: a case that
fell back to the byte path fails.

The blocks of a case hold distinct random bytes (stripes 0..2); further stripes hold the blocks that isolate one term
each: all 0x00 and all 0xFF (the affine terms) and ONE-HOT blocks, a single nonzero byte at the first and last byte of
every piece of every piece size, of every 2 KiB row, and of the tail (one position multiplier each).  The reference
of a (block size, piece size) is computed once and shared.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import crc32c_plain as CP

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
GUARD, BAND = 64, 0xC3
ROW, AUTO_SPAN = 2048, 256 << 10                        # psum_kernels.hpp kPsumRowBytes, kPsumAutoSpan
BYTE_RUN, BYTE_WG = 64, 64 * 128                        # byte path: bytes per lane, per workgroup
SLOTS, SRC = 7, [5, 0, 3, 6, 2]                         # n = 5 of a stripe's 7 slots, permuted
SIZES = (1, 15, 16, 17, 511, 512, 513, 2047, 2048, 2049, 4096, 6165, 8192 + 16 + 5, 12288 + 53)
PIECES = (512, 1024, 2048, 4096, 8192)
SPANS = (0, 2048, 4096)
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return torch


@pytest.fixture(scope="module")
def psum(ecg):
    import ecg_psum
    ecg_psum.lib()
    yield ecg_psum
    ecg_psum.set_span_bytes(0)


@pytest.fixture(scope="module")
def sums(ecg):
    import ecg_sum
    ecg_sum.lib()
    return ecg_sum


@pytest.fixture(scope="module")
def heal(ecg):
    import ecg_heal
    ecg_heal.lib()
    return ecg_heal


@pytest.fixture(scope="module")
def heal2(ecg):
    import ecg_heal2
    ecg_heal2.lib()
    return ecg_heal2


# ---- blocks, references, arenas, geometry

def _one_hot_positions(B):
    vec = B & ~15
    pos = {0, 3, 4, 15, 16, B - 1, vec, vec - 1, vec - 16}
    for step in (512, 1024, ROW):                        # every piece size and span is a multiple of one of these
        for g in range(0, B // step + 2):
            pos |= {g * step, g * step - 1}
    return sorted(p for p in pos if 0 <= p < B)


@functools.lru_cache(maxsize=None)
def _blocks(B):
    """(blocks [S][SLOTS][B], the selection): three stripes of distinct random bytes, then the stripes that hold the
    special blocks in the summed slots.  Read-only: shared by every case of B."""
    rng = np.random.default_rng(2000 + B)
    special = [np.zeros(B, np.uint8), np.full(B, 0xFF, np.uint8)]
    for i, p in enumerate(_one_hot_positions(B)):
        blk = np.zeros(B, np.uint8)
        blk[p] = (37 * i) % 255 + 1
        special.append(blk)
    S = 3 + -(-len(special) // len(SRC))
    blocks = rng.integers(0, 256, (S, SLOTS, B), dtype=np.uint8)
    for i, blk in enumerate(special):
        blocks[3 + i // len(SRC), SRC[i % len(SRC)]] = blk
    perm = [int(v) for v in rng.permutation(S)]
    sel = perm + [perm[1]]                               # scrambled, one stripe twice
    blocks.setflags(write=False)
    return blocks, sel


def _piece_sums(blocks, P):
    """crc32c of every piece of every block by the definition: [..., B] -> [..., Q] uint32.  One walk of `many` over
    all pieces at a time; `lengths` gives the ragged last piece."""
    blocks = np.asarray(blocks, dtype=np.uint8)
    B = blocks.shape[-1]
    Q = -(-B // P)
    width = min(P, B)
    padded = np.zeros(blocks.shape[:-1] + (Q * width,), np.uint8)
    padded[..., :B] = blocks
    rows = padded.reshape(blocks.shape[:-1] + (Q, width))
    lengths = np.full(rows.shape[:-1], width)
    lengths[..., Q - 1] = B - (Q - 1) * width
    return CP.many(rows, lengths if B % width else None).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _want(B, P):
    want = _piece_sums(_blocks(B)[0], P)
    want.setflags(write=False)
    return want


def _arena(blocks, pitch=None):
    """[S][slots][pitch] host image of [S][slots][B] block bytes inside bands of 0xC3; the default pitch keeps every
    block 16-byte aligned and leaves a 48-byte gap."""
    S, slots, B = blocks.shape
    pitch = pitch or ((GUARD + B + GUARD + 15) & ~15) + 48
    img = np.full((S, slots, pitch), BAND, np.uint8)
    img[:, :, GUARD:GUARD + B] = blocks
    return img


def _to_dev(torch, img, shift=0):
    flat = torch.empty(img.size + 16, dtype=torch.uint8, device="cuda")
    view = flat[shift:shift + img.size]
    view.copy_(torch.from_numpy(img.reshape(-1)))
    return view.view(img.shape)


def _geometry(B, P, span, aligned, blocks):
    """The launch the library is meant to choose (include/ecg_psum.h ecg_psum_last_launch), restated."""
    vec = (B & ~15) if aligned else 0
    geo = dict(piece_bytes=P, pieces_per_block=-(-B // P), blocks=blocks)
    if vec:
        return dict(geo, path=0, span_bytes=min(span or AUTO_SPAN, -(-vec // ROW) * ROW))
    return dict(geo, path=1, span_bytes=min(BYTE_WG, -(-B // BYTE_RUN) * BYTE_RUN))


def _regime(B, P, span):
    """What the vector launch of an aligned block meets (the issue's table), restated: a set of words."""
    vec = B & ~15
    out = set()
    if vec:
        sb = _geometry(B, P, span, True, 1)["span_bytes"]
        longest = min(P, -(-vec // ROW) * ROW)           # the rows of the longest piece
        out.add("a" if P < ROW else "b" if longest <= sb else "c")
        if P >= ROW and vec > sb:
            out.add("workgroups per piece: %d" % -(-longest // sb))
    else:
        out.add("byte only")
    if B % P:
        out.add("ragged")
    if vec and B % 16 and (B - 1) // P * P == vec:
        out.add("all-tail last piece")
    if B < P:
        out.add("B < P")
    return out


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _ints(torch, values):
    return None if values is None else torch.tensor([int(v) for v in values], dtype=torch.int32, device="cuda")


def _check_call(torch, psum, d, img, B, P, span, aligned, n_blocks, call, want, launches=None):
    """Run `call` with the span forced to `span`; compare all sums, the arena, the counters and the geometry."""
    psum.set_span_bytes(span)
    c0 = psum.counters()
    got = call()
    torch.cuda.synchronize()
    c1 = psum.counters()
    assert got.dtype == torch.int32 and tuple(got.shape) == want.shape, (tuple(got.shape), want.shape)
    g = _u32(got)
    if not np.array_equal(g, want):
        diff = np.argwhere(g != want)
        first = tuple(diff[0])
        raise AssertionError((B, P, span, aligned, len(diff), diff[:8].tolist(), hex(int(g[first])),
                              hex(int(want[first]))))
    assert np.array_equal(d.cpu().numpy(), img), (B, P, span, "the arena changed")
    vec = (B & ~15) if aligned else 0
    assert c1["launches"] - c0["launches"] == ((vec > 0) + (vec < B) if launches is None else launches)
    assert c1["bytes"] - c0["bytes"] == n_blocks * B
    last = psum.last_launch()
    assert last == _geometry(B, P, span, aligned, n_blocks), (B, P, span, aligned, last)
    return g


def _strided(torch, psum, B, pieces, spans, shift=0, pitch=None):
    blocks, sel = _blocks(B)
    img = _arena(blocks, pitch)
    d = _to_dev(torch, img, shift)
    view = d[:, :, GUARD:GUARD + B]
    aligned = shift % 16 == 0 and img.shape[2] % 16 == 0
    ids = _ints(torch, sel)
    for P in pieces:
        want = _want(B, P)[sel][:, SRC]
        for span in spans:
            _check_call(torch, psum, d, img, B, P, span, aligned, len(sel) * len(SRC),
                        lambda: psum.pieces_batch(SRC, view, P, stripe_ids=ids), want)


# ---- every size at which a part of the kernels can go wrong

def test_the_sizes_reach_every_regime():
    """No library call: the restated geometry alone, so that the lists above are seen to reach every case."""
    reach = {(B, P, span): _regime(B, P, span) for B in SIZES for P in PIECES for span in SPANS}
    every = set().union(*reach.values())
    assert every >= {"byte only", "a", "b", "c", "workgroups per piece: 1", "workgroups per piece: 2",
                     "workgroups per piece: 4", "ragged", "all-tail last piece", "B < P"}, every
    assert reach[1, 512, 0] == {"byte only", "ragged", "B < P"}
    assert reach[513, 512, 0] == {"a", "ragged", "all-tail last piece"}
    assert reach[2049, 2048, 2048] == {"b", "ragged", "all-tail last piece"}
    assert reach[12341, 2048, 4096] == {"b", "ragged", "workgroups per piece: 1"}      # two pieces per workgroup
    assert reach[12341, 4096, 2048] == {"c", "ragged", "workgroups per piece: 2"}
    assert reach[8213, 8192, 2048] == {"c", "ragged", "workgroups per piece: 4"}
    assert reach[12341, 8192, 4096] == {"c", "ragged", "workgroups per piece: 2"}
    assert reach[6165, 512, 0] == {"a", "ragged"} and reach[6165, 1024, 4096] == {"a", "ragged"}
    assert reach[4096, 4096, 0] == {"b"} and reach[4096, 8192, 0] == {"b", "ragged", "B < P"}
    assert max(len(_one_hot_positions(B)) for B in SIZES) <= 64


def test_the_reference_of_the_pieces_is_the_definition():
    """`_piece_sums` against `bitwise` over the slices themselves."""
    rng = np.random.default_rng(9)
    blocks = rng.integers(0, 256, (2, 1300), dtype=np.uint8)
    got = _piece_sums(blocks, 512)
    assert got.shape == (2, 3)
    for s in range(2):
        for q in range(3):
            assert int(got[s, q]) == CP.bitwise(blocks[s, 512 * q:512 * (q + 1)].tobytes())
    assert int(_piece_sums(blocks[0, :7], 512)[0]) == CP.bitwise(blocks[0, :7].tobytes())
    assert np.array_equal(_piece_sums(blocks[:, :1024], 512)[:, 1], CP.many(blocks[:, 512:1024]))


@gpu
@pytest.mark.parametrize("B", SIZES)
def test_every_size_piece_and_span(torch_cuda, psum, B):
    _strided(torch_cuda, psum, B, PIECES, SPANS)


@gpu
@pytest.mark.parametrize("B", (17, 2049, 12288 + 53))
def test_unaligned_base_and_stride_run_the_byte_kernel(torch_cuda, psum, B):
    """base + 1 and a block stride of 2049 + B: one byte-kernel launch covers everything (12288 + 53: two workgroups
    per block, pieces that end inside either)."""
    _strided(torch_cuda, psum, B, (512, 4096), (2048,), shift=1, pitch=2049 + B)
    last = psum.last_launch()
    assert last["path"] == 1 and last["span_bytes"] == min(BYTE_WG, -(-B // BYTE_RUN) * BYTE_RUN)
    assert -(-B // last["span_bytes"]) == (2 if B > BYTE_WG else 1)


@gpu
def test_all_stripes_in_order_and_an_out_tensor(torch_cuda, psum):
    """stripe_ids None; `out` prefilled with a pattern: the call zeroes it before it XORs into it."""
    torch = torch_cuda
    B, P = 6165, 1024
    blocks, _ = _blocks(B)
    img = _arena(blocks)
    d = _to_dev(torch, img)
    view = d[:, :, GUARD:GUARD + B]
    out = torch.full((blocks.shape[0], len(SRC), 7), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    got = _check_call(torch, psum, d, img, B, P, 2048, True, blocks.shape[0] * len(SRC),
                      lambda: psum.pieces_batch(SRC, view, P, out=out), _want(B, P)[:, SRC])
    assert np.array_equal(_u32(out), got)


@gpu
def test_more_columns_than_one_launch_holds(torch_cuda, psum):
    """n = 300 block ids, more than the 256 a launch carries in its arguments: two vector and two byte launches."""
    torch = torch_cuda
    B, n = 2048 + 16 + 3, 300
    rng = np.random.default_rng(300)
    blocks = rng.integers(0, 256, (2, n, B), dtype=np.uint8)
    img = _arena(blocks)
    d = _to_dev(torch, img)
    view = d[:, :, GUARD:GUARD + B]
    src = [int(v) for v in rng.permutation(n)]
    for P in (512, 2048):
        _check_call(torch, psum, d, img, B, P, 2048, True, 2 * n, lambda: psum.pieces_batch(src, view, P),
                    _piece_sums(blocks, P)[:, src], launches=4)


# ---- large blocks at the auto span, and the block sums

@gpu
@pytest.mark.parametrize("P", (64 << 10, 1 << 20), ids=["64KiB", "1MiB"])
def test_large_blocks_with_the_auto_span(ecg, torch_cuda, psum, sums, P):
    """B = 2^20 + 53 against ecg_sum_crc32c of the pieces copied back (tests/test_sum_host.py pins it on the
    definition, which would walk this size for seconds per block).  At the auto span a 64 KiB piece is a quarter of a
    workgroup's span and a 1 MiB piece lies over four workgroups."""
    torch = torch_cuda
    S, n, B = 2, 3, (1 << 20) + 53
    full = torch.empty((S, n, (B + 15) & ~15), dtype=torch.uint8, device="cuda")
    ecg.fill_random(full, 0xB10C + n)
    view = full[:, :, :B]
    psum.set_span_bytes(0)
    c0 = psum.counters()
    got = psum.pieces_batch(list(range(n)), view, P)
    torch.cuda.synchronize()
    c1 = psum.counters()
    host = view.cpu().numpy()
    Q = -(-B // P)
    want = np.array([[[sums.crc32c(host[s, j, q * P:(q + 1) * P]) for q in range(Q)] for j in range(n)]
                     for s in range(S)], dtype=np.uint32)
    assert np.array_equal(_u32(got), want), (np.argwhere(_u32(got) != want)[:8].tolist())
    assert len(set(int(v) for v in want.ravel())) == S * n * Q
    assert c1["launches"] - c0["launches"] == 2 and c1["bytes"] - c0["bytes"] == S * n * B
    geo = _geometry(B, P, 0, True, S * n)
    assert geo["span_bytes"] == AUTO_SPAN and psum.last_launch() == geo
    block_sums = _u32(sums.blocks_batch(list(range(n)), view))
    for s in range(S):
        for j in range(n):
            assert psum.fold(_u32(got)[s, j], P, B) == int(block_sums[s, j])
    assert np.array_equal(view.cpu().numpy(), host)


@gpu
@pytest.mark.parametrize("B,P", [(12288 + 53, 512), (12288 + 53, 4096), (513, 512), (2048, 2048)])
def test_fold_of_the_piece_sums_is_the_block_sum(torch_cuda, psum, sums, B, P):
    torch = torch_cuda
    blocks, _ = _blocks(B)
    view = _to_dev(torch, _arena(blocks))[:, :, GUARD:GUARD + B]
    psum.set_span_bytes(2048)
    got = _u32(psum.pieces_batch(SRC, view, P))
    whole = _u32(sums.blocks_batch(SRC, view))
    assert np.array_equal(whole, CP.many(blocks[:, SRC]))
    for s in range(blocks.shape[0]):
        for j in range(len(SRC)):
            assert psum.fold(got[s, j], P, B) == int(whole[s, j]), (s, j)


# ---- the handle's forms, the batch scope

RS64 = next(c for c in GOLDEN if c["name"] == "RS(6,4)")
RS104 = next(c for c in GOLDEN if c["name"] == "RS(10,4)")
RS81 = next(c for c in GOLDEN if c["name"] == "RS(8,1)")


@gpu
def test_inline_through_ec_and_ec_batch(ecg, torch_cuda, psum):
    """RS(6,4) at B = 4096 + 21: ecg_psum.ec over the ten block pointers of one stripe (INLINE), aligned and shifted
    by one byte, at a piece size of either vector kernel; ec_batch over the stripes of the same handle with a
    selection."""
    torch = torch_cuda
    code = ecg.ec_factory(RS64["type"], ecg.CodingParameters(**RS64["params"]))
    k, n, B = code.k, code.k + code.m, 4096 + 21
    assert (k, n) == (6, 10)
    rng = np.random.default_rng(64)
    blocks = rng.integers(0, 256, (3, n, B), dtype=np.uint8)
    img = _arena(blocks)
    for P in (512, 2048):
        want = _piece_sums(blocks, P)
        for shift in (0, 1):
            d = _to_dev(torch, img, shift)
            for s in (0, 2):
                ptrs = [d[s, b, GUARD:GUARD + B] for b in range(n)]
                _check_call(torch, psum, d, img, B, P, 2048, shift == 0, n,
                            lambda: psum.ec(code, ptrs[:k], ptrs[k:], B, P), want[s:s + 1])
        d = _to_dev(torch, img)
        view = d[:, :, GUARD:GUARD + B]
        _check_call(torch, psum, d, img, B, P, 4096, True, 3 * n, lambda: psum.ec_batch(code, view, P), want)
        _check_call(torch, psum, d, img, B, P, 0, True, 2 * n,
                    lambda: psum.ec_batch(code, view, P, stripe_ids=_ints(torch, [2, 0])), want[[2, 0]])


@gpu
def test_psum_flushes_the_batch_scope(ecg, oracle, torch_cuda, psum):
    """A dev_matrix_encode recorded in a batch scope, then the piece sums of the same blocks inside the scope: the call
    flushes the scope first, so it sees the encode's parity, not the stale one."""
    torch = torch_cuda
    k, m, B, P = 6, 4, 4096 + 16, 1024
    M = [int(v) for v in RS64["matrix"]]
    rng = np.random.default_rng(65)
    data = [rng.integers(0, 256, B, dtype=np.uint8) for _ in range(k)]
    coding = [np.zeros(B, np.uint8) for _ in range(m)]
    oracle.jerasure_matrix_encode(k, m, M, data, coding, B)
    want = _piece_sums(np.stack(data + coding), P)
    stale = np.stack(data + [np.full(B, 0xA5, np.uint8)] * m)[None]
    assert not (_piece_sums(stale[0], P)[k:] == want[k:]).any()
    d = torch.from_numpy(stale).cuda()
    with ecg.batch():
        ecg.dev_matrix_encode(k, m, M, [d[0, j] for j in range(k)], [d[0, k + j] for j in range(m)], B)
        got = psum.pieces_batch(list(range(k + m)), d, P)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(got)[0], want)


# ---- verify, and the chain that block sums cannot start

def _encoded(oracle, c, S, B, seed):
    """[S][k + m][B] stripes of code c as the oracle encodes them, and the flat matrix."""
    k, m = c["k"], c["m"]
    M = [int(v) for v in c["matrix"]]
    rng = np.random.default_rng(seed)
    out = np.zeros((S, k + m, B), np.uint8)
    for s in range(S):
        data = [rng.integers(0, 256, B, dtype=np.uint8) for _ in range(k)]
        coding = [np.zeros(B, np.uint8) for _ in range(m)]
        oracle.jerasure_matrix_encode(k, m, M, data, coding, B)
        out[s] = np.stack(data + coding)
    return out, M


def _upload(torch, stripes, pitch=None):
    """A [S][n][B] view of a [S][n][pitch] tensor (default: B rounded up to 16) filled with 0xEE, holding `stripes`."""
    S, n, B = stripes.shape
    full = torch.full((S, n, pitch or (B + 15) & ~15), 0xEE, dtype=torch.uint8, device="cuda")
    view = full[:, :, :B]
    view.copy_(torch.from_numpy(stripes))
    return full, view


def _verdicts(original, damaged, P, sel, n_cols=None):
    """targets and bad as the definition gives them, from where the bytes differ."""
    n = original.shape[1] if n_cols is None else n_cols
    B = original.shape[2]
    Q = -(-B // P)
    targets = np.full((len(sel), Q), -1, np.int64)
    bad = np.zeros((len(sel), Q), np.int64)
    for i, s in enumerate(sel):
        for q in range(Q):
            cols = [j for j in range(n) if (original[s, j, q * P:(q + 1) * P] != damaged[s, j, q * P:(q + 1) * P]).any()]
            bad[i, q] = len(cols)
            targets[i, q] = -1 if not cols else cols[0] if len(cols) == 1 else n
    return targets, bad


def _verify(torch, psum, view, P, recorded, sel, src=None):
    n = view.shape[1] if src is None else len(src)
    src = list(range(n)) if src is None else src
    expected = recorded[torch.tensor(sel, device="cuda").long()][:, :n].contiguous()
    c0 = psum.counters()
    got, targets, bad = psum.verify_batch(src, view, P, expected, stripe_ids=_ints(torch, sel))
    torch.cuda.synchronize()
    B = view.shape[2]
    assert psum.counters()["launches"] - c0["launches"] == 2 + (B % 16 != 0)     # the vector part, the tail, the compare
    assert psum.last_launch()["path"] == 0
    Q = -(-B // P)
    assert targets.dtype == torch.int32 and bad.dtype == torch.int32 and targets.is_contiguous()
    assert tuple(targets.shape) == (len(sel), Q) and tuple(bad.shape) == (len(sel), Q)
    host = view.cpu().numpy()
    assert np.array_equal(_u32(got), _piece_sums(host[sel][:, src], P))          # the computed sums, every one
    return targets, targets.cpu().numpy().astype(np.int64), bad.cpu().numpy().astype(np.int64)


@gpu
def test_verify_names_the_block_of_every_piece_row(ecg, oracle, torch_cuda, psum):
    """S = 6 stripes of RS(10,4), B = 4 * 2048 + 53, P = 2048: five piece rows per stripe, the last one 53 bytes.
    Damage is planted so that piece rows show -1, a block, and n; targets and bad over a scrambled selection with a
    duplicate, through both verify forms."""
    torch = torch_cuda
    S, B, P = 6, 4 * 2048 + 53, 2048
    n = 14
    original, _ = _encoded(oracle, RS104, S, B, 104)
    _, view = _upload(torch, original)
    psum.set_span_bytes(4096)
    recorded = psum.pieces_batch(list(range(n)), view, P)
    assert np.array_equal(_u32(recorded), _piece_sums(original, P))
    sel = [4, 1, 0, 3, 5, 1]
    _, targets, bad = _verify(torch, psum, view, P, recorded, sel)
    assert (targets == -1).all() and (bad == 0).all()

    damaged = original.copy()
    rng = np.random.default_rng(11)
    damaged[1, 3, 100:2300] ^= rng.integers(1, 256, 2200, dtype=np.uint8)   # a data block, over the edge of pieces 0 | 1
    damaged[4, 13, B - 1] ^= 0x01                                           # a parity block, the last tail byte
    damaged[3, 7, 2048 + 40:2048 + 60] ^= 0x3C                              # two blocks in piece row 1 of stripe 3
    damaged[3, 12, 2048 + 900:2048 + 910] ^= 0x55
    damaged[3, 7, 3 * 2048] ^= 0x80                                         # and one of them alone in piece row 3
    damaged[5, 0, 2047] ^= 0x10                                             # two blocks of a stripe in different rows
    damaged[5, 9, 2048] ^= 0x10
    view.copy_(torch.from_numpy(damaged))
    want_t, want_b = _verdicts(original, damaged, P, sel)
    assert want_t.tolist() == [[-1, -1, -1, -1, 13], [3, 3, -1, -1, -1], [-1] * 5, [-1, n, -1, 7, -1],
                               [0, 9, -1, -1, -1], [3, 3, -1, -1, -1]]
    assert want_b[3].tolist() == [0, 2, 0, 1, 0]
    _, targets, bad = _verify(torch, psum, view, P, recorded, sel)
    assert np.array_equal(targets, want_t) and np.array_equal(bad, want_b), (targets.tolist(), bad.tolist())
    code = ecg.ec_factory(RS104["type"], ecg.CodingParameters(**RS104["params"]))
    expected = recorded[torch.tensor(sel, device="cuda").long()].contiguous()
    ev, et, eb = psum.verify_ec_batch(code, view, P, expected, stripe_ids=_ints(torch, sel))
    assert np.array_equal(et.cpu().numpy(), want_t) and np.array_equal(eb.cpu().numpy(), want_b)
    assert np.array_equal(_u32(ev), _piece_sums(damaged[sel], P))
    assert np.array_equal(_u32(psum.ec_batch(code, view, P)), _piece_sums(damaged, P))
    # a verify over fewer columns answers its own column count for "more than one"
    _, targets, bad = _verify(torch, psum, view, P, recorded, sel, src=list(range(8)))
    want_t, want_b = _verdicts(original, damaged, P, sel, n_cols=8)
    assert want_t[3].tolist() == [-1, 7, -1, 7, -1]
    assert np.array_equal(targets, want_t) and np.array_equal(bad, want_b)
    assert np.array_equal(view.cpu().numpy(), damaged)


@gpu
@pytest.mark.parametrize("B,pitch,whole_view", [(8192, 8192, True), (8192, 8192 + 48, False), (8192 + 53, 10240, True),
                                                 (8192 + 53, 8192 + 64, False)],
                         ids=["stride-multiple", "stride-padded", "ragged-stride-multiple", "ragged-stride-padded"])
def test_the_chain_that_block_sums_cannot_start(ecg, oracle, torch_cuda, psum, sums, heal, B, pitch, whole_view):
    """RS(8,1): r = 1, ANY mode is refused.  One stripe has three blocks damaged in three different piece rows and a
    fourth row with two blocks damaged.  The block verify answers n and the heal leaves the stripe alone; the piece
    verify names a block per row, heal_rows turns that into piece-row stripes, and heal TARGET restores the three
    rows byte for byte and leaves the two-block row untouched byte for byte.  With a ragged last piece the third
    damage lies in it, tail bytes included."""
    torch = torch_cuda
    k, m, S, P = 8, 1, 4, 2048
    n, Q = k + m, -(-B // P)
    original, M = _encoded(oracle, RS81, S, B, 81)
    full, view = _upload(torch, original, pitch)
    assert (view.stride(0) % P == 0) == whole_view
    with pytest.raises(ecg.EcgError) as e:
        heal.encode_batch(k, m, M, view)
    assert e.value.code == ecg.ECG_EINVAL and b"proportional" in ecg.lib().ecg_last_error()
    psum.set_span_bytes(0)
    recorded = psum.pieces_batch(list(range(n)), view, P)
    recorded_blocks = sums.blocks_batch(list(range(n)), view)
    assert np.array_equal(_u32(recorded), _piece_sums(original, P))

    damaged = original.copy()
    rng = np.random.default_rng(81)
    damaged[2, 2, 10:1500] ^= rng.integers(1, 256, 1490, dtype=np.uint8)            # piece row 0: a data block
    damaged[2, 5, 2048:4096] ^= rng.integers(1, 256, 2048, dtype=np.uint8)          # piece row 1: another, all of it
    damaged[2, 0, 2 * 2048 + 7] ^= 0x21                                              # piece row 2: two blocks
    damaged[2, 4, 3 * 2048 - 1] ^= 0x42
    last = (Q - 1) * P                                                               # piece row Q - 1: the parity
    damaged[2, 8, last + 3:B] ^= rng.integers(1, 256, B - last - 3, dtype=np.uint8)
    damaged[0, 6, 5000] ^= 0xFF                                                      # and one byte of another stripe
    view.copy_(torch.from_numpy(damaged))
    image = full.cpu().numpy()
    sel = [2, 3, 0]
    ids = _ints(torch, sel)

    # the block sums: stripe 2 has more than one damaged block, and a heal with those targets changes no byte of it
    _, bt, bb = sums.verify_batch(list(range(n)), view, recorded_blocks[ids.long()].contiguous(), stripe_ids=ids)
    assert bt.tolist() == [n, -1, 6] and bb.tolist() == [5, 0, 1]
    heal.encode_batch(k, m, M, view, stripe_ids=_ints(torch, [2]), targets=bt[:1].contiguous())
    torch.cuda.synchronize()
    assert np.array_equal(full.cpu().numpy(), image)

    # the piece sums: a block per row
    d_targets, targets, bad = _verify(torch, psum, view, P, recorded, sel)
    want_t, _ = _verdicts(original, damaged, P, sel)
    assert want_t[0].tolist() == ([2, 5, n, 8] if Q == 4 else [2, 5, n, -1, 8]) and want_t[2, 2] == 6
    assert np.array_equal(targets, want_t)
    entries = psum.heal_rows(view, d_targets, P, stripe_ids=ids)
    if whole_view:
        per = view.stride(0) // P
        full_rows, full_targets = [2 * per, 2 * per + 1], [2, 5]
        if B % P == 0:
            full_rows, full_targets = full_rows + [2 * per + 3], full_targets + [8]
        rows0 = sorted(zip(entries[0][1].tolist(), entries[0][2].tolist()))
        assert rows0 == sorted(zip(full_rows + [0 * per + 2], full_targets + [6]))
        assert tuple(entries[0][0].shape)[1:] == (n, P) and entries[0][0].stride(0) == P
        assert len(entries) == (1 if B % P == 0 else 2)
    else:
        assert len(entries) == 4                                                     # piece rows 0, 1, 2 and the last
    if B % P:
        assert tuple(entries[-1][0].shape) == (S, n, B - last) and entries[-1][1].tolist() == [2]
    for rows_view, row_ids, row_targets in entries:
        assert row_ids.dtype == torch.int32 and row_targets.dtype == torch.int32 and row_ids.is_cuda
        assert rows_view.data_ptr() >= view.data_ptr() and rows_view.dtype == torch.uint8
        heal.encode_batch(k, m, M, rows_view, stripe_ids=row_ids, targets=row_targets)
    torch.cuda.synchronize()

    after = view.cpu().numpy()
    healed = original.copy()
    healed[2, :, 2 * P:3 * P] = damaged[2, :, 2 * P:3 * P]                           # the two-block row, untouched
    assert np.array_equal(after, healed)
    after_full = full.cpu().numpy()
    assert (after_full[:, :, B:] == 0xEE).all()                                      # nothing outside the blocks
    _, targets, bad = _verify(torch, psum, view, P, recorded, sel)
    want = np.full((3, Q), -1)
    want[0, 2] = n
    assert np.array_equal(targets, want) and bad.sum() == 2 and bad[0, 2] == 2


@gpu
def test_a_piece_row_into_heal2_target2(ecg, oracle, torch_cuda, psum, heal2):
    """RS(10,4), P = 2048.  In one piece row a data block is garbage and a parity block has a run.  A verify over all
    n blocks answers n for that row, so the pass that names the block is the one over the k data blocks; heal_rows
    (columns = k) makes the row a stripe, TARGET2 corrects the named block and finds the parity's run as its pair
    partner, and a verify over all n blocks then comes back clean."""
    torch = torch_cuda
    k, m, S, B, P = 10, 4, 4, 4 * 2048 + 21, 2048
    n = k + m
    original, M = _encoded(oracle, RS104, S, B, 105)
    _, view = _upload(torch, original)
    psum.set_span_bytes(0)
    recorded = psum.pieces_batch(list(range(n)), view, P)
    damaged = original.copy()
    rng = np.random.default_rng(12)
    damaged[1, 4, 2 * P:3 * P] = rng.integers(0, 256, P, dtype=np.uint8)            # garbage, one piece of it
    damaged[1, 11, 2 * P + 500:2 * P + 700] ^= rng.integers(1, 256, 200, dtype=np.uint8)   # a run in a second block
    damaged[3, 0, 7] ^= 0x80
    view.copy_(torch.from_numpy(damaged))
    sel = [1, 3, 2]
    _, targets, bad = _verify(torch, psum, view, P, recorded, sel)
    assert targets[0].tolist() == [-1, -1, n, -1, -1] and bad[0, 2] == 2 and targets[1, 0] == 0
    d_targets, targets, bad = _verify(torch, psum, view, P, recorded, sel, src=list(range(k)))
    assert targets.tolist() == [[-1, -1, 4, -1, -1], [0, -1, -1, -1, -1], [-1] * 5]
    entries = psum.heal_rows(view, d_targets, P, stripe_ids=_ints(torch, sel), columns=k)
    assert [(e[1].tolist(), e[2].tolist()) for e in entries] == [([3], [0]), ([1], [4])]
    reports = [heal2.encode_batch(k, m, M, v, stripe_ids=r, targets=t).cpu().numpy() for v, r, t in entries]
    assert reports[1][0, n + 2] > 0 and reports[1][0, n + 1] == 0           # pairs were needed, nothing was left
    _, targets, bad = _verify(torch, psum, view, P, recorded, sel)
    assert (targets == -1).all() and (bad == 0).all()
    assert np.array_equal(view.cpu().numpy(), original)


@gpu
def test_heal_rows_refuses_row_ids_past_int32(ecg, torch_cuda, psum):
    """A view whose stripe stride is 2^22 pieces: stripe 512's rows start at 2^31.  No byte of it is touched."""
    torch = torch_cuda
    base = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    stripes = torch.as_strided(base, (513, 2, 1024), (0, 512, 1))           # stride 0: handled per piece index
    targets = torch.full((1, 2), -1, dtype=torch.int32, device="cuda")
    targets[0, 1] = 1
    got = psum.heal_rows(stripes, targets, 512, stripe_ids=_ints(torch, [512]))
    assert len(got) == 1 and got[0][1].tolist() == [512] and got[0][2].tolist() == [1]

    class Wide:                                                              # the shape and strides of a 2^40-byte view
        shape, device = (513, 2, 1024), base.device
        def stride(self, d): return (1 << 31, 512, 1)[d]
        def storage_offset(self): return 0
    with pytest.raises(ecg.EcgError) as e:
        psum.heal_rows(Wide(), targets, 512, stripe_ids=_ints(torch, [512]))
    assert e.value.code == ecg.ECG_EINVAL and "int32" in str(e.value)


@gpu
def test_empty_calls_leave_the_outputs_untouched(torch_cuda, psum):
    torch = torch_cuda
    d = torch.zeros((2, 3, 64), dtype=torch.uint8, device="cuda")
    out = torch.full((2, 3), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    tg = torch.full((2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    c0, l0 = psum.counters(), psum.last_launch()
    ids = (ctypes.c_int * 3)(0, 1, 2)
    for B, S_sel in ((0, 2), (64, 0), (0, 0)):             # (a view of zero bytes has no pointer: the C ABI directly)
        assert psum.lib().ecg_psum_pieces_batch(3, ids, d.data_ptr(), d.stride(0), d.stride(1), B, 512, None, S_sel,
                                                out.data_ptr(), None) == 0
        assert psum.lib().ecg_psum_verify_batch(3, ids, d.data_ptr(), d.stride(0), d.stride(1), B, 512, None, S_sel,
                                                out.data_ptr(), out.data_ptr(), tg.data_ptr(), tg.data_ptr(),
                                                None) == 0
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A5A5A).all()) and bool((tg == 0x5A5A5A5A).all())
    assert psum.counters() == c0 and psum.last_launch() == l0
