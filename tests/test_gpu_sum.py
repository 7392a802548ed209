"""Block checksums on the GPU: every crc_sum_kernel / crc_sum_byte_kernel of libecg_sum.so and the verify's compare
against the definition (tests/crc32c_plain.py, which shares no table with the product).

Every case uploads an arena -- blocks inside 64-byte bands of 0xC3, a pitch with a gap, slots the call does not name --
runs one call, compares ALL its sums with the definition, the whole arena with its image before the call, `counters()`
with the declared launches and bytes, and `last_launch()` with the geometry the case is meant to reach: a case that
fell back to the byte path fails.

The blocks of a case hold distinct random bytes (stripes 0..2); further stripes hold the blocks that isolate one term
each: all 0x00 and all 0xFF (the affine term) and ONE-HOT blocks, a single nonzero byte at 0, 3, 4, 15, 16, 2047, 2048,
B - 1, each segment's and each row's first and last byte for both forced segment sizes, and the first byte of the
tail (one position multiplier each).  The reference of a block size is computed once and shared, and every strided
case runs with both LDS table schemes.
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
ROW, AUTO_SEGMENT = 2048, 256 << 10                     # sum_kernels.hpp kSumRowBytes, kSumAutoSegment
BYTE_RUN, BYTE_WG = 64, 64 * 128                        # byte path: bytes per lane, per workgroup
SLOTS, SRC = 7, [5, 0, 3, 6, 2]                         # n = 5 of a stripe's 7 slots, permuted
SIZES = (1, 3, 15, 16, 17, 2047, 2048, 2049, 4096, 6144 + 16 + 5)
SEGMENTS = (2048, 4096)
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return torch


@pytest.fixture(scope="module")
def sums(ecg):
    import ecg_sum
    ecg_sum.lib()
    yield ecg_sum
    ecg_sum.set_segment_bytes(0)
    ecg_sum.set_table_scheme(-1)


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


# ---- blocks, arenas, geometry

def _one_hot_positions(B):
    vec = B & ~15
    pos = {0, 3, 4, 15, 16, 2047, 2048, B - 1, vec}
    for seg in SEGMENTS:
        for g in range(0, B // seg + 2):
            pos |= {g * seg, g * seg - 1}
    for r in range(1, 4):                                # rows are aligned to a segment's end: the ragged one's edges
        pos |= {vec - r * ROW, vec - r * ROW - 1}
    return sorted(p for p in pos if 0 <= p < B)


@functools.lru_cache(maxsize=None)
def _blocks(B):
    """(blocks [S][SLOTS][B], their sums [S][SLOTS] by the definition, the selection): three stripes of distinct random
    bytes, then the stripes that hold the special blocks in the summed slots.  Read-only: shared by every case of B."""
    rng = np.random.default_rng(1000 + B)
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
    want = CP.many(blocks)
    blocks.setflags(write=False)
    want.setflags(write=False)
    return blocks, want, sel


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


def _geometry(B, seg, aligned, blocks):
    """The launch the library is meant to choose (include/ecg_sum.h ecg_sum_last_launch), restated."""
    vec = (B & ~15) if aligned else 0
    if vec:
        sb = min(seg or AUTO_SEGMENT, -(-vec // ROW) * ROW)
        return dict(path=0, segment_bytes=sb, segments_per_block=-(-vec // sb), blocks=blocks)
    bpw = min(BYTE_WG, -(-B // BYTE_RUN) * BYTE_RUN)
    return dict(path=1, segment_bytes=bpw, segments_per_block=-(-B // bpw), blocks=blocks)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _ints(torch, values):
    return None if values is None else torch.tensor([int(v) for v in values], dtype=torch.int32, device="cuda")


def _check_call(torch, sums, d, img, B, seg, aligned, n_blocks, call, want, launches=None):
    """Run `call` with the segment forced to `seg`; compare all sums, the arena, the counters and the geometry."""
    sums.set_segment_bytes(seg)
    c0 = sums.counters()
    got = call()
    torch.cuda.synchronize()
    c1 = sums.counters()
    assert got.dtype == torch.int32 and tuple(got.shape) == want.shape
    g = _u32(got)
    if not np.array_equal(g, want):
        diff = np.argwhere(g != want)
        first = tuple(diff[0])
        raise AssertionError((B, seg, aligned, len(diff), diff[:8].tolist(), hex(int(g[first])), hex(int(want[first]))))
    assert np.array_equal(d.cpu().numpy(), img), (B, seg, "the arena changed")
    vec = (B & ~15) if aligned else 0
    assert c1["launches"] - c0["launches"] == ((vec > 0) + (vec < B) if launches is None else launches)
    assert c1["bytes"] - c0["bytes"] == n_blocks * B
    last = sums.last_launch()
    geo = _geometry(B, seg, aligned, n_blocks)
    assert {f: last[f] for f in geo} == geo, (B, seg, aligned, last)
    return g


def _strided(torch, sums, B, seg, shift=0, pitch=None):
    """Both table schemes (the byte path has none: table_scheme reads 0)."""
    blocks, want, sel = _blocks(B)
    img = _arena(blocks, pitch)
    d = _to_dev(torch, img, shift)
    view = d[:, :, GUARD:GUARD + B]
    aligned = shift % 16 == 0 and img.shape[2] % 16 == 0
    ids = _ints(torch, sel)
    try:
        for scheme in (0, 1):
            sums.set_table_scheme(scheme)
            _check_call(torch, sums, d, img, B, seg, aligned, len(sel) * len(SRC),
                        lambda: sums.blocks_batch(SRC, view, stripe_ids=ids), want[sel][:, SRC])
            assert sums.last_launch()["table_scheme"] == (scheme if aligned and B >= 16 else 0)
    finally:
        sums.set_table_scheme(-1)


# ---- every size at which a part of the kernel can go wrong

def test_the_sizes_reach_one_two_and_more_segments_a_ragged_one_and_the_tail():
    """No library call: the restated geometry alone, so that the size list above is seen to reach every case."""
    geo = {(B, seg): _geometry(B, seg, True, 1) for B in SIZES for seg in SEGMENTS}
    assert [geo[B, 2048]["path"] for B in SIZES] == [1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    assert geo[2049, 4096]["segments_per_block"] == 1 and geo[2049, 4096]["segment_bytes"] == 2048
    assert geo[4096, 2048]["segments_per_block"] == 2 and geo[4096, 4096]["segments_per_block"] == 1
    assert geo[6165, 4096]["segments_per_block"] == 2     # 4096 and a ragged 2048 + 16, then 5 bytes of tail
    assert geo[6165, 2048]["segments_per_block"] == 4     # three whole rows and a ragged segment of 16 bytes
    assert max(len(_one_hot_positions(B)) for B in SIZES) <= 30


@gpu
@pytest.mark.parametrize("B", SIZES)
def test_every_size_and_segment(torch_cuda, sums, B):
    for seg in SEGMENTS:
        _strided(torch_cuda, sums, B, seg)


@gpu
@pytest.mark.parametrize("B", (17, 2049, 6144 + 16 + 5, 8192 + 100))
def test_unaligned_base_and_stride_run_the_byte_kernel(torch_cuda, sums, B):
    """base + 1 and a block stride of 2049 + B: one byte-kernel launch covers everything (8192 + 100: two workgroups
    per block)."""
    _strided(torch_cuda, sums, B, 2048, shift=1, pitch=2049 + B)
    assert sums.last_launch()["path"] == 1
    if B > BYTE_WG:
        assert sums.last_launch()["segments_per_block"] == 2


@gpu
def test_all_stripes_in_order_and_an_out_tensor(torch_cuda, sums):
    """stripe_ids None; `out` prefilled with a pattern: the call zeroes it before it XORs into it."""
    torch = torch_cuda
    B = 6144 + 16 + 5
    blocks, want, _ = _blocks(B)
    img = _arena(blocks)
    d = _to_dev(torch, img)
    view = d[:, :, GUARD:GUARD + B]
    out = torch.full((blocks.shape[0], len(SRC)), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    got = _check_call(torch, sums, d, img, B, 2048, True, blocks.shape[0] * len(SRC),
                      lambda: sums.blocks_batch(SRC, view, out=out), want[:, SRC])
    assert np.array_equal(_u32(out), got)


@gpu
def test_more_columns_than_one_launch_holds(torch_cuda, sums):
    """n = 300 block ids, more than the 256 a launch carries in its arguments: two vector and two byte launches."""
    torch = torch_cuda
    B, n = 2048 + 16 + 3, 300
    rng = np.random.default_rng(300)
    blocks = rng.integers(0, 256, (2, n, B), dtype=np.uint8)
    img = _arena(blocks)
    d = _to_dev(torch, img)
    view = d[:, :, GUARD:GUARD + B]
    src = [int(v) for v in rng.permutation(n)]
    _check_call(torch, sums, d, img, B, 2048, True, 2 * n, lambda: sums.blocks_batch(src, view),
                CP.many(blocks)[:, src], launches=4)


# ---- large exponents, the auto segment

def _pitched(torch, S, n, B):
    """An uninitialised [S][n][B] view whose blocks are 16-byte aligned."""
    pitch = (B + 15) & ~15
    return torch.empty((S, n, pitch), dtype=torch.uint8, device="cuda")[:, :, :B]


@gpu
@pytest.mark.parametrize("S,n,B,scheme", [(1, 2, (1 << 29) + (1 << 11) + 21, -1), (2, 3, (1 << 20) + 53, 0),
                                          (2, 3, (1 << 20) + 53, 1)], ids=["512MiB", "1MiB-scheme0", "1MiB-scheme1"])
def test_large_blocks_with_the_auto_segment(ecg, torch_cuda, sums, S, n, B, scheme):
    """Against ecg_sum_crc32c of the same bytes copied back (tests/test_sum_host.py pins it on the definition, which
    would walk these sizes for minutes).  8 * B passes 2^32 in the first case, which runs a second time with one row
    per segment: only then does a segment have 2^29 bytes or more behind it."""
    torch = torch_cuda
    full = torch.empty((S, n, (B + 15) & ~15), dtype=torch.uint8, device="cuda")
    ecg.fill_random(full, 0xB10C + n)
    view = full[:, :, :B]
    sums.set_segment_bytes(0)
    sums.set_table_scheme(scheme)
    c0 = sums.counters()
    got = sums.blocks_batch(list(range(n)), view)
    torch.cuda.synchronize()
    c1 = sums.counters()
    sums.set_table_scheme(-1)
    assert scheme < 0 or sums.last_launch()["table_scheme"] == scheme
    host = view.cpu().numpy()
    want = np.array([[sums.crc32c(host[s, j]) for j in range(n)] for s in range(S)], dtype=np.uint32)
    assert np.array_equal(_u32(got), want), ([hex(int(v)) for v in _u32(got).ravel()], [hex(int(v)) for v in want.ravel()])
    assert len(set(int(v) for v in want.ravel())) == S * n
    assert c1["launches"] - c0["launches"] == 2 and c1["bytes"] - c0["bytes"] == S * n * B
    last = sums.last_launch()
    geo = _geometry(B, 0, True, S * n)
    assert geo["segment_bytes"] == AUTO_SEGMENT and geo["segments_per_block"] == -(-(B & ~15) // AUTO_SEGMENT)
    assert {f: last[f] for f in geo} == geo, last
    if B >= 1 << 29:
        # with 256 KiB segments no segment of this block has 2^29 bytes behind it; with one row per segment the first
        # 2 KiB do, and 8 * that passes 2^32
        assert B - AUTO_SEGMENT < 1 << 29 <= B - ROW
        sums.set_segment_bytes(ROW)
        got = sums.blocks_batch(list(range(n)), view)
        torch.cuda.synchronize()
        assert np.array_equal(_u32(got), want)
        geo = _geometry(B, ROW, True, S * n)
        last = sums.last_launch()
        assert geo["segments_per_block"] == (1 << 18) + 2 and {f: last[f] for f in geo} == geo, last
    assert np.array_equal(view.cpu().numpy(), host)


# ---- the handle's forms, the batch scope

RS64 = next(c for c in GOLDEN if c["name"] == "RS(6,4)")
RS104 = next(c for c in GOLDEN if c["name"] == "RS(10,4)")
RS81 = next(c for c in GOLDEN if c["name"] == "RS(8,1)")


@gpu
def test_inline_through_ec_and_ec_batch(ecg, torch_cuda, sums):
    """RS(6,4) at B = 4096 + 21: ecg_sum.ec over the ten block pointers of one stripe (INLINE), aligned and shifted by
    one byte; ec_batch over the stripes of the same handle with a selection."""
    torch = torch_cuda
    code = ecg.ec_factory(RS64["type"], ecg.CodingParameters(**RS64["params"]))
    k, n, B = code.k, code.k + code.m, 4096 + 21
    assert (k, n) == (6, 10)
    rng = np.random.default_rng(64)
    blocks = rng.integers(0, 256, (3, n, B), dtype=np.uint8)
    want = CP.many(blocks)
    img = _arena(blocks)
    for shift in (0, 1):
        d = _to_dev(torch, img, shift)
        for s in (0, 2):
            ptrs = [d[s, b, GUARD:GUARD + B] for b in range(n)]
            _check_call(torch, sums, d, img, B, 2048, shift == 0, n, lambda: sums.ec(code, ptrs[:k], ptrs[k:], B),
                        want[s:s + 1])
    d = _to_dev(torch, img)
    view = d[:, :, GUARD:GUARD + B]
    _check_call(torch, sums, d, img, B, 4096, True, 3 * n, lambda: sums.ec_batch(code, view), want)
    _check_call(torch, sums, d, img, B, 0, True, 2 * n,
                lambda: sums.ec_batch(code, view, stripe_ids=_ints(torch, [2, 0])), want[[2, 0]])


@gpu
def test_sum_flushes_the_batch_scope(ecg, oracle, torch_cuda, sums):
    """A dev_matrix_encode recorded in a batch scope, then a sum of the same blocks inside the scope: the sum flushes
    the scope first, so it sees the encode's parity, not the stale one."""
    torch = torch_cuda
    k, m, B = 6, 4, 4096 + 16
    M = [int(v) for v in RS64["matrix"]]
    rng = np.random.default_rng(65)
    data = [rng.integers(0, 256, B, dtype=np.uint8) for _ in range(k)]
    coding = [np.zeros(B, np.uint8) for _ in range(m)]
    oracle.jerasure_matrix_encode(k, m, M, data, coding, B)
    want = CP.many(np.stack(data + coding))
    stale = np.stack(data + [np.full(B, 0xA5, np.uint8)] * m)[None]
    assert not np.array_equal(CP.many(stale[0])[k:], want[k:])
    d = torch.from_numpy(stale).cuda()
    with ecg.batch():
        ecg.dev_matrix_encode(k, m, M, [d[0, j] for j in range(k)], [d[0, k + j] for j in range(m)], B)
        got = sums.blocks_batch(list(range(k + m)), d)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(got)[0], want)


# ---- verify, and the chain the headers promise

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


def _upload(torch, stripes):
    S, n, B = stripes.shape
    view = _pitched(torch, S, n, B)
    view.copy_(torch.from_numpy(stripes))
    return view


def _verify(torch, sums, view, recorded, sel, src=None):
    n = view.shape[1] if src is None else len(src)
    src = list(range(n)) if src is None else src
    expected = recorded[torch.tensor(sel, device="cuda").long()][:, :n].contiguous()
    c0 = sums.counters()
    got, targets, bad = sums.verify_batch(src, view, expected, stripe_ids=_ints(torch, sel))
    torch.cuda.synchronize()
    assert sums.counters()["launches"] - c0["launches"] == 3         # the vector part, the tail, the compare
    assert sums.last_launch()["path"] == 0
    assert targets.dtype == torch.int32 and bad.dtype == torch.int32 and targets.is_contiguous()
    host = view.cpu().numpy()
    assert np.array_equal(_u32(got), CP.many(host[sel][:, src]))     # the computed sums, every one
    return targets, [int(v) for v in targets.cpu()], [int(v) for v in bad.cpu()]


@gpu
def test_verify_and_the_heal_it_feeds(ecg, oracle, torch_cuda, sums, heal):
    """S = 8 stripes of RS(10,4), B = 4096 + 21, sums recorded clean.  No damage: every target -1.  A run in one block:
    that block.  Two damaged blocks: n.  verify -> its targets straight into ecg_heal_encode_batch TARGET -> verify
    again: clean, and the stripe with two damaged blocks untouched, byte for byte."""
    torch = torch_cuda
    k, m, S, B = 10, 4, 8, 4096 + 21
    n = k + m
    original, M = _encoded(oracle, RS104, S, B, 104)
    view = _upload(torch, original)
    sums.set_segment_bytes(2048)
    recorded = sums.blocks_batch(list(range(n)), view)
    assert np.array_equal(_u32(recorded), CP.many(original))
    code = ecg.ec_factory(RS104["type"], ecg.CodingParameters(**RS104["params"]))
    assert np.array_equal(_u32(sums.ec_batch(code, view)), _u32(recorded))
    sel = [6, 2, 0, 5, 7, 1]
    _, targets, bad = _verify(torch, sums, view, recorded, sel)
    assert targets == [-1] * 6 and bad == [0] * 6

    damaged = original.copy()
    rng = np.random.default_rng(11)
    damaged[2, 3, 100:2300] ^= rng.integers(1, 256, 2200, dtype=np.uint8)   # a data block, across a row edge
    damaged[6, 13, B - 1] ^= 0x01                                           # a parity block, the last tail byte
    damaged[5, 7, 40:60] ^= 0x3C                                            # two blocks of one stripe
    damaged[5, 12, 3000:3010] ^= 0x55
    view.copy_(torch.from_numpy(damaged))
    d_targets, targets, bad = _verify(torch, sums, view, recorded, sel)
    assert targets == [13, 3, -1, n, -1, -1] and bad == [1, 1, 0, 2, 0, 0]
    ev, et, eb = sums.verify_ec_batch(code, view, recorded[torch.tensor(sel, device="cuda").long()].contiguous(),
                                      stripe_ids=_ints(torch, sel))
    assert [int(v) for v in et.cpu()] == targets and [int(v) for v in eb.cpu()] == bad

    report = heal.encode_batch(k, m, M, view, stripe_ids=_ints(torch, sel), targets=d_targets).cpu().numpy()
    assert report[0, 13] == 1 and report[1, 3] == 2200 and not report[3, :n].any() and report[3, n + 1] == 30
    _, targets, bad = _verify(torch, sums, view, recorded, sel)
    assert targets == [-1, -1, -1, n, -1, -1] and bad == [0, 0, 0, 2, 0, 0]
    after = view.cpu().numpy()
    assert np.array_equal(after[5], damaged[5])                             # untouched, byte for byte
    keep = [s for s in range(S) if s != 5]
    assert np.array_equal(after[keep], original[keep])


@gpu
def test_the_chain_over_rs_8_1(ecg, oracle, torch_cuda, sums, heal):
    """r = 1: ANY mode is refused, so the heal cannot start without a named block -- the case ecg_heal.h cites.  The
    sums name it."""
    torch = torch_cuda
    k, m, S, B = 8, 1, 4, 4096 + 21
    original, M = _encoded(oracle, RS81, S, B, 81)
    view = _upload(torch, original)
    with pytest.raises(ecg.EcgError) as e:
        heal.encode_batch(k, m, M, view)
    assert e.value.code == ecg.ECG_EINVAL and b"proportional" in ecg.lib().ecg_last_error()
    sums.set_segment_bytes(4096)
    recorded = sums.blocks_batch(list(range(k + m)), view)
    damaged = original.copy()
    rng = np.random.default_rng(81)
    damaged[0, 8, 4000:] ^= rng.integers(1, 256, B - 4000, dtype=np.uint8)  # the parity, into the tail
    damaged[3, 2] = rng.integers(0, 256, B, dtype=np.uint8)                 # a whole data block
    view.copy_(torch.from_numpy(damaged))
    sel = [3, 1, 0]
    d_targets, targets, bad = _verify(torch, sums, view, recorded, sel)
    assert targets == [2, -1, 8] and bad == [1, 0, 1]
    heal.encode_batch(k, m, M, view, stripe_ids=_ints(torch, sel), targets=d_targets)
    _, targets, bad = _verify(torch, sums, view, recorded, sel)
    assert targets == [-1, -1, -1] and bad == [0, 0, 0]
    assert np.array_equal(view.cpu().numpy(), original)


@gpu
def test_targets_into_heal2_target2(ecg, oracle, torch_cuda, sums, heal2):
    """One data block garbage plus a run in a parity block of the same stripe.  A verify over all n blocks sees two
    mismatches and answers n by its definition, so the pass that names the block is the one a store runs over its k
    data blocks (src_ids 0..k-1, whose columns are the block ids): it names the garbage block, TARGET2 corrects it and
    finds the parity's run as its pair partner, and a verify over all n blocks then comes back clean."""
    torch = torch_cuda
    k, m, S, B = 10, 4, 4, 4096 + 21
    n = k + m
    original, M = _encoded(oracle, RS104, S, B, 105)
    view = _upload(torch, original)
    sums.set_segment_bytes(0)
    recorded = sums.blocks_batch(list(range(n)), view)
    damaged = original.copy()
    rng = np.random.default_rng(12)
    damaged[1, 4] = rng.integers(0, 256, B, dtype=np.uint8)                 # garbage
    damaged[1, 11, 500:700] ^= rng.integers(1, 256, 200, dtype=np.uint8)    # a run in a second block
    damaged[3, 0, 7] ^= 0x80
    view.copy_(torch.from_numpy(damaged))
    sel = [1, 3, 2]
    _, targets, bad = _verify(torch, sums, view, recorded, sel)
    assert targets == [n, 0, -1] and bad == [2, 1, 0]
    d_targets, targets, bad = _verify(torch, sums, view, recorded, sel, src=list(range(k)))
    assert targets == [4, 0, -1] and bad == [1, 1, 0]
    report = heal2.encode_batch(k, m, M, view, stripe_ids=_ints(torch, sel), targets=d_targets).cpu().numpy()
    assert report[0, n + 2] > 0 and report[0, n + 1] == 0                   # pairs were needed, nothing was left
    _, targets, bad = _verify(torch, sums, view, recorded, sel)
    assert targets == [-1, -1, -1] and bad == [0, 0, 0]
    assert np.array_equal(view.cpu().numpy(), original)


@gpu
def test_empty_calls_leave_the_outputs_untouched(torch_cuda, sums):
    torch = torch_cuda
    d = torch.zeros((2, 3, 64), dtype=torch.uint8, device="cuda")
    out = torch.full((2, 3), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    c0 = sums.counters()
    ids = (ctypes.c_int * 3)(0, 1, 2)
    for B, S_sel in ((0, 2), (64, 0), (0, 0)):             # (a view of zero bytes has no pointer: the C ABI directly)
        assert sums.lib().ecg_sum_blocks_batch(3, ids, d.data_ptr(), d.stride(0), d.stride(1), B, None, S_sel,
                                               out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A5A5A).all()) and sums.counters() == c0
