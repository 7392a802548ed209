"""The update sums on the GPU (libecg_usum.so, include/ecg_usum.h).

Part one holds one call per case against tests/usum_plain.py: the WHOLE sum table -- pre-filled with random words, not
real sums, so that a word written that should not be shows -- and the whole report are compared.  The call reads only
delta, the records and the table, so these cases need no blocks.  Part two runs the chain on real stripes: sums by
ecg_sum / ecg_psum, ecg_update in WRITE mode with its delta output, ecg_usum with the update's report, and then the
table must equal fresh sums of all stripes and verify clean, while the table without the usum call is flagged at
exactly the touched blocks and piece rows.
"""
import contextlib
import functools
import json
import os

import numpy as np
import pytest

import update_plain as UP
import usum_plain as US

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
THREADS = 128                                              # gf_kernels.hpp kThreads: 16-byte columns per workgroup row
B0 = 8 * 1024 + 80                                         # the last piece of 512 .. 4096 bytes has 80 bytes
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return torch


@pytest.fixture(scope="module")
def usum(ecg):
    import ecg_usum
    ecg_usum.lib()
    return ecg_usum


def _code(name):
    c = next(c for c in GOLDEN if c["name"] == name)
    return c, c["k"], c["m"], [int(v) for v in c["matrix"]]


@contextlib.contextmanager
def _cols_per_wg(ecg, cpw):
    saved = ecg.get_option(ecg.ECG_OPT_COLS_PER_WG)
    try:
        ecg.set_option(ecg.ECG_OPT_COLS_PER_WG, cpw)
        yield
    finally:
        ecg.set_option(ecg.ECG_OPT_COLS_PER_WG, saved)


def _geometry(ecg, max_len, R, max_nnz, piece_bytes):
    cpw = ecg.get_option(ecg.ECG_OPT_COLS_PER_WG)
    cpw = THREADS if cpw <= 0 else -(-cpw // THREADS) * THREADS
    chunk = 16 * cpw
    return {"cols_per_wg": cpw, "wg_per_record": 1 if max_len < 1 else (chunk + max_len - 2) // chunk + 1, "R": R,
            "max_nnz": max_nnz, "piece_bytes": piece_bytes}


def _delta(rng, nbytes):
    """Random bytes with runs of zeros, some of them longer than a 16-byte column and than a wave's 1 KiB."""
    d = rng.integers(0, 256, nbytes, dtype=np.uint8)
    for at, ln in zip(rng.integers(0, nbytes, 12), (3, 16, 40, 100, 700, 1500, 5, 17, 33, 64, 2500, 9)):
        d[at:at + ln] = 0
    return d


def _table(rng, S, n, B, piece_bytes):
    return rng.integers(0, 1 << 32, (S, n, US.pieces(B, piece_bytes)), dtype=np.uint32)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(torch, ecg, usum, G, src, dst, ids, table, recs, delta, B, piece_bytes, which=3, max_len=None, up=None,
         want=None):
    """One apply on the device against the plain form (`want` = (table, report) if the caller has it already): the
    whole table, the whole report, the counters and the last launch."""
    recs = np.asarray(recs, dtype=np.int64).reshape(-1, 5)
    max_len = B if max_len is None else max_len
    if want is None:
        want_table = table.copy()
        want = (want_table, US.usum(G, src, dst, ids, want_table, recs, delta, B, max_len, piece_bytes, which, up))
    d_table = _dev(torch, table.view(np.int32))
    d_up = None if up is None else _dev(torch, np.asarray(up, dtype=np.int32))
    c0 = usum.counters()
    rep = usum.apply(d_table, recs, _dev(torch, delta), B, G=G, src_ids=src, dst_ids=dst, sum_ids=ids,
                     piece_bytes=piece_bytes, which=which, max_len=max_len, update_report=d_up)
    torch.cuda.synchronize()
    c1 = usum.counters()
    got = d_table.cpu().numpy().view(np.uint32)
    g = rep.cpu().numpy().astype(np.int64)
    assert np.array_equal(g, want[1]), (np.argwhere(g != want[1])[:4].tolist(), g[:6].tolist(), want[1][:6].tolist())
    assert np.array_equal(got, want[0]), (piece_bytes, which, np.argwhere(got != want[0])[:6].tolist())
    assert c1["launches"] - c0["launches"] == 1 and c1["records"] - c0["records"] == len(recs)
    nnz = int(np.count_nonzero(np.asarray(G).reshape(len(dst), len(src)), axis=0).max())
    assert usum.last_launch() == _geometry(ecg, max_len, len(recs), nnz, piece_bytes)
    return got, g


# ---- 1. offsets x lengths x staging alignment, at every piece size and two chunk sizes

OFFS = (0, 1, 15, 16, 17, 511, 512, 513)
LENS = (0, 1, 15, 16, 17, 31, 33, 511, 512, 513, 2048, 2049, 4097, None)          # None: B - off
PIECES = (0, 512, 1024, 4096, 1 << 30)


def _in_off(at, off, cls):
    """The first staging offset >= at that is congruent to off mod 16 (cls 0), mod 4 but not mod 16 (1), or at an odd
    distance from it (2)."""
    fits = {0: lambda d: d % 16 == 0, 1: lambda d: d % 4 == 0 and d % 16 != 0, 2: lambda d: d % 2 == 1}[cls]
    while not fits(at - off):
        at += 1
    return at


@functools.lru_cache(maxsize=None)
def _grid_case(piece_bytes):
    """RS(10,4), 2 stripes: the records (they overlap: here that is legal), delta, the random table and what the plain
    form makes of it.  Computed once per piece size and left unchanged."""
    _, k, m, M = _code("RS(10,4)")
    rng = np.random.default_rng(41)
    recs, at = [], 5
    for off in OFFS:
        for ln in LENS:
            for cls in range(3):
                ln_ = B0 - off if ln is None else ln
                at = _in_off(at, off, cls)
                recs.append([len(recs) % 2, (len(recs) // 2) % k, off, ln_, at])
                at += ln_ + int(rng.integers(0, 3))
    recs = np.array(recs, dtype=np.int64)
    delta = _delta(rng, at + 7)
    ids = list(range(k + m))
    table = _table(rng, 2, k + m, B0, piece_bytes)
    want = table.copy()
    rep = US.usum(M, ids[:k], ids[k:], ids, want, recs, delta, B0, B0, piece_bytes)
    return M, ids[:k], ids[k:], ids, table, recs, delta, (want, rep)


@gpu
@pytest.mark.parametrize("cpw", (128, 256))
@pytest.mark.parametrize("piece_bytes", PIECES)
def test_alignment_grid(ecg, torch_cuda, usum, piece_bytes, cpw):
    M, src, dst, ids, table, recs, delta, want = _grid_case(piece_bytes)
    assert not want[1][:, 0].any() and not np.array_equal(want[0], table)
    with _cols_per_wg(ecg, cpw):
        _run(torch_cuda, ecg, usum, M, src, dst, ids, table, recs, delta, B0, piece_bytes, want=want)
        assert usum.last_launch()["wg_per_record"] == (6 if cpw == 128 else 4)     # one record, several workgroups


# ---- 2. many records into one block and one piece

@gpu
@pytest.mark.parametrize("piece_bytes", (0, 512))
def test_many_records_meet_one_sum_word(ecg, torch_cuda, usum, piece_bytes):
    _, k, m, M = _code("RS(10,4)")
    rng = np.random.default_rng(42)
    recs, at = [], 0
    for i in range(64):                                                       # all in piece 3 of stripe 1
        ln = int(rng.integers(16, 49))
        off = 3 * 512 + int(rng.integers(0, 512 - ln + 1))
        recs.append([1, i % k, off, ln, at])
        at += ln + int(rng.integers(0, 4))
    delta = rng.integers(1, 256, at + 3, dtype=np.uint8)
    ids = list(range(k + m))
    table = _table(rng, 2, k + m, B0, piece_bytes)
    got, _ = _run(torch_cuda, ecg, usum, M, ids[:k], ids[k:], ids, table, recs, delta, B0, piece_bytes, max_len=48)
    changed = np.argwhere(got != table)
    q = 3 if piece_bytes else 0
    assert {tuple(c) for c in changed.tolist()} == {(1, b, q) for b in ids}   # parity words took all 64 contributions


# ---- 3. refusals, the update's report, which, sum_ids, columns of 0, 1, 3 and 8 nonzero coefficients

G_NNZ = np.zeros((8, 4), np.int64)
G_NNZ[5, 1] = 7
G_NNZ[[0, 3, 6], 2] = (1, 2, 142)
G_NNZ[:, 3] = (3, 1, 29, 76, 143, 157, 70, 95)
SRC_NNZ, DST_NNZ = [4, 9, 2, 30], [1, 0, 12, 5, 7, 11, 3, 8]
IDS_NNZ = [8, 30, 1, 9, 17, 12, 3, 2, 0]                                   # scrambled; 4, 5, 7, 11 missing, 17 unused


@gpu
@pytest.mark.parametrize("which", (1, 2, 3))
@pytest.mark.parametrize("piece_bytes", (0, 1024))
def test_refusals_which_and_named_sums(ecg, torch_cuda, usum, piece_bytes, which):
    rng = np.random.default_rng(43 + which)
    S, nb, ml = 3, 6000, 1500
    delta = _delta(rng, nb)
    off = rng.integers(0, B0 - ml, 40)
    recs = np.stack([rng.integers(0, S, 40), np.arange(40) % 4, off, rng.integers(0, ml + 1, 40),
                     rng.integers(0, nb - ml, 40)], axis=1)
    refused = [[-1, 0, 0, 4, 0], [S, 1, 0, 4, 0], [0, 4, 0, 4, 0], [0, -1, 0, 4, 0], [0, 3, B0 - 3, 4, 0],
               [0, 3, -16, 32, 0], [0, 3, 0, -1, 0], [0, 3, 0, ml + 1, 0], [0, 3, 0, 9, nb - 8], [0, 3, 0, 9, -1]]
    recs = np.concatenate([recs[:20], refused, recs[20:]])
    up = np.zeros((len(recs), 2), np.int64)
    up[[2, 7, 33], 0] = (3, 5, 1)                                              # the update refused three legal ones
    up[2, 1] = 99                                                              # its `changed` is not read
    table = _table(rng, S, len(IDS_NNZ), B0, piece_bytes)
    for report in (None, up):
        got, rep = _run(torch_cuda, ecg, usum, G_NNZ, SRC_NNZ, DST_NNZ, IDS_NNZ, table, recs, delta, B0, piece_bytes,
                        which, ml, report)
        assert rep[20:30, 0].tolist() == [1, 1, 2, 2, 3, 3, 3, 4, 5, 5] and not rep[20:30, 1].any()
        assert (got[:, IDS_NNZ.index(17)] == table[:, IDS_NNZ.index(17)]).all()
        data_cols = [IDS_NNZ.index(b) for b in SRC_NNZ if b in IDS_NNZ]
        par_cols = [IDS_NNZ.index(b) for b in DST_NNZ if b in IDS_NNZ]
        assert (got[:, data_cols] != table[:, data_cols]).any() == bool(which & 1)
        assert (got[:, par_cols] != table[:, par_cols]).any() == bool(which & 2)
    assert rep[[2, 7, 33]].tolist() == [[3, 0], [5, 0], [1, 0]]


@gpu
def test_delta_all_zero_writes_nothing(ecg, torch_cuda, usum):
    _, k, m, M = _code("Azure(8,2,2)")
    rng = np.random.default_rng(44)
    recs, nb = UP.legal_records(rng, 2, k, B0, 6, 3000)
    ids = list(range(k + m))
    table = _table(rng, 2, k + m, B0, 512)
    got, rep = _run(torch_cuda, ecg, usum, M, ids[:k], ids[k:], ids, table, recs, np.zeros(nb, np.uint8), B0, 512)
    assert np.array_equal(got, table) and not rep.any()


# ---- 4. the longest block

@gpu
@pytest.mark.parametrize("piece_bytes", (0, 1 << 30))
def test_block_of_2_31_less_1(ecg, torch_cuda, usum, piece_bytes):
    """Only offsets and tail shifts are long: no block exists."""
    _, k, m, M = _code("RS(10,4)")
    B = (1 << 31) - 1
    rng = np.random.default_rng(45)
    delta = rng.integers(1, 256, 200, dtype=np.uint8)
    recs = [[0, 2, 5, 33, 7], [0, 7, B - 40, 40, 50], [0, 9, B - 1, 1, 3], [0, 0, (1 << 30) - 9, 20, 100],
            [0, 1, B - 15, 15, 120], [0, 3, B, 0, 0], [0, 3, B, 1, 0]]
    ids = list(range(k + m))
    table = _table(rng, 1, k + m, B, piece_bytes)
    _, rep = _run(torch_cuda, ecg, usum, M, ids[:k], ids[k:], ids, table, recs, delta, B, piece_bytes, max_len=64)
    assert rep.tolist() == [[0, 33], [0, 40], [0, 1], [0, 20], [0, 15], [0, 0], [3, 0]]


# ---- 5. batch scope and stream

@gpu
def test_batch_scope_flushes_first_and_side_stream_orders(ecg, torch_cuda, usum):
    torch = torch_cuda
    _, k, m, M = _code("RS(10,4)")
    rng = np.random.default_rng(46)
    B = 1077
    recs, nb = UP.legal_records(rng, 1, k, B, 6, 300)
    delta = _delta(rng, nb)
    ids = list(range(k + m))
    table = _table(rng, 1, k + m, B, 0)
    want = table.copy()
    want_rep = US.usum(M, ids[:k], ids[k:], ids, want, recs, delta, B, 300, 0)
    code = ecg.ec_factory(ecg.ECTYPE.RS, ecg.CodingParameters(k=k, m=m))
    blocks = torch.zeros((k + m, B), dtype=torch.uint8, device="cuda")
    d_table = _dev(torch, table.view(np.int32))
    with ecg.batch():                                                      # an encode is recorded, not launched ...
        code.encode([blocks[j] for j in range(k)], [blocks[k + j] for j in range(m)], B)
        rep = usum.apply(d_table, recs, _dev(torch, delta), B, k=k, m=m, matrix=M, max_len=300)   # ... until here
    torch.cuda.synchronize()
    assert np.array_equal(rep.cpu().numpy(), want_rep)
    assert np.array_equal(d_table.cpu().numpy().view(np.uint32), want)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                          # upload, apply and read back on one stream
        d2 = _dev(torch, table.view(np.int32))
        rep2 = usum.apply(d2, recs, _dev(torch, delta), B, code=code, max_len=300)
        after = d2.clone()
    side.synchronize()
    assert np.array_equal(after.cpu().numpy().view(np.uint32), want) and np.array_equal(rep2.cpu().numpy(), want_rep)


# ---- 6. end to end on real stripes: sums, update, update sums, verify

def _fresh(ids, stripes, piece_bytes):
    import ecg_psum
    import ecg_sum
    if piece_bytes == 0:
        return ecg_sum.blocks_batch(ids, stripes).reshape(stripes.shape[0], len(ids), 1).contiguous()
    return ecg_psum.pieces_batch(ids, stripes, piece_bytes)


def _verify(ids, stripes, piece_bytes, table):
    """(targets, bad) as [S][Q] numpy arrays."""
    import ecg_psum
    import ecg_sum
    if piece_bytes == 0:
        _, targets, bad = ecg_sum.verify_batch(ids, stripes, table.reshape(table.shape[0], len(ids)).contiguous())
        return targets.cpu().numpy()[:, None], bad.cpu().numpy()[:, None]
    _, targets, bad = ecg_psum.verify_batch(ids, stripes, piece_bytes, table)
    return targets.cpu().numpy(), bad.cpu().numpy()


@gpu
@pytest.mark.parametrize("piece_bytes", (0, 512))
@pytest.mark.parametrize("name", ("RS(10,4)", "Azure(8,2,2)"))
def test_update_then_usum_then_verify_is_clean(ecg, torch_cuda, usum, name, piece_bytes):
    import ecg_update
    torch = torch_cuda
    c, k, m, M = _code(name)
    n, S, B = k + m, 16, B0
    Q = US.pieces(B, piece_bytes)
    G = np.asarray(M).reshape(m, k)
    rng = np.random.default_rng(47 + len(name))
    code = ecg.ec_factory(c["type"], ecg.CodingParameters(**c["params"]))
    ids = list(range(n))
    stripes = torch.empty((S, n, B), dtype=torch.uint8, device="cuda")
    ecg.fill_random(stripes, 0xC0DE)
    ecg.encode_batch(k, m, M, stripes[:, :k], stripes[:, k:])
    held = stripes.clone()                                                  # the parity holder's copy
    recs, nb = UP.legal_records(rng, S, k, B, 3, 3000)
    recs = np.concatenate([recs[recs[:, 0] != 5], [[S, 0, 0, 4, 0]]])       # stripe 5 untouched; one refused record
    old = stripes.cpu().numpy()
    data_in = np.zeros(nb, np.uint8)
    for s, col, off, ln, in_off in recs[:-1]:                               # every written byte changes
        data_in[in_off:in_off + ln] = old[s, col, off:off + ln] ^ rng.integers(1, 256, ln, dtype=np.uint8)
    d_in = _dev(torch, data_in)
    d_delta = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    table = _fresh(ids, stripes, piece_bytes)
    stale = table.clone()

    up = ecg_update.ec_batch(code, stripes, recs, d_in, delta_out=d_delta, max_len=3000)
    rep = usum.apply(table, recs, d_delta, B, code=code, piece_bytes=piece_bytes, max_len=3000, update_report=up)
    torch.cuda.synchronize()
    assert np.array_equal(rep.cpu().numpy(), up.cpu().numpy()) and rep.cpu().numpy()[-1].tolist() == [1, 0]
    fresh = _fresh(ids, stripes, piece_bytes)
    assert torch.equal(table, fresh) and not torch.equal(table, stale)
    targets, bad = _verify(ids, stripes, piece_bytes, table)
    assert (targets == -1).all() and not bad.any()

    # the verify is not vacuous: the table as it was is flagged at exactly the touched blocks and piece rows
    touched = np.zeros((S, n, Q), bool)
    for s, col, off, ln, _ in recs[:-1]:
        if ln > 0:
            q0, q1 = (off // piece_bytes, (off + ln - 1) // piece_bytes) if piece_bytes else (0, 0)
            touched[s, [col] + [k + i for i in range(m) if G[i, col]], q0:q1 + 1] = True
    assert np.array_equal((fresh != stale).cpu().numpy(), touched) and not touched[5].any()
    targets, bad = _verify(ids, stripes, piece_bytes, stale)
    count = touched.sum(axis=1)
    assert np.array_equal(bad, count) and count.max() > 1
    first = np.where(count == 0, -1, np.where(count == 1, touched.argmax(axis=1), n))
    assert np.array_equal(targets, first)

    # the split form: a data holder (which = 1), and a parity holder that is shipped delta and applies it in DELTA mode
    split = stale.clone()
    usum.apply(split, recs, d_delta, B, k=k, m=m, matrix=M, piece_bytes=piece_bytes, which=usum.DATA, max_len=3000,
               update_report=up)
    assert torch.equal(split[:, :k], fresh[:, :k]) and torch.equal(split[:, k:], stale[:, k:])
    up2 = ecg_update.ec_batch(code, held, recs, d_delta, mode=ecg_update.DELTA, max_len=3000)
    usum.apply(split, recs, d_delta, B, G=M, src_ids=ids[:k], dst_ids=ids[k:], sum_ids=ids, piece_bytes=piece_bytes,
               which=usum.PARITY, max_len=3000, update_report=up2)
    torch.cuda.synchronize()
    assert torch.equal(split, fresh) and torch.equal(held[:, k:], stripes[:, k:])
