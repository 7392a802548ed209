"""The verified range read on the GPU: the kernels of libecg_vread.so against the definition (tests/vread_plain.py over
tests/dread_plain.py and tests/crc32c_plain.py), bit for bit.

Every case uploads a guard-band arena (tests/gf_arena.py) whose lost blocks are filled with garbage and an answer buffer
filled with a canary, runs one call and compares THE WHOLE ANSWER BUFFER, the full report, THE WHOLE SUMS TABLE and THE
WHOLE ARENA (which must be unchanged) with the definition, then `counters()` and `last_launch()`: a store outside a
record's range or into a refused record's bytes shows, a read of a lost block shows, a sum that lands in another
record's row shows.  The recorded table is that of the stripes before anything was lost or damaged.

B = 4096 + 512 + 48 + 5: a ragged last piece with a vector part and a byte tail; Q = 10 / 3 / 2 / 1 at P = 512 / 2048 /
4096 / 8192, and block sums.  Every shape runs at span = auto and span = 2048, where a 4096-byte piece is split over
two workgroups and a 512-byte piece shares a row with three others.

Every test here loads libecg_vread.so and runs its kernels.
"""
import contextlib

import numpy as np
import pytest

import dread_plain as DP
import gf_arena as A
import heal2_plain as P2
import test_gpu_dread as TG
import vread_plain as VP

GUARD = A.GUARD
CANARY = 0xC9
B0, S0 = 4096 + 512 + 48 + 5, 6
PIECES = (512, 2048, 4096, 8192, 0)
AUTO_SPAN, ROW = 256 << 10, 2048                                # psum_kernels.hpp kPsumAutoSpan, kPsumRowBytes
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return torch


@pytest.fixture(scope="module")
def vread(ecg):
    import ecg_vread
    ecg_vread.lib()
    return ecg_vread


@contextlib.contextmanager
def _span(V, span):
    V.set_span_bytes(span)
    try:
        yield
    finally:
        V.set_span_bytes(0)


def _geometry(P, B, max_len, R, span, path=0):
    Pk = P or max(512, 1 << (B - 1).bit_length())
    NP = VP.max_pieces(max_len, P, B)
    cover = max(1, min(NP * Pk, B))
    span = min(span or AUTO_SPAN, -(-cover // ROW) * ROW)
    return {"path": path, "piece_bytes": Pk, "max_pieces": NP, "span_bytes": span, "wg_per_record": -(-cover // span),
            "R": R}


def _run(torch, V, img, B, H, src, lost, P, table, recs, out_bytes, call, max_len=None, shift=0, span=0):
    """Upload img (base `shift` bytes past a 16-byte boundary) and a canary-filled answer buffer, run
    call(view, lost, P, table, records, out) once and compare report, sums, answer buffer, arena, counters and last
    launch with the definition.  Returns (report, sums, answer), numpy."""
    recs = np.asarray(recs, dtype=np.int64).reshape(-1, 5)
    max_len = B if max_len is None else max_len
    H = np.asarray(H, dtype=np.int64).reshape(-1, len(src))
    flags = None if lost is None else np.asarray(lost).astype(bool)
    want_out = np.full(out_bytes, CANARY, np.uint8)
    want_rep, want_sums = VP.vread(H, src, A.blocks(img, B), flags, P, table, recs, max_len, want_out)
    d = A.to_dev(torch, img, shift)
    d_out = torch.full((out_bytes,), CANARY, dtype=torch.uint8, device="cuda")
    c0, l0 = V.counters(), V.last_launch()
    with _span(V, span):
        out, rep, sums = call(A.blocks(d, B), flags, P, table, recs, d_out)
        torch.cuda.synchronize()
    c1, l1 = V.counters(), V.last_launch()
    assert out is d_out and rep.dtype == torch.int32 and tuple(rep.shape) == (len(recs), 4)
    g = rep.cpu().numpy().view(np.uint32).astype(np.int64)
    assert np.array_equal(g, want_rep), (P, span, shift, np.argwhere(g != want_rep)[:4].tolist(), g[:12].tolist())
    gs = sums.cpu().numpy().view(np.uint32).astype(np.int64)
    assert gs.shape == want_sums.shape and np.array_equal(gs, want_sums), (P, span, np.argwhere(gs != want_sums)[:6].tolist())
    got_out = d_out.cpu().numpy()
    assert np.array_equal(got_out, want_out), ("answer buffer", np.flatnonzero(got_out != want_out)[:8].tolist())
    assert np.array_equal(d.cpu().numpy(), img), "the arena changed"
    ran = len(recs) > 0 and max_len > 0
    assert c1["launches"] - c0["launches"] == (1 if ran else 0)
    assert c1["records"] - c0["records"] == (len(recs) if ran else 0)
    aligned = shift % 16 == 0 and img.shape[2] % 16 == 0
    assert l1 == (_geometry(P, B, max_len, len(recs), span, 0 if aligned else 1) if ran else l0), l1
    return g, gs, got_out


def _place(recs, classes=(0, 9, 4)):
    """out_off for every record (unaligned classes, canary gaps); returns out_bytes."""
    offs, out_bytes = TG._pack([r[3] for r in recs], classes)
    for rec, at in zip(recs, offs):
        rec[4] = at
    return out_bytes


def _store(oracle, km, seed):
    """An RS store of S0 stripes: stripe 0 whole, 1 one lost data block, 2 m lost, 3 two lost, 4 a lost parity, 5 m + 1
    lost (no lost block of it is recoverable)."""
    k, m, H = TG._rs(oracle, km)
    n = k + m
    stripes = TG._codewords(H, k, S0, B0, seed)
    lost = np.zeros((S0, n), bool)
    lost[1, 1] = True
    lost[2, :m] = True
    lost[3, [0, k]] = True
    lost[4, n - 1] = True
    lost[5, :m + 1] = True
    return k, m, n, H, stripes, lost


_TABLES = {}


def _table(stripes, n, P, key):
    """The recorded table of a store, worked out once per (store, P)."""
    if (key, P) not in _TABLES:
        _TABLES[key, P] = VP.expected_table(stripes, list(range(n)), P)
    return _TABLES[key, P]


def _boundary(P):
    """A piece boundary inside the block (512 where the pieces are not shorter than the block)."""
    return P if 0 < P < B0 else 512


# ---- 1. the record mix on a clean store

@gpu
@pytest.mark.parametrize("P", PIECES, ids=[f"P{p}" for p in PIECES])
@pytest.mark.parametrize("km", TG.RS_CODES, ids=TG.RS_IDS)
def test_record_mix_on_a_clean_store(ecg, oracle, torch_cuda, vread, km, P):
    """Inside one piece, 3 bytes across a piece boundary, three pieces with unaligned off and len, ranges ending at B,
    whole blocks, len 0, present and lost columns, unaligned out_off and states 1, 2, 3, 5, 6, in one call per span.
    State 4 cannot stand beside a whole-block record (len > max_len = B breaks rule 3 first): a second call with
    max_len = 1000 holds it.  Every answered record is state 0, its sums are the table's and its bytes those of
    ecg_dread."""
    import ecg_dread
    torch = torch_cuda
    k, m, n, H, stripes, lost = _store(oracle, km, 11)
    table = _table(stripes, n, P, ("clean", km))
    b = _boundary(P)
    good = [[1, 1, b + 10, 100, 0], [0, 2, b + 10, 100, 0],                      # inside one piece: lost, present
            [2, 0, b - 1, 3, 0], [4, 0, b - 2, 3, 0],                            # 3 bytes across a boundary
            [3, 0, b - 5, min(b + 10, B0 - b), 0], [2, m, 507, 1027, 0],         # unaligned, up to three pieces
            [1, 1, B0 - 37, 37, 0], [4, n - 1, B0 - 700, 700, 0], [0, k, B0 - 1, 1, 0],   # ending at B
            [2, m - 1, 0, B0, 0], [0, n - 1, 0, B0, 0], [3, k, 0, B0, 0],        # whole blocks
            [1, 1, 77, 0, 0], [0, 0, B0, 0, 0], [5, n - 1, 4600, 61, 0]]         # len 0; present in the broken stripe
    slots = [[0, 0, 0, 64, 0] for _ in range(5)]                                 # where the refused records point
    out_bytes = _place(good + slots)
    at = [r[4] for r in slots]
    bad = [[S0, 0, 0, 16, at[0]], [0, n, 32, 16, at[1]], [2, 3, B0 - 15, 16, at[2]], [0, 1, 64, 32, -1],
           [0, 1, 64, 32, out_bytes - 31], [5, 0, 64, 64, at[3]], [5, m, 0, 64, at[4]]]
    states = [1, 2, 3, 5, 5, 6, 6]
    recs = np.array(good + bad, dtype=np.int64)
    order = np.random.default_rng(13).permutation(len(recs))
    where = {int(o): p for p, o in enumerate(order)}
    matrix = [int(v) for v in H[:, :k].reshape(-1)]
    img = TG._arena(stripes, lost)
    call = lambda v, f, p, t, r, o: vread.encode_batch(k, m, matrix, v, f, p, t, r, o, max_len=B0)
    for span in (0, ROW):
        g, sums, out = _run(torch, vread, img, B0, H, list(range(n)), lost, P, table, recs[order], out_bytes, call,
                            span=span)
        assert [int(g[where[len(good) + i], 0]) for i in range(len(bad))] == states
        for i, (s, col, off, ln, at) in enumerate(good):
            row = g[where[i]]
            assert row.tolist() == [0, k if lost[s, col] else 1, 0, VP.NO_PIECE], (i, row)
            q0, npieces, _ = VP.cover(off, ln, P, B0)
            assert sums[where[i], :npieces].tolist() == [int(v) for v in table[s, col, q0:q0 + npieces]], i
            assert np.array_equal(out[at:at + ln], stripes[s, col, off:off + ln]), i
    assert vread.last_launch()["wg_per_record"] == -(-B0 // ROW) == 3
    # the same records through ecg_dread: the same bytes, the same {state, reads}
    d = A.to_dev(torch, img)
    d_out = torch.full((out_bytes,), CANARY, dtype=torch.uint8, device="cuda")
    _, rep = ecg_dread.encode_batch(k, m, matrix, A.blocks(d, B0), lost, recs[order], d_out, max_len=B0)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), out) and np.array_equal(rep.cpu().numpy(), g[:, :2])

    short = [[1, 1, 511, 1000, 0], [3, 2, 17, 1001, 0], [0, 1, 0, 1000, 0], [2, 1, 3000, 1661, 0], [1, 0, 5, 0, 0]]
    out_bytes = _place(short)
    call = lambda v, f, p, t, r, o: vread.encode_batch(k, m, matrix, v, f, p, t, r, o, max_len=1000)
    for span in (0, ROW):
        g, _, _ = _run(torch, vread, img, B0, H, list(range(n)), lost, P, table, short, out_bytes, call, max_len=1000,
                       span=span)
        assert g[:, 0].tolist() == [0, 4, 0, 4, 0]


# ---- 2. damage

@gpu
@pytest.mark.parametrize("P,span", ((512, 0), (512, ROW), (4096, ROW), (0, 0)), ids=("P512", "P512-2048", "P4096-2048", "block"))
@pytest.mark.parametrize("km", TG.RS_CODES, ids=TG.RS_IDS)
def test_damage_is_state_7(ecg, oracle, torch_cuda, vread, km, P, span):
    """One flipped byte (or one wrong recorded sum) per call; the definition gives every record's verdict, and the
    record each case is about is named."""
    torch = torch_cuda
    k, m, n, H, stripes, lost = _store(oracle, km, 21)
    table = _table(stripes, n, P, ("damage", km))
    b = _boundary(P)
    Q = VP.pieces(P, B0)
    piece = lambda x: 0 if P == 0 else x // P
    state, reads, coef, _ = DP.plan(H, lost[1], 1)
    assert state == 0 and reads == k
    sv = int(np.flatnonzero(coef)[0])                                    # a survivor the lost column is rebuilt from
    pc = int(np.flatnonzero(coef)[-1])                                   # another, read as a present column
    assert sv != pc and not lost[1, sv] and not lost[1, pc]
    recs = [[1, 1, b + 10, 100, 0], [1, pc, b + 10, 100, 0], [1, 1, B0 - 20, 20, 0],
            [1, 1, 5, 4200 if b == 4096 else 1100, 0], [0, 2, 0, 64, 0]]
    out_bytes = _place(recs)
    assert piece(5) == 0 and piece(recs[3][2] + recs[3][3] - 1) == min(Q - 1, 1 if b == 4096 else 2)
    matrix = [int(v) for v in H[:, :k].reshape(-1)]
    call = lambda v, f, p, t, r, o: vread.encode_batch(k, m, matrix, v, f, p, t, r, o, max_len=B0)
    clean = TG._arena(stripes, lost)

    def run(flips=(), tab=table):
        img = clean.copy()
        for col, x in flips:
            img[1, col, GUARD + x] ^= 0x20
        return _run(torch, vread, img, B0, H, list(range(n)), lost, P, tab, recs, out_bytes, call, span=span)

    g0, _, out0 = run()
    assert g0[:, 0].tolist() == [0] * 5
    # a survivor, inside record 0's cover but outside its range: state 7, and the answer is what the definition gives
    g, _, out = run([(sv, b + 300)])
    assert g[0].tolist() == [7, k, 1, piece(b + 300)] and g[4, 0] == 0
    assert np.array_equal(out[recs[0][4]:recs[0][4] + 100], out0[recs[0][4]:recs[0][4] + 100])
    # a survivor, outside record 0's cover (with block sums there is no such byte in the block)
    far = 3000 if b == 512 else 200
    g, _, _ = run([(sv, far)])
    assert P == 0 or piece(far) != piece(b + 10)
    assert g[0, 0] == (7 if P == 0 else 0)
    # a present column inside the range
    g, _, out = run([(pc, b + 50)])
    assert g[1].tolist() == [7, 1, 1, piece(b + 50)]
    assert out[recs[1][4] + 40] == out0[recs[1][4] + 40] ^ 0x20                  # the bytes of a state-7 record ARE stored
    # the byte tail of the last piece
    assert B0 - 2 >= (B0 & ~15)
    g, _, _ = run([(sv, B0 - 2)])
    assert g[2].tolist() == [7, k, 1, Q - 1]
    # a wrong recorded sum: state 7 for exactly the records that cover it
    tab = table.copy()
    tab[1, 1, piece(b + 10)] ^= 0x100
    g, _, out = run(tab=tab)
    covering = [i for i, (s, col, off, ln, _) in enumerate(recs)
                if (s, col) == (1, 1) and piece(off) <= piece(b + 10) <= piece(off + ln - 1)]
    assert 0 in covering and 3 in covering and 1 not in covering
    assert [i for i in range(5) if g[i, 0] == 7] == covering and np.array_equal(out, out0)
    assert vread.mismatched_rows(recs, g, P) == VP.mismatched_rows(recs, g, P) != []
    # two bad pieces in one record
    g, _, _ = run([(sv, 100), (sv, b + 100)])
    assert g[3].tolist() == [7, k, min(2, Q), 0]


# ---- 3. an LRC answers from the local group, verified

@gpu
def test_lrc_local_group(torch_cuda, ecg, vread):
    """Azure(8,2,2) with five lost blocks, more than its four parities: a block alone in its local group is answered
    from the group and verified; a block of the group that lost three is state 6."""
    torch = torch_cuda
    k, m, H = TG._check("Azure(8,2,2)")
    n, B, S, P = k + m, B0, 2, 512
    local = [q for q in range(m) if np.count_nonzero(H[q, :k]) == k // 2]
    group = [np.flatnonzero(H[q, :k]).tolist() for q in local]
    glob = [k + q for q in range(m) if q not in local]
    stripes = TG._codewords(H, k, S, B, 31)
    table = VP.expected_table(stripes, list(range(n)), P)
    lost = np.zeros((S, n), bool)
    lost[0, [group[0][1]] + group[1][:3] + [glob[0]]] = True
    recs = [[0, group[0][1], 100, 1000, 0], [0, group[1][0], 100, 1000, 0], [0, group[1][3], 5, 333, 0],
            [1, 2, 0, 64, 0], [0, glob[0], 4600, 61, 0]]
    out_bytes = _place(recs, classes=(9, 0))
    g, _, _ = _run(torch, vread, TG._arena(stripes, lost), B, H, list(range(n)), lost, P, table, recs, out_bytes,
                   lambda v, f, p, t, r, o: vread.matrix_batch(H, list(range(n)), v, f, p, t, r, o, max_len=1000),
                   max_len=1000)
    none = VP.NO_PIECE
    assert g.tolist() == [[0, 4, 0, none], [6, 0, 0, none], [0, 1, 0, none], [0, 1, 0, none], [0, 2, 0, none]]


# ---- 4. no lost flags at all

@gpu
@pytest.mark.parametrize("km", TG.RS_CODES, ids=TG.RS_IDS)
def test_null_lost_is_an_all_zero_lost(torch_cuda, ecg, oracle, vread, km):
    """The ordinary verified read: d_lost = NULL answers as an all-zero d_lost does."""
    torch = torch_cuda
    k, m, H = TG._rs(oracle, km)
    n, S, P = k + m, 3, 2048
    stripes = TG._codewords(H, k, S, B0, 41)
    table = VP.expected_table(stripes, list(range(n)), P)
    zero = np.zeros((S, n), bool)
    recs = [[0, 0, 2047, 3, 0], [1, n - 1, 0, B0, 0], [2, k, 4000, 661, 0], [1, 1, 9, 0, 0], [2, 0, 100, 50, 0]]
    out_bytes = _place(recs)
    img = TG._arena(stripes, zero)
    img[2, 0, GUARD + 1500] ^= 1                                         # damage, so that both calls meet state 7
    call = lambda v, f, p, t, r, o: vread.matrix_batch(H, list(range(n)), v, f, p, t, r, o)
    a = _run(torch, vread, img, B0, H, list(range(n)), None, P, table, recs, out_bytes, call)
    b = _run(torch, vread, img, B0, H, list(range(n)), zero, P, table, recs, out_bytes, call)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert a[0][:, 0].tolist() == [0, 0, 0, 0, 7] and a[0][4].tolist() == [7, 1, 1, 0]


# ---- 5. a check of 72 columns

@gpu
def test_72_columns(torch_cuda, ecg, vread):
    """k = 64, m = 8: the plan's lanes hold two columns each, and a 64-source fold under the CRC."""
    torch = torch_cuda
    k, m, B, S, P = 64, 8, 1077, 2, 512
    n = k + m
    CM = P2.cauchy(m, k)
    H = DP.check_of(CM, k, m)
    stripes = TG._codewords(H, k, S, B, 51)
    table = VP.expected_table(stripes, list(range(n)), P)
    lost = np.zeros((S, n), bool)
    lost[0, [1, 40, 63, 64, 70]] = True
    lost[1, [64, 71]] = True
    recs = [[0, 1, 0, B, 0], [0, 64, 510, 3, 0], [0, 70, 1024, 53, 0], [0, 65, 5, 77, 0], [1, 71, 500, 577, 0],
            [1, 64, 1076, 1, 0]]
    out_bytes = _place(recs, classes=(0, 9))
    img = TG._arena(stripes, lost)
    call = lambda v, f, p, t, r, o: vread.encode_batch(k, m, [int(v) for v in CM.reshape(-1)], v, f, p, t, r, o)
    g, _, _ = _run(torch, vread, img, B, H, list(range(n)), lost, P, table, recs, out_bytes, call)
    assert g[:, :3].tolist() == [[0, k, 0]] * 3 + [[0, 1, 0]] + [[0, k, 0]] * 2
    img[1, 3, GUARD + 1030] ^= 0x80                                      # a survivor's byte in the ragged last piece
    g, _, _ = _run(torch, vread, img, B, H, list(range(n)), lost, P, table, recs, out_bytes, call)
    assert g[4].tolist() == [7, k, 1, 2] and g[5].tolist() == [7, k, 1, 2] and not g[:4, 0].any()


# ---- 6. an unaligned layout

@gpu
@pytest.mark.parametrize("P", (512, 4096, 0), ids=("P512", "P4096", "block"))
def test_unaligned_layout_takes_the_byte_kernel(torch_cuda, ecg, oracle, vread, P):
    """Base + 1: no block is 16-byte aligned and every byte takes the byte kernel; the answers are those of the aligned
    layout, damage included."""
    torch = torch_cuda
    k, m, n, H, stripes, lost = _store(oracle, (4, 2), 61)
    table = VP.expected_table(stripes, list(range(n)), P)
    recs = [[1, 1, 522, 100, 0], [2, 0, 511, 3, 0], [3, k, 0, B0, 0], [0, 2, B0 - 700, 700, 0], [1, 1, 77, 0, 0],
            [5, 0, 64, 64, 0], [4, 0, 4090, 571, 0]]
    out_bytes = _place(recs)
    img = TG._arena(stripes, lost)
    img[4, 0, GUARD + 4659] ^= 4                                         # the last record's last piece
    call = lambda v, f, p, t, r, o: vread.matrix_batch(H, list(range(n)), v, f, p, t, r, o)
    got = [_run(torch, vread, img, B0, H, list(range(n)), lost, P, table, recs, out_bytes, call, shift=shift, span=span)
           for shift, span in ((0, 0), (1, 0), (1, ROW))]
    assert all(np.array_equal(x, y) for g in got[1:] for x, y in zip(g, got[0]))
    assert got[0][0][:, 0].tolist() == [0, 0, 0, 0, 0, 6, 7] and vread.last_launch()["path"] == 1


# ---- 7. nothing to move

@gpu
def test_max_len_zero_and_no_records(torch_cuda, ecg, oracle, vread):
    """max_len == 0: NP = 0, no main launch; records with len > 0 are state 4, empty ones are answered.  R == 0: no
    launch at all."""
    torch = torch_cuda
    k, m, n, H, stripes, lost = _store(oracle, (4, 2), 71)
    table = VP.expected_table(stripes, list(range(n)), 512)
    recs = [[1, 1, 5, 0, 3], [1, 1, 5, 1, 3], [5, 0, 0, 0, 0], [0, 3, 0, 16, 20]]
    call = lambda v, f, p, t, r, o: vread.matrix_batch(H, list(range(n)), v, f, p, t, r, o, max_len=0)
    img = TG._arena(stripes, lost)
    g, sums, _ = _run(torch, vread, img, B0, H, list(range(n)), lost, 512, table, recs, 64, call, max_len=0)
    assert g[:, :2].tolist() == [[0, k], [4, 0], [6, 0], [4, 0]] and sums.shape == (4, 0)
    g, _, _ = _run(torch, vread, img, B0, H, list(range(n)), lost, 512, table, np.zeros((0, 5), np.int64), 64, call,
                   max_len=0)
    assert g.shape == (0, 4)
