"""The verified range read from its definition (include/ecg_vread.h), numpy over tests/dread_plain.py (records, states
1-6, the plan rule) and tests/crc32c_plain.py (test helper: imports nothing of the project).

`cover` and `max_pieces` are the header's two host helpers; `expected_table` is the store's recorded table, the CRC-32C
of every piece of every block; `vread` answers records into a buffer one range at a time: the column over the whole
cover, its pieces' sums, the range's bytes, and the report {state, reads, bad, first_bad}.
"""
import numpy as np

import crc32c_plain
import dread_plain as DP

MISMATCH = 7
NO_PIECE = 0xFFFFFFFF
MIN_PIECE, MAX_PIECE = 512, 1 << 30


def piece_ok(piece_bytes):
    return piece_bytes == 0 or (MIN_PIECE <= piece_bytes <= MAX_PIECE and piece_bytes & (piece_bytes - 1) == 0)


def pieces(piece_bytes, B):
    """Q: the sums a block has in the table."""
    return 1 if piece_bytes == 0 else max(1, -(-B // piece_bytes))


def bounds(q, piece_bytes, B):
    """The bytes [lo, hi) of piece q of a B-byte block."""
    if piece_bytes == 0:
        return 0, B
    return q * piece_bytes, min((q + 1) * piece_bytes, B)


def cover(off, ln, piece_bytes, B):
    """(q0, npieces, cover_bytes) of bytes [off, off + ln) of a B-byte block; all zero for an empty range."""
    assert piece_ok(piece_bytes) and 0 <= off and 0 <= ln and off + ln <= B
    if ln == 0:
        return 0, 0, 0
    if piece_bytes == 0:
        return 0, 1, B
    q0, q1 = off // piece_bytes, (off + ln - 1) // piece_bytes
    return q0, q1 - q0 + 1, bounds(q1, piece_bytes, B)[1] - bounds(q0, piece_bytes, B)[0]


def max_pieces(max_len, piece_bytes, B):
    """The most pieces a range of max_len bytes inside a B-byte block can cover, by trying every offset that matters:
    the last byte of a piece, and the last offset the block allows."""
    assert piece_ok(piece_bytes) and 0 <= max_len <= B
    if max_len == 0:
        return 0
    if piece_bytes == 0:
        return 1
    offs = {B - max_len} | {o for o in range(piece_bytes - 1, B - max_len + 1, piece_bytes)}
    return max(cover(o, max_len, piece_bytes, B)[1] for o in offs)


def expected_table(stripes, src_ids, piece_bytes):
    """[S][n][Q] uint32: the CRC-32C of every piece of column j (slot src_ids[j]) of every stripe."""
    S, _, B = stripes.shape
    Q = pieces(piece_bytes, B)
    table = np.zeros((S, len(src_ids), Q), np.uint32)
    for q in range(Q):
        lo, hi = bounds(q, piece_bytes, B)
        table[:, :, q] = crc32c_plain.many(stripes[:, list(src_ids), lo:hi])
    return table


def vread(H, src_ids, stripes, lost, piece_bytes, expected, records, max_len, out):
    """Answer the records over stripes ([S][slots][B] uint8, column j of H is slot src_ids[j]; never written) into out
    (1-D uint8, changed in place).  lost: [S][n] flags or None.  expected: [S][n][Q].  Returns (report, sums): the
    (R, 4) report {state, reads, bad, first_bad} and the (R, NP) computed sums, both int64."""
    H = np.asarray(H, dtype=np.int64).reshape(-1, len(src_ids))
    n = H.shape[1]
    S, _, B = stripes.shape
    if lost is None:
        lost = np.zeros((S, n), bool)
    NP = max_pieces(max_len, piece_bytes, B)
    report = np.zeros((len(records), 4), np.int64)
    report[:, 3] = NO_PIECE
    sums = np.zeros((len(records), NP), np.int64)
    for i, rec in enumerate(records):
        st = DP.state_of(rec, n, B, S, max_len, out.size)
        if st == DP.ANSWERED:
            s, col, off, ln, out_off = (int(v) for v in rec)
            st, reads, c, _ = DP.plan(H, lost[s], col)
        report[i, 0] = st
        if st != DP.ANSWERED:
            continue
        report[i, 1] = reads
        q0, npieces, cover_bytes = cover(off, ln, piece_bytes, B)
        lo = bounds(q0, piece_bytes, B)[0]
        value = np.zeros(cover_bytes, np.uint8)                                  # the column over the whole cover
        for j in np.flatnonzero(c):
            assert not lost[s][j]                                                # blocks in E are never read
            value ^= DP.MUL[int(c[j])][stripes[s, src_ids[j], lo:lo + cover_bytes]]
        for p in range(npieces):
            a, b = bounds(q0 + p, piece_bytes, B)
            sums[i, p] = crc32c_plain.bitwise(value[a - lo:b - lo])
            if sums[i, p] != int(expected[s, col, q0 + p]):
                if report[i, 2] == 0:
                    report[i, 3] = q0 + p
                report[i, 2] += 1
        if report[i, 2]:
            report[i, 0] = MISMATCH
        out[out_off:out_off + ln] = value[off - lo:off - lo + ln]                # stored also in state 7
    return report, sums


def mismatched_rows(records, report, piece_bytes):
    """The sorted (stripe, q) pairs from the first bad piece to the end of the cover of every state-7 record."""
    rows = set()
    for rec, rep in zip(records, report):
        if int(rep[0]) != MISMATCH:
            continue
        s, _, off, ln, _ = (int(v) for v in rec)
        last = 0 if piece_bytes == 0 else (off + ln - 1) // piece_bytes
        rows.update((s, q) for q in range(int(rep[3]), last + 1))
    return sorted(rows)
