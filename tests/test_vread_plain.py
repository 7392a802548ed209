"""tests/vread_plain.py against what include/ecg_vread.h states (CPU, numpy only): the cover's edge cases, the sums of
a present column, the sums of a rebuilt column, state 7 and the precedence of the states.
"""
import json
import os

import numpy as np

import crc32c_plain
import dread_plain as DP
import test_dread_plain as TDP
import vread_plain as VP

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]


def _store(B, S, seed):
    c = next(c for c in GOLDEN if c["name"] == "RS(6,2)")
    k, m = 6, 2
    H = DP.check_of(c["matrix"], k, m)
    stripes = np.stack([TDP.codeword(H, k, B, seed + s) for s in range(S)])
    return k, m, H, stripes


def test_cover_edge_cases():
    B = 4661                                                                     # 9 pieces of 512 and one of 53
    assert VP.pieces(512, B) == 10 and VP.pieces(4096, B) == 2 and VP.pieces(8192, B) == 1 and VP.pieces(0, B) == 1
    assert VP.cover(0, 0, 512, B) == (0, 0, 0) and VP.cover(B, 0, 512, B) == (0, 0, 0)
    assert VP.cover(0, 1, 512, B) == (0, 1, 512) and VP.cover(511, 1, 512, B) == (0, 1, 512)
    assert VP.cover(511, 2, 512, B) == (0, 2, 1024) and VP.cover(510, 3, 512, B) == (0, 2, 1024)
    assert VP.cover(512, 512, 512, B) == (1, 1, 512) and VP.cover(512, 513, 512, B) == (1, 2, 1024)
    assert VP.cover(B - 1, 1, 512, B) == (9, 1, 53)                              # the ragged last piece alone
    assert VP.cover(4607, 54, 512, B) == (8, 2, 512 + 53)                        # off + len == B, two pieces
    assert VP.cover(0, B, 512, B) == (0, 10, B) and VP.cover(0, B, 8192, B) == (0, 1, B)
    assert VP.cover(100, 7, 0, B) == (0, 1, B) and VP.cover(100, 0, 0, B) == (0, 0, 0)
    assert VP.cover(0, 513, 512, 513) == (0, 2, 513) and VP.cover(512, 1, 512, 513) == (1, 1, 1)     # a 1-byte piece
    for P in (0, 512, 1024, 2048, 4096, 8192):
        for ml in (0, 1, 2, 3, 511, 512, 513, 514, 1024, 1025, 1026, 4096, 4098, B):
            want = max((VP.cover(o, ml, P, B)[1] for o in range(B - ml + 1)), default=0)   # every offset
            assert VP.max_pieces(ml, P, B) == want, (P, ml)
    assert not VP.piece_ok(256) and not VP.piece_ok(768) and not VP.piece_ok(1 << 31) and VP.piece_ok(1 << 30)


def test_sums_of_a_present_column_are_the_stored_pieces():
    B, S = 1100, 2
    k, m, H, stripes = _store(B, S, 5)
    n = k + m
    for P in (0, 512, 1024):
        table = VP.expected_table(stripes, list(range(n)), P)
        assert table.shape == (S, n, VP.pieces(P, B))
        for q in range(table.shape[2]):
            lo, hi = VP.bounds(q, P, B)
            assert int(table[1, 3, q]) == crc32c_plain.bitwise(stripes[1, 3, lo:hi])
        recs = [[1, 3, 500, 30, 0], [0, 7, 1099, 1, 30], [0, 0, 0, B, 31]]
        out = np.full(31 + B, 0xC3, np.uint8)
        rep, sums = VP.vread(H, list(range(n)), stripes, None, P, table, recs, B, out)
        assert rep[:, :3].tolist() == [[0, 1, 0]] * 3 and rep[:, 3].tolist() == [VP.NO_PIECE] * 3
        assert np.array_equal(out, np.concatenate([stripes[1, 3, 500:530], stripes[0, 7, 1099:], stripes[0, 0]]))
        for (s, col, off, ln, _), row in zip(recs, sums):
            q0, npieces, _ = VP.cover(off, ln, P, B)
            assert row[:npieces].tolist() == [int(v) for v in table[s, col, q0:q0 + npieces]]
            assert not row[npieces:].any()
        assert sums.shape[1] == VP.max_pieces(B, P, B)


def test_a_rebuilt_column_matches_the_recorded_sums_and_damage_is_state_7():
    B, S, P = 1100, 1, 512
    k, m, H, stripes = _store(B, S, 9)
    n = k + m
    table = VP.expected_table(stripes, list(range(n)), P)
    lost = np.zeros((S, n), bool)
    lost[0, [1, 6]] = True
    held = stripes.copy()
    held[lost] = 0x99
    recs = [[0, 1, 510, 3, 0], [0, 6, 1090, 10, 3], [0, 2, 0, 5, 13]]
    out = np.full(18, 0xC3, np.uint8)
    rep, sums = VP.vread(H, list(range(n)), held, lost, P, table, recs, 10, out)
    assert rep.tolist() == [[0, k, 0, VP.NO_PIECE], [0, k, 0, VP.NO_PIECE], [0, 1, 0, VP.NO_PIECE]]
    assert np.array_equal(out, np.concatenate([stripes[0, 1, 510:513], stripes[0, 6, 1090:], stripes[0, 2, :5]]))
    assert sums.shape == (3, 2) and sums[0].tolist() == [int(v) for v in table[0, 1, :2]]
    # a flipped byte of a survivor in piece 1, outside every range: the records that cover piece 1 are state 7
    held[0, 3, 700] ^= 0x40
    out2 = np.full(18, 0xC3, np.uint8)
    rep2, _ = VP.vread(H, list(range(n)), held, lost, P, table, recs, 10, out2)
    assert rep2.tolist() == [[7, k, 1, 1], [0, k, 0, VP.NO_PIECE], [0, 1, 0, VP.NO_PIECE]]
    assert np.array_equal(out2, out)                                             # the range itself is undamaged
    assert VP.mismatched_rows(recs, rep2, P) == [(0, 1)]
    # a wrong recorded sum: state 7 for exactly the records covering it; two bad pieces in one record
    table2 = table.copy()
    table2[0, 1, 0] ^= 1
    table2[0, 1, 1] ^= 1
    held[0, 3, 700] ^= 0x40
    rep3, _ = VP.vread(H, list(range(n)), held, lost, P, table2, recs, 10, np.full(18, 0xC3, np.uint8))
    assert rep3.tolist() == [[7, k, 2, 0], [0, k, 0, VP.NO_PIECE], [0, 1, 0, VP.NO_PIECE]]
    assert VP.mismatched_rows(recs, rep3, P) == [(0, 0), (0, 1)]


def test_state_precedence():
    """States 1-6 come before 7 and refuse the record as a whole; an empty record covers no piece."""
    B, S, P = 1100, 2, 512
    k, m, H, stripes = _store(B, S, 13)
    n = k + m
    table = VP.expected_table(stripes, list(range(n)), P) ^ np.uint32(1)         # every recorded sum is wrong
    lost = np.zeros((S, n), bool)
    lost[1, [0, 2, 3]] = True                                                    # m + 1 lost
    recs = [[2, n, -1, B + 1, -1], [0, n, -1, 5, 0], [0, 0, 1099, 2, 0], [0, 0, 0, 41, 0], [0, 0, 0, 40, 1],
            [1, 0, 0, 8, 0], [0, 3, 5, 0, 40], [0, 3, 5, 1, 39], [1, 5, 0, 39, 0]]
    out = np.full(40, 0xC3, np.uint8)
    rep, sums = VP.vread(H, list(range(n)), stripes, lost, P, table, recs, 40, out)
    assert rep[:, 0].tolist() == [1, 2, 3, 4, 5, 6, 0, 7, 7]
    assert rep[:, 1].tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 1]
    assert rep[:, 2].tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 1]
    assert rep[:, 3].tolist() == [VP.NO_PIECE] * 7 + [0, 0]
    assert not sums[:7].any()
    want = np.full(40, 0xC3, np.uint8)
    want[39] = stripes[0, 3, 5]
    want[:39] = stripes[1, 5, :39]
    assert np.array_equal(out, want)                                             # state 7: the bytes ARE stored
