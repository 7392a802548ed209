"""tests/update_plain.py, the plain form the GPU update tests compare with, checked on the CPU against the oracle's
encode: after any legal record set the parities are the encode of the new data.  Test infrastructure only: nothing here
loads a library of the project.
"""
import json
import os

import numpy as np
import pytest

import update_plain as UP

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
CODES = ["RS(10,4)", "Azure(8,2,2)", "Azure+1(8,3,2)"]


def _code(name):
    c = next(c for c in GOLDEN if c["name"] == name)
    return c["k"], c["m"], [int(v) for v in c["matrix"]]


def _encode(oracle, k, m, M, data):
    """[S][k][B] data -> [S][k+m][B] stripes, parity by the oracle's encode."""
    S, _, B = data.shape
    out = np.zeros((S, k + m, B), np.uint8)
    for s in range(S):
        d = [data[s, j].copy() for j in range(k)]
        c = [np.zeros(B, np.uint8) for _ in range(m)]
        oracle.jerasure_matrix_encode(k, m, M, d, c, B)
        out[s] = np.stack(d + c)
    return out


@pytest.mark.parametrize("name", CODES)
def test_write_keeps_the_stripe_a_codeword(oracle, name):
    k, m, M = _code(name)
    S, B = 3, 211
    rng = np.random.default_rng(len(name))
    stripes = _encode(oracle, k, m, M, rng.integers(0, 256, (S, k, B), dtype=np.uint8))
    before = stripes.copy()
    recs, in_bytes = UP.legal_records(rng, S, k, B, 6, 64)
    assert UP.check_records(recs, k, B, S, 64, in_bytes, True) == -1
    data_in = rng.integers(0, 256, in_bytes, dtype=np.uint8)
    delta = np.full(in_bytes, 0xEE, np.uint8)
    src, dst = list(range(k)), list(range(k, k + m))
    rep = UP.update(M, src, dst, stripes, recs, data_in, UP.WRITE, 64, delta)
    assert not rep[:, 0].any()
    want = before[:, :k].copy()
    covered = np.zeros(in_bytes, bool)
    for s, col, off, ln, in_off in recs:
        want[s, col, off:off + ln] = data_in[in_off:in_off + ln]
        covered[in_off:in_off + ln] = True
    assert np.array_equal(stripes[:, :k], want)
    assert np.array_equal(stripes, _encode(oracle, k, m, M, want))       # the parities: the oracle's encode
    assert (delta[~covered] == 0xEE).all()
    assert rep[:, 1].sum() == np.count_nonzero(before[:, :k] != want)

    # DELTA mode fed with WRITE mode's delta: the same parities, the data left alone
    again = before.copy()
    rep2 = UP.update(M, src, dst, again, recs, delta, UP.DELTA, 64)
    assert np.array_equal(again[:, k:], stripes[:, k:]) and np.array_equal(again[:, :k], before[:, :k])
    assert np.array_equal(rep2, rep)


def test_refused_records_leave_every_byte_alone(oracle):
    k, m, M = _code("RS(10,4)")
    S, B, max_len, in_bytes = 2, 100, 40, 64
    rng = np.random.default_rng(5)
    stripes = _encode(oracle, k, m, M, rng.integers(0, 256, (S, k, B), dtype=np.uint8))
    data_in = rng.integers(0, 256, in_bytes, dtype=np.uint8)
    bad = {UP.BAD_STRIPE: [[-1, 0, 0, 4, 0], [S, 0, 0, 4, 0]],
           UP.BAD_COL: [[0, -1, 0, 4, 0], [0, k, 0, 4, 0]],
           UP.BAD_RANGE: [[0, 0, -1, 4, 0], [0, 0, 0, -1, 0], [0, 0, B - 3, 4, 0], [0, 0, B + 1, 0, 0]],
           UP.TOO_LONG: [[0, 0, 0, max_len + 1, 0]],
           UP.BAD_STAGING: [[0, 0, 0, 4, -1], [0, 0, 0, 4, in_bytes - 3], [0, 0, 0, 0, in_bytes + 1]]}
    for state, recs in bad.items():
        for rec in recs:
            got, delta = stripes.copy(), np.full(in_bytes, 0xEE, np.uint8)
            for mode, dl in ((UP.WRITE, delta), (UP.DELTA, None)):
                rep = UP.update(M, list(range(k)), list(range(k, k + m)), got, [rec], data_in, mode, max_len, dl)
                assert rep.tolist() == [[state, 0]], rec
            assert np.array_equal(got, stripes) and (delta == 0xEE).all()
            assert UP.check_records([[1, 1, 0, 4, 0], rec], k, B, S, max_len, in_bytes) == 1
    # the order of the rules: a record that breaks several is given the first
    assert UP.state_of([S, k, -1, max_len + 1, -1], k, B, S, max_len, in_bytes) == UP.BAD_STRIPE
    assert UP.state_of([0, k, -1, max_len + 1, -1], k, B, S, max_len, in_bytes) == UP.BAD_COL
    assert UP.state_of([0, 0, 0, max_len + 1, -1], k, B, S, max_len, in_bytes) == UP.TOO_LONG
    assert UP.state_of([0, 0, B, 0, in_bytes], k, B, S, max_len, in_bytes) == UP.APPLIED      # empty, at the ends


def test_check_records_and_traffic():
    k, B, S = 4, 64, 3
    ok = [[0, 0, 0, 5, 0], [0, 1, 5, 4, 5], [1, 0, 0, 5, 9], [0, 2, 20, 0, 0]]          # touching; another stripe; empty
    assert UP.check_records(ok, k, B, S, 16, 32, True) == -1
    assert UP.check_records(ok + [[0, 3, 8, 2, 20]], k, B, S, 16, 32) == 4               # [8,10) meets [5,9)
    assert UP.check_records(ok + [[2, 3, 8, 2, 13]], k, B, S, 16, 32) == -1              # staging is not compared ...
    assert UP.check_records(ok + [[2, 3, 8, 2, 13]], k, B, S, 16, 32, True) == 4         # ... unless delta is written
    assert UP.check_records([[0, 0, 4, 4, 0], [0, 0, 0, 16, 8]], k, B, S, 16, 32) == 1   # a range inside another
    nnz = [4, 0, 2, 1]
    recs = [[0, 0, 0, 10, 0], [0, 1, 10, 3, 10], [1, 3, 0, 7, 13], [1, 2, 9, 0, 20]]
    assert UP.traffic_bytes(nnz, recs, UP.WRITE) == 10 * 11 + 3 * 3 + 7 * 5
    assert UP.traffic_bytes(nnz, recs, UP.WRITE, True) == 10 * 12 + 3 * 4 + 7 * 6
    assert UP.traffic_bytes(nnz, recs, UP.DELTA) == 10 * 9 + 3 * 1 + 7 * 3
