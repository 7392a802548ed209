"""tests/usum_plain.py, the plain form the update-sum tests compare with, held on the CPU against the truth: the
CRC-32C of the blocks and pieces of stripes the oracle encoded, before and after tests/update_plain.py changed them.
Test infrastructure only: nothing here loads a library of the project.
"""
import json
import os

import numpy as np
import pytest

import crc32c_plain
import update_plain as UP
import usum_plain as US

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
CODES = ["RS(10,4)", "Azure(8,2,2)", "Azure+1(8,3,2)"]
B = 8 * 1024 + 80                                  # the last piece of 512 and of 2048 bytes has 80 bytes
S = 2


def _code(name):
    c = next(c for c in GOLDEN if c["name"] == name)
    return c["k"], c["m"], [int(v) for v in c["matrix"]]


def _encode(oracle, k, m, M, data):
    out = np.zeros((data.shape[0], k + m, data.shape[2]), np.uint8)
    for s in range(data.shape[0]):
        d = [data[s, j].copy() for j in range(k)]
        c = [np.zeros(data.shape[2], np.uint8) for _ in range(m)]
        oracle.jerasure_matrix_encode(k, m, M, d, c, data.shape[2])
        out[s] = np.stack(d + c)
    return out


def test_arithmetic():
    for data, crc in crc32c_plain.KNOWN:
        d = np.frombuffer(data, np.uint8)
        # crc32c(d) = raw(d) ^ crc32c(0^len)
        assert US.raw(d) ^ crc32c_plain.bitwise(bytes(len(d))) == crc
    rng = np.random.default_rng(1)
    a, b = rng.integers(0, 256, 37, dtype=np.uint8), rng.integers(0, 256, 90, dtype=np.uint8)
    assert US.raw(np.concatenate([a, b])) == US.shift(US.raw(a), 90) ^ US.raw(b)
    assert US.raw(np.concatenate([np.zeros(11, np.uint8), a])) == US.raw(a)
    assert US.shift(US.ONE, 0) == US.ONE and US.mul(US.ONE, 0x12345678) == 0x12345678
    assert US.shift(US.shift(5, (1 << 31) - 40), 40) == US.shift(5, (1 << 31))


@pytest.fixture(scope="module", params=CODES)
def case(request, oracle):
    """Encoded stripes, a legal record set with some records that cross piece borders and reach the block's end, the
    stripes after the update and WRITE mode's delta."""
    k, m, M = _code(request.param)
    rng = np.random.default_rng(len(request.param))
    old = _encode(oracle, k, m, M, rng.integers(0, 256, (S, k, B), dtype=np.uint8))
    recs, in_bytes = UP.legal_records(rng, S, k, B, 5, 3000)
    recs = np.concatenate([recs, [[0, 1, 0, 0, 0]]])                        # an empty record
    new = old.copy()
    data_in = rng.integers(0, 256, in_bytes, dtype=np.uint8)
    tail = max(r[2] + r[3] for r in recs if r[0] == 1)                       # stripe 1: up to the block's last byte
    extra = np.array([[1, k - 1, tail, B - tail, in_bytes]])
    data_in = np.concatenate([data_in, rng.integers(0, 256, B - tail + 3, dtype=np.uint8)])
    recs = np.concatenate([recs, extra])
    delta = np.zeros(data_in.size, np.uint8)
    src, dst = list(range(k)), list(range(k, k + m))
    rep = UP.update(M, src, dst, new, recs, data_in, UP.WRITE, B, delta)
    assert not rep[:, 0].any()
    return dict(k=k, m=m, M=M, src=src, dst=dst, old=old, new=new, recs=recs, delta=delta, rep=rep)


@pytest.mark.parametrize("piece_bytes", [0, 512, 2048])
def test_updated_table_is_the_table_of_the_new_stripes(case, piece_bytes):
    c = case
    ids = list(range(c["k"] + c["m"]))
    table = US.piece_table(c["old"], piece_bytes)
    want = US.piece_table(c["new"], piece_bytes)
    assert not np.array_equal(table, want)
    rep = US.usum(c["M"], c["src"], c["dst"], ids, table, c["recs"], c["delta"], B, B, piece_bytes)
    assert np.array_equal(rep, c["rep"])                                     # nonzero is the update's changed
    assert np.array_equal(table, want)


def test_which_splits_the_table_between_data_and_parity_holders(case):
    c, k = case, case["k"]
    ids = list(range(k + c["m"]))
    old, want = US.piece_table(c["old"], 512), US.piece_table(c["new"], 512)
    data, parity = old.copy(), old.copy()
    US.usum(c["M"], c["src"], c["dst"], ids, data, c["recs"], c["delta"], B, B, 512, US.DATA)
    US.usum(c["M"], c["src"], c["dst"], ids, parity, c["recs"], c["delta"], B, B, 512, US.PARITY)
    assert np.array_equal(data[:, :k], want[:, :k]) and np.array_equal(data[:, k:], old[:, k:])
    assert np.array_equal(parity[:, k:], want[:, k:]) and np.array_equal(parity[:, :k], old[:, :k])
    # a table that names only some blocks, in another order: the others are skipped
    some = [k + 1, 0, k - 1]
    part = np.ascontiguousarray(old[:, some])
    US.usum(c["M"], c["src"], c["dst"], some, part, c["recs"], c["delta"], B, B, 512, US.BOTH)
    assert np.array_equal(part, want[:, some])


def test_refused_records_change_nothing_and_meeting_records_add(case):
    c, k = case, case["k"]
    ids = list(range(k + c["m"]))
    nb = c["delta"].size
    table = US.piece_table(c["old"], 2048)
    before = table.copy()
    bad = [[-1, 0, 0, 4, 0], [S, 0, 0, 4, 0], [0, k, 0, 4, 0], [0, 0, B - 3, 4, 0], [0, 0, -1, 4, 0], [0, 0, 0, 65, 0],
           [0, 0, 0, 4, nb - 3], [0, 0, 0, 4, -1]]
    rep = US.usum(c["M"], c["src"], c["dst"], ids, table, bad, c["delta"], B, 64, 2048)
    assert rep[:, 0].tolist() == [1, 1, 2, 3, 3, 4, 5, 5] and not rep[:, 1].any()
    assert np.array_equal(table, before)
    legal = [[0, 0, 100, 40, 7]]
    rep = US.usum(c["M"], c["src"], c["dst"], ids, table, legal, c["delta"], B, 64, 2048, update_report=[[3, 9]])
    assert rep.tolist() == [[3, 0]] and np.array_equal(table, before)      # the update refused it
    # two records over the same bytes add: the same one twice cancels, two different ones give the sum of both
    twice = [[0, 0, 100, 40, 7], [0, 0, 100, 40, 7]]
    US.usum(c["M"], c["src"], c["dst"], ids, table, twice, c["delta"], B, 64, 2048)
    assert np.array_equal(table, before)
    both = [[0, 0, 100, 40, 7], [0, 3, 120, 30, 900]]
    one_by_one = before.copy()
    US.usum(c["M"], c["src"], c["dst"], ids, table, both, c["delta"], B, 64, 2048)
    for r in both:
        US.usum(c["M"], c["src"], c["dst"], ids, one_by_one, [r], c["delta"], B, 64, 2048)
    assert np.array_equal(table, one_by_one) and not np.array_equal(table, before)
    assert US.traffic_bytes([4] * k, both, B, 2048, US.BOTH) == 40 + 30 + 8 * 2 * 5
