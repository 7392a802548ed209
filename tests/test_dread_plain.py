"""tests/dread_plain.py against what include/ecg_dread.h states about the plan rule (CPU, numpy only): over every golden
code with a matrix and m <= 8, every lost set of up to m + 2 columns (at most 300 sampled per size) and every lost
column in it.
"""
import json
import os

import numpy as np
import pytest

import dread_plain as DP
import gf_plain

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
CODES = [c for c in GOLDEN if "matrix" in c and c["m"] <= 8]
MDS = ("RS(", "ERS(")
LIMIT = 300


def cases(c):
    """[(E, col)] of a code: its lost sets of 1..m + 2 columns and every column of each."""
    n = c["k"] + c["m"]
    rng = np.random.default_rng(1000 + n)
    return [(E, col) for t in range(1, c["m"] + 3) for E in DP.lost_sets(n, t, LIMIT, rng) for col in E]


def codeword(H, k, B, seed):
    """[n][B]: random data under H = [G | I]."""
    data = np.random.default_rng(seed).integers(0, 256, (k, B), dtype=np.uint8)
    return np.concatenate([data, gf_plain.apply(H[:, :k], data)])


@pytest.mark.parametrize("c", CODES, ids=[c["name"] for c in CODES])
def test_plan_rule(c):
    k, m = c["k"], c["m"]
    n = k + m
    H = DP.check_of(c["matrix"], k, m)
    word = codeword(H, k, 24, 7 + n)
    assert not gf_plain.apply(H, word).any()
    seen = {0: 0, 6: 0}
    for E, col in cases(c):
        lost = np.zeros(n, bool)
        lost[E] = True
        state, reads, coef, wH = DP.plan(H, lost, col)
        seen[state] += 1
        assert (state == DP.ANSWERED) == DP.recoverable(H, E, col), (E, col)     # the verdict is exact
        if state != DP.ANSWERED:
            assert reads == 0 and not coef.any()
            continue
        assert wH[E].tolist() == [1 if j == col else 0 for j in E], (E, col)    # c restricted to E: the unit vector
        assert not coef[E].any() and reads == np.count_nonzero(coef) >= 1
        if c["name"].startswith(MDS):
            assert reads == k, (E, col, reads)                                   # an MDS code reads k blocks
        garbled = word.copy()
        garbled[E] = 0xEE                                                        # blocks in E are never read
        assert np.array_equal(gf_plain.apply(coef[None, :], garbled)[0], word[col]), (E, col)
    assert seen[0] > 0
    if m >= 2 and not c["name"].startswith("RS(8,1"):
        assert seen[6] > 0                                                       # both verdicts were met


def test_local_reads():
    """One lost data block of an Azure LRC is read from its local group: k / l blocks."""
    for name, want in (("Azure(12,2,2)", 6), ("Azure(8,2,2)", 4)):
        c = next(c for c in GOLDEN if c["name"] == name)
        k, m = c["k"], c["m"]
        H = DP.check_of(c["matrix"], k, m)
        for col in range(k):
            lost = np.zeros(k + m, bool)
            lost[col] = True
            state, reads, coef, _ = DP.plan(H, lost, col)
            assert (state, reads) == (DP.ANSWERED, want), (name, col, reads)


def test_more_losses_than_parities_can_still_be_local():
    """Azure(8,2,2), five lost blocks: a block alone in its local group is answered from the group, reads 4."""
    c = next(c for c in GOLDEN if c["name"] == "Azure(8,2,2)")
    k, m = c["k"], c["m"]
    H = DP.check_of(c["matrix"], k, m)
    found = 0
    for E, col in cases(c):
        if len(E) == 5:
            lost = np.zeros(k + m, bool)
            lost[E] = True
            state, reads, _, _ = DP.plan(H, lost, col)
            found += state == DP.ANSWERED and reads == 4
    assert found > 0


def test_a_present_column_is_a_copy():
    c = next(c for c in GOLDEN if c["name"] == "RS(6,2)")
    H = DP.check_of(c["matrix"], 6, 2)
    lost = np.zeros(8, bool)
    lost[[0, 1, 2, 7]] = True                                                    # more than m lost: a copy all the same
    state, reads, coef, _ = DP.plan(H, lost, 4)
    assert (state, reads) == (DP.ANSWERED, 1) and coef.tolist() == [0, 0, 0, 0, 1, 0, 0, 0]


def test_dread_and_check_records():
    c = next(c for c in GOLDEN if c["name"] == "RS(6,2)")
    k, m, B, S = 6, 2, 40, 2
    H = DP.check_of(c["matrix"], k, m)
    stripes = np.stack([codeword(H, k, B, 90 + s) for s in range(S)])
    lost = np.zeros((S, k + m), bool)
    lost[0, [1, 6]] = True
    lost[1, [0, 2, 3]] = True
    held = stripes.copy()
    held[lost] = 0x99
    recs = [[0, 1, 3, 20, 0], [0, 6, 0, 40, 20], [0, 2, 7, 9, 60], [1, 0, 0, 8, 69], [1, 5, 39, 1, 77], [2, 0, 0, 1, 0],
            [0, 8, 0, 1, 0], [0, 0, 39, 2, 0], [0, 0, 0, 41, 0], [0, 0, 0, 1, 78], [0, 3, 5, 0, 78]]
    out = np.full(78, 0xC3, np.uint8)
    rep = DP.dread(H, list(range(k + m)), held, lost, recs, 40, out)
    assert rep[:, 0].tolist() == [0, 0, 0, 6, 0, 1, 2, 3, 3, 5, 0]
    assert rep[:, 1].tolist() == [k, k, 1, 0, 1, 0, 0, 0, 0, 0, 1]
    want = np.concatenate([stripes[0, 1, 3:23], stripes[0, 6], stripes[0, 2, 7:16], np.full(8, 0xC3, np.uint8),
                           stripes[1, 5, 39:40]])
    assert np.array_equal(out, want)
    assert DP.check_records(recs[:3], k + m, B, S, 40, 78) == -1
    assert DP.check_records(recs, k + m, B, S, 40, 78) == 5
    assert DP.check_records(recs[:3] + [[1, 1, 0, 4, 58]], k + m, B, S, 40, 78) == 3     # [58, 62) meets [60, 69)
    assert DP.check_records(recs[:3] + [[1, 1, 0, 0, 58]], k + m, B, S, 40, 78) == -1    # an empty range overlaps none
    assert DP.check_records(recs[:3], k + m, B, S, 20, 200) == 1                         # 40 bytes > max_len
