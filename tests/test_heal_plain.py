"""The definition of in-place correction (tests/heal_plain.py) on hand cases; no GPU and no library."""
import json
import os

import numpy as np

import gf_plain
import heal_plain as HP
import locate_plain as LP

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
B = 96


def _golden(name):
    return next(c for c in GOLDEN if c["name"] == name)


def _H(c):
    k, m = c["k"], c["m"]
    return np.concatenate([np.asarray(c["matrix"], dtype=np.int64).reshape(m, k), np.eye(m, dtype=np.int64)], axis=1)


def _stripe(c, seed=1):
    k, m = c["k"], c["m"]
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, (k, B), dtype=np.uint8)
    return np.concatenate([data, gf_plain.apply(np.asarray(c["matrix"]).reshape(m, k), data)])


def test_clean_stripe_is_left_alone():
    c = _golden("RS(10,4)")
    H, stripe = _H(c), _stripe(c)
    for target in (None, 3, -1):
        out, rep = HP.heal(H, stripe, target)
        assert np.array_equal(out, stripe) and not rep.any()


def test_single_block_damage_is_restored_exactly():
    c = _golden("RS(10,4)")
    H, stripe = _H(c), _stripe(c)
    n = 14
    for b in (0, 3, 9, 10, 13):                          # data blocks, parity blocks
        bad = stripe.copy()
        bad[b, 40] ^= 0x80
        bad[b, 41] ^= 0x01
        bad[b, 50:60] ^= np.arange(7, 17, dtype=np.uint8)
        bad[b, B - 1] ^= 0xFF
        want = np.zeros(n + 2, np.int64)
        want[b] = want[n] = 13
        for target in (None, b):
            out, rep = HP.heal(H, bad, target)
            assert np.array_equal(out, stripe), (b, target)
            assert np.array_equal(rep, want), (b, target, rep)
            assert LP.verdict(rep) == (b, [b])


def test_any_report_equals_the_locate_votes():
    c = _golden("RS(6,4)")
    H, stripe = _H(c), _stripe(c, 2)
    rng = np.random.default_rng(5)
    stripe[1, 3:20] ^= rng.integers(1, 256, 17, dtype=np.uint8)
    stripe[8, 30:33] ^= 0x11
    stripe[2, 70] ^= 0x5A                                # two blocks at one position: unexplained with r = 4
    stripe[6, 70] ^= 0xC3
    votes = LP.votes(H, stripe)
    assert votes[10] == 21 and votes[11] == 1
    out, rep = HP.heal(H, stripe)
    assert np.array_equal(rep, votes)
    assert rep[:10].sum() + rep[11] == rep[10]
    for t in range(10):                                  # TARGET: report[t] = votes[t], the rest untouched
        _, rt = HP.heal(H, stripe, t)
        want = np.zeros(12, np.int64)
        want[t], want[10], want[11] = votes[t], votes[10], votes[10] - votes[t]
        assert np.array_equal(rt, want), (t, rt)


def test_wrong_and_out_of_range_targets_change_nothing():
    c = _golden("RS(10,4)")
    H, stripe = _H(c), _stripe(c)
    bad = stripe.copy()
    bad[4, 10:20] ^= 0x33
    for target in (5, 0, 13, -1, 14, -7):
        out, rep = HP.heal(H, bad, target)
        assert np.array_equal(out, bad), target
        assert not rep[:14].any() and rep[14] == rep[15] == 10, (target, rep)


def test_six_blocks_at_disjoint_positions_are_all_restored():
    """Six erasures are beyond an RS(10,4) decode; position by position each has one damaged block."""
    c = _golden("RS(10,4)")
    H, stripe = _H(c), _stripe(c, 3)
    bad = stripe.copy()
    rng = np.random.default_rng(6)
    blocks = (0, 2, 5, 9, 11, 13)
    for i, b in enumerate(blocks):
        bad[b, 16 * i:16 * i + 9] ^= rng.integers(1, 256, 9, dtype=np.uint8)
    out, rep = HP.heal(H, bad)
    assert np.array_equal(out, stripe)
    want = np.zeros(16, np.int64)
    want[list(blocks)] = 9
    want[14] = 54
    assert np.array_equal(rep, want)
    assert LP.verdict(rep) == (LP.MULTIPLE, list(blocks))
    out, rep = HP.heal(H, bad, 5)                        # TARGET: only block 5's positions
    fixed = bad.copy()
    fixed[5] = stripe[5]
    assert np.array_equal(out, fixed) and rep[5] == 9 and rep[14] == 54 and rep[15] == 45


def test_two_blocks_at_one_position_with_r_4_are_left_and_counted():
    c = _golden("RS(10,4)")
    H, stripe = _H(c), _stripe(c)
    bad = stripe.copy()
    bad[2, 30] ^= 0x5A
    bad[7, 30] ^= 0xC3
    out, rep = HP.heal(H, bad)
    assert np.array_equal(out, bad)
    want = np.zeros(16, np.int64)
    want[14] = want[15] = 1
    assert np.array_equal(rep, want)
    for target in (2, 7):
        out, rep = HP.heal(H, bad, target)
        assert np.array_equal(out, bad) and np.array_equal(rep, want)


def test_r_1_target_restores_the_named_block():
    c = _golden("RS(8,1)")
    H, stripe = _H(c), _stripe(c)
    bad = stripe.copy()
    bad[5, 17] ^= 0x42
    out, rep = HP.heal(H, bad, 5)
    assert np.array_equal(out, stripe) and list(rep) == [0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0]
    out, rep = HP.heal(H, bad, 6)                        # any block explains an r = 1 syndrome: the wrong one is written
    assert out[6, 17] != bad[6, 17] and rep[6] == 1


def test_zero_column_is_never_corrected():
    H = np.array([[1, 0, 3], [2, 0, 1]])
    stripe = np.zeros((3, 8), np.uint8)
    stripe[1, 2] = 9                                     # damage in the block no row covers: invisible
    stripe[0, 3] = 1
    for target in (None, 1):
        out, rep = HP.heal(H, stripe, target)
        assert out[1, 2] == 9 and rep[1] == 0
    out, rep = HP.heal(H, stripe)
    assert out[0, 3] == 0 and list(rep) == [1, 0, 0, 1, 0]


def test_targets_from_votes():
    votes = np.array([[0, 0, 0, 0, 0], [0, 4, 0, 4, 0], [2, 2, 0, 2, 0], [1, 0, 2, 3, 0], [0, 3, 0, 4, 1],
                      [0, 0, 0, 2, 2], [0, -1, 0, -1, 0]], dtype=np.int32)
    assert list(HP.targets_from_votes(votes)) == [-1, 1, -1, -1, -1, -1, 1]
