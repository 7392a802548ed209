"""tests/heal2_plain.py, the numpy restatement of two-block correction, on hand cases (no GPU, no library)."""
import numpy as np
import pytest

import gf_plain
import heal2_plain as P
import heal_plain as HP

mul = gf_plain.mul


def _mds(r, k, seed=0):
    """[C | I] with C an r x k Cauchy matrix: every r columns are independent."""
    return np.concatenate([P.cauchy(r, k, seed), np.eye(r, dtype=np.int64)], axis=1)


def _consistent(H, B, seed):
    """One stripe that satisfies H = [C | I]: random data, parity = C * data."""
    r, n = H.shape
    data = np.random.default_rng(seed).integers(0, 256, (n - r, B), dtype=np.uint8)
    stripe = np.concatenate([data, gf_plain.apply(H[:, :n - r], data)])
    assert not gf_plain.apply(H, stripe).any()
    return stripe


# a deliberately dependent check: column 3 = column 0 ^ column 1 ^ column 2, every 3 columns still independent
H_DEP4 = _mds(4, 3, seed=5)[:, :3]
H_DEP4 = np.concatenate([H_DEP4, (H_DEP4[:, 0] ^ H_DEP4[:, 1] ^ H_DEP4[:, 2])[:, None], np.eye(4, dtype=np.int64)[:, :2]],
                        axis=1)
# and one with a dependent triple: column 2 = column 0 ^ 2 * column 1
H_DEP3 = np.array([[1, 1, 1 ^ 2, 1], [1, 2, 1 ^ 4, 4], [1, 4, 1 ^ 8, 16], [1, 8, 1 ^ 16, 64]], dtype=np.int64)


def test_rank_and_independence():
    assert P.rank([[1, 2], [2, 4]]) == 1 and P.rank([[1, 2], [2, 5]]) == 2 and P.rank([[0, 0], [0, 0]]) == 0
    assert P.rank(np.eye(5, dtype=np.int64)) == 5 and P.rank([[3, 0, 0]]) == 1
    assert mul(2, 0x80) == 0x1D                                  # the field, not the integers
    assert P.rank([[1, 2], [0x80, 0x1D]]) == 1
    for r in (3, 4, 5):
        H = _mds(r, 4, seed=r)
        assert P.independent(H, r) and not P.independent(H, r + 1)
    assert P.independent(H_DEP4, 3) and P.dependent_set(H_DEP4, 4) == (0, 1, 2, 3)
    assert P.independent(H_DEP3, 2) and P.dependent_set(H_DEP3, 3) == (0, 1, 2)
    Hz = _mds(4, 3)
    Hz[:, 1] = 0
    assert P.dependent_set(Hz, 3) == (0, 1, 2) and not P.independent(Hz, 1)
    assert P.accepts(_mds(4, 6), True) and P.accepts(_mds(3, 6), False) and not P.accepts(_mds(3, 6), True)
    assert not P.accepts(_mds(2, 6), False) and not P.accepts(H_DEP4, True) and P.accepts(H_DEP4, False)
    assert not P.accepts(H_DEP3, False) and not P.accepts(_mds(4, 29), True) and P.accepts(_mds(4, 28), True)
    assert P.independent(np.array([[1], [1], [1]]), 4)           # fewer columns than k: all of them


def test_families():
    assert P.family(4, None) == ([0, 1, 2, 3], [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)])
    assert P.family(4, 2) == ([0, 1, 2, 3], [(0, 2), (1, 2), (2, 3)])
    assert P.family(4, 4) == P.family(4, -1) == ([], [])


def test_a_dependent_check_gives_two_explanations():
    """s = 7 * (h_0 ^ h_1) = 7 * (h_2 ^ h_3) under H_DEP4: two pairs explain it, and a library that accepted this H
    in ANY2 could not know which to write.  TARGET2 with t = 0 admits only the first; an independent H has one."""
    s = np.array([mul(7, int(a) ^ int(b)) for a, b in zip(H_DEP4[:, 0], H_DEP4[:, 1])], dtype=np.uint8)
    assert P.explanations(H_DEP4, s) == [{0: 7, 1: 7}, {2: 7, 3: 7}]
    assert P.explanations(H_DEP4, s, target=0) == [{0: 7, 1: 7}]
    assert P.explanations(H_DEP4, s, target=4) == [] and P.explanations(H_DEP4, s, target=9) == []
    with pytest.raises(AssertionError):
        P.heal2(H_DEP4, np.zeros((6, 4), np.uint8))
    # a dependent triple: a single is also a pair
    s = np.array([mul(9, int(v)) for v in H_DEP3[:, 2]], dtype=np.uint8)
    assert P.explanations(H_DEP3, s) == [{2: 9}, {0: 9, 1: mul(9, 2)}]
    H = _mds(4, 4, seed=2)
    s = np.array([mul(7, int(a)) ^ mul(0x91, int(b)) for a, b in zip(H[:, 1], H[:, 6])], dtype=np.uint8)
    assert P.explanations(H, s) == [{1: 7, 6: 0x91}]
    assert P.explanations(H, np.zeros(4, np.uint8)) == []


def test_heal2_on_planted_damage():
    H = _mds(5, 4, seed=3)                                       # n = 9, every 5 columns independent
    n, B = 9, 64
    clean = _consistent(H, B, 1)
    stripe = clean.copy()
    stripe[2, 3] ^= 0x11                                         # a single
    stripe[0, 10] ^= 0x22                                        # a pair (table, identity) ...
    stripe[7, 10] ^= 0x33
    stripe[0, 11] ^= 0x44                                        # ... and next to it a pair that shares block 0
    stripe[4, 11] ^= 0x55
    stripe[5, 40] ^= 1                                           # (identity, identity)
    stripe[8, 40] ^= 0xFF
    stripe[[1, 3, 6], 50] ^= np.array([5, 6, 7], np.uint8)       # three blocks: r = 5 leaves it alone
    out, rep = P.heal2(H, stripe)
    want = clean.copy()
    want[[1, 3, 6], 50] = stripe[[1, 3, 6], 50]
    assert np.array_equal(out, want)
    assert rep.tolist() == [2, 0, 1, 0, 1, 1, 0, 1, 1, 5, 1, 3]
    assert rep[:n].sum() - rep[n + 2] + rep[n + 1] == rep[n]
    # every correction agrees with the enumeration over every pair of values
    syn = gf_plain.apply(H, stripe)
    for x in (3, 10, 11, 40, 50):
        ex = P.explanations(H, syn[:, x])
        assert len(ex) == (0 if x == 50 else 1)
        for A in ex:
            for b, e in A.items():
                assert out[b, x] == stripe[b, x] ^ e
    # TARGET2 on block 0: its two pairs and every single; the (5, 8) pair stays
    out, rep = P.heal2(H, stripe, target=0)
    want[[5, 8], 40] = stripe[[5, 8], 40]
    assert np.array_equal(out, want) and rep.tolist() == [2, 0, 1, 0, 1, 0, 0, 1, 0, 5, 2, 2]
    # a target that names no block: nothing
    for t in (-1, n, 1 << 20):
        out, rep = P.heal2(H, stripe, target=t)
        assert np.array_equal(out, stripe) and rep.tolist() == [0] * n + [5, 5, 0]
    out, rep = P.heal2(H, clean)
    assert np.array_equal(out, clean) and not rep.any()


def test_singles_only_is_the_heal():
    H = _mds(4, 6, seed=4)
    stripes = np.stack([_consistent(H, 200, s) for s in range(3)])
    rng = np.random.default_rng(9)
    for s, b, lo in ((1, 0, 0), (1, 7, 50), (2, 9, 120), (2, 3, 199)):
        stripes[s, b, lo:lo + 30] ^= rng.integers(1, 256, min(30, 200 - lo), dtype=np.uint8)
    out2, rep2 = P.heal2_stripes(H, stripes)
    out1, rep1 = HP.heal_stripes(H, stripes)
    assert np.array_equal(out2, out1) and np.array_equal(rep2[:, :12], rep1) and not rep2[:, 12].any()
    assert not gf_plain.apply(H, out2[1]).any()


def test_garbage_block_plus_a_run_with_r3():
    """TARGET2 over r = 3: block 2 garbage and named, a run in block 5; with the wrong target the overlap stays."""
    H = _mds(3, 5, seed=6)
    assert P.independent(H, 3)
    clean = _consistent(H, 300, 7)
    stripe = clean.copy()
    rng = np.random.default_rng(8)
    stripe[2] = rng.integers(0, 256, 300, dtype=np.uint8)
    stripe[5, 100:140] ^= rng.integers(1, 256, 40, dtype=np.uint8)
    out, rep = P.heal2(H, stripe, target=2)
    assert np.array_equal(out, clean)
    overlap = np.count_nonzero(stripe[2, 100:140] != clean[2, 100:140])
    assert rep[10] == overlap and rep[5] == 40 and rep[9] == 0 and rep[2] == np.count_nonzero(stripe[2] != clean[2])
    out, rep = P.heal2(H, stripe, target=4)                      # r = 3: a wrong name may also miscorrect
    assert rep[:8].sum() - rep[10] + rep[9] == rep[8]
