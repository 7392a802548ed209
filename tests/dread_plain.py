"""The degraded range read from its definition (include/ecg_dread.h), numpy over tests/gf_plain.py's table and
tests/restore_plain.py's `reduce` (test helper: imports nothing of the project).

`plan` is the header's plan rule read line by line: the rows are put in the order of step 1 as an actual permutation of
H, the matrix [H | I] is eliminated in place with scalar row operations and the row transform is read off its right
half -- not the packed transform-only form of the kernel.  `recoverable` is the rank criterion the header states beside
the rule, over restore_plain's elimination with row swaps; `dread` answers records into a buffer one byte range at a
time; `check_records` restates the host helper.
"""
import numpy as np

import gf_plain
import restore_plain

ANSWERED, BAD_STRIPE, BAD_COL, BAD_RANGE, TOO_LONG, BAD_OUT, UNRECOVERABLE = range(7)
MUL = gf_plain.TABLE


def check_of(matrix, k, m):
    """H = [matrix | I], m x (k + m)."""
    return np.concatenate([np.asarray(matrix, dtype=np.int64).reshape(m, k), np.eye(m, dtype=np.int64)], axis=1)


def recoverable(H, E, col):
    """A w with w * H_E = unit_col exists iff rank H_E > rank H_{E \\ col}."""
    H = np.asarray(H, dtype=np.int64)
    E = sorted(int(j) for j in E)
    rest = [j for j in E if j != col]
    return restore_plain.rank(H[:, E]) > (restore_plain.rank(H[:, rest]) if rest else 0)


def plan(H, lost, col):
    """(state, reads, c, wH): state 0 or 6; c[j] for the survivors (0 on E and everywhere in state 6); wH = w * H over
    all n columns (None where col found no pivot), so that a caller can look at it on E."""
    H = np.asarray(H, dtype=np.int64)
    r, n = H.shape
    lost = np.asarray(lost).astype(bool)
    c = np.zeros(n, np.int64)
    if not lost[col]:
        c[col] = 1
        return ANSWERED, 1, c, c.copy()
    E = [int(j) for j in np.flatnonzero(lost)]
    outside = np.count_nonzero(H[:, ~lost], axis=1)
    order = sorted(range(r), key=lambda q: (int(outside[q]), q))                 # step 1
    A = np.concatenate([H[order], np.eye(r, dtype=np.int64)[order]], axis=1)   # [H | T] with T * H = the left half
    used = [False] * r
    pivot_of = {}
    for e in E:                                                                  # step 2
        p = next((i for i in range(r) if not used[i] and A[i, e]), None)
        if p is None:
            continue
        used[p] = True
        pivot_of[e] = p
        A[p] = MUL[restore_plain.inv(int(A[p, e]))][A[p]]
        for i in range(r):
            if i != p and A[i, e]:
                A[i] ^= MUL[int(A[i, e])][A[p]]
    if col not in pivot_of:                                                      # step 3
        return UNRECOVERABLE, 0, c, None
    w = A[pivot_of[col], n:]
    wH = gf_plain.apply(w[None, :], H.astype(np.uint8))[0].astype(np.int64)
    assert np.array_equal(wH, A[pivot_of[col], :n])
    unit = np.zeros(len(E), np.int64)
    unit[E.index(col)] = 1
    if not np.array_equal(wH[E], unit):
        return UNRECOVERABLE, 0, c, wH
    c[~lost] = wH[~lost]                                                         # step 4
    return ANSWERED, int(np.count_nonzero(c)), c, wH


def state_of(rec, n, B, S, max_len, out_bytes):
    """States 1-5 of one record: the first rule it breaks."""
    stripe, col, off, ln, out_off = (int(v) for v in rec)
    if not 0 <= stripe < S:
        return BAD_STRIPE
    if not 0 <= col < n:
        return BAD_COL
    if off < 0 or ln < 0 or off + ln > B:
        return BAD_RANGE
    if ln > max_len:
        return TOO_LONG
    if out_off < 0 or out_off + ln > out_bytes:
        return BAD_OUT
    return ANSWERED


def dread(H, src_ids, stripes, lost, records, max_len, out):
    """Answer the records over stripes ([S][slots][B] uint8, column j of H is slot src_ids[j]; never written) into out
    (1-D uint8, changed in place).  lost: [S][n] flags.  Returns the (R, 2) report {state, reads}."""
    H = np.asarray(H, dtype=np.int64).reshape(-1, len(src_ids))
    n = H.shape[1]
    S, _, B = stripes.shape
    report = np.zeros((len(records), 2), np.int64)
    for i, rec in enumerate(records):
        st = state_of(rec, n, B, S, max_len, out.size)
        if st == ANSWERED:
            s, col, off, ln, out_off = (int(v) for v in rec)
            st, reads, c, _ = plan(H, lost[s], col)
        report[i, 0] = st
        if st != ANSWERED:
            continue
        report[i, 1] = reads
        acc = np.zeros(ln, np.uint8)
        for j in np.flatnonzero(c):
            assert not lost[s][j]                                                # blocks in E are never read
            acc ^= MUL[int(c[j])][stripes[s, src_ids[j], off:off + ln]]
        out[out_off:out_off + ln] = acc
    return report


def _overlaps(a, b):
    """Two half-open ranges share a byte (an empty range shares none)."""
    return a[0] < a[1] and b[0] < b[1] and a[0] < b[1] and b[0] < a[1]


def check_records(records, n, B, S, max_len, out_bytes):
    """-1 if no record breaks a rule 1-5 and the out ranges are pairwise disjoint; else the index of the first record
    that is refused or whose out range overlaps that of a record before it."""
    seen = []
    for i, rec in enumerate(records):
        if state_of(rec, n, B, S, max_len, out_bytes) != ANSWERED:
            return i
        _, _, _, ln, out_off = (int(v) for v in rec)
        if any(_overlaps((out_off, out_off + ln), p) for p in seen):
            return i
        seen.append((out_off, out_off + ln))
    return -1


def lost_sets(n, t, limit, rng):
    """Every lost set of size t over n columns if there are at most `limit`, else `limit` sampled ones (distinct)."""
    from itertools import combinations
    from math import comb
    if comb(n, t) <= limit:
        return [list(E) for E in combinations(range(n), t)]
    seen = set()
    while len(seen) < limit:
        seen.add(tuple(sorted(int(v) for v in rng.choice(n, t, replace=False))))
    return [list(E) for E in sorted(seen)]
