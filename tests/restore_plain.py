"""Named-block restoration from its definition (test helper, numpy only, on top of tests/gf_plain.py).

For a check matrix H (r x n over GF(2^8) / 0x11d), one stripe of n blocks of B bytes with s[x] = H * v[x], and flags
over the n blocks, E = the flagged blocks, t = |E|:
    state 0  1 <= t <= r and the columns H[:, E] are independent,   1  t = 0,   2  t > r,   3  dependent columns;
    in state 0, for every bad x (s[x] != 0) with an e such that H_E * e = s[x]:  v_b[x] ^= e_b for b in E, e_b != 0;
    report[b] = positions corrected in block b (b < n), report[n] = bad positions, report[n + 1] = bad positions left
    untouched, report[n + 2] = the state.
The elimination here is on H[:, E] alone, independent of the positions (plain Gaussian elimination with the first
nonzero row as pivot and row swaps -- not the kernels' swap-free form, and over tests/gf_plain.py's table, not the
library's).  `restore` then PROVES its answer by the definition before it returns it: gf_plain.apply(H[:, E], e) == s
wherever it corrected, and rank [H_E | s] = t + 1 -- no solution -- wherever it left a bad position alone.
"""
import numpy as np

import gf_plain

USABLE, NONE_FLAGGED, TOO_MANY, DEPENDENT = 0, 1, 2, 3


def inv(a):
    """1 / a by search over the multiplication table."""
    assert a != 0
    return int(np.flatnonzero(gf_plain.TABLE[a] == 1)[0])


def reduce(M):
    """Row-reduce a copy of M (rows x cols, ints) over all its columns.  Returns (reduced, transform T with
    T * M = reduced, pivot columns): plain Gauss-Jordan with row swaps."""
    M = np.array(M, dtype=np.int64)
    rows, cols = M.shape
    A = np.concatenate([M, np.eye(rows, dtype=np.int64)], axis=1)
    pivots, top = [], 0
    for c in range(cols):
        nz = [q for q in range(top, rows) if A[q, c]]
        if not nz:
            continue
        A[[top, nz[0]]] = A[[nz[0], top]]
        A[top] = gf_plain.TABLE[inv(int(A[top, c]))][A[top]]
        for q in range(rows):
            if q != top and A[q, c]:
                A[q] ^= gf_plain.TABLE[int(A[q, c])][A[top]]
        pivots.append(c)
        top += 1
        if top == rows:
            break
    return A[:, :cols], A[:, cols:], pivots


def rank(M):
    return len(reduce(M)[2])


def state_of(H, flags):
    H = np.asarray(H, dtype=np.int64)
    r = H.shape[0]
    E = [int(j) for j in np.flatnonzero(np.asarray(flags))]
    if not E:
        return NONE_FLAGGED, E
    if len(E) > r:
        return TOO_MANY, E
    return (USABLE if rank(H[:, E]) == len(E) else DEPENDENT), E


def restore(H, stripe, flags):
    """H: r x n; stripe: [n][B] uint8; flags: n values, nonzero = flagged.  Returns (restored [n][B] copy, report:
    n + 3 counters as an int64 array)."""
    H = np.asarray(H, dtype=np.int64)
    r, n = H.shape
    stripe = np.asarray(stripe, dtype=np.uint8)
    assert stripe.shape[0] == n and len(flags) == n
    out = stripe.copy()
    syn = gf_plain.apply(H, stripe)                      # [r][B]
    bad = np.flatnonzero(syn.any(axis=0))
    report = np.zeros(n + 3, np.int64)
    state, E = state_of(H, flags)
    report[n] = bad.size
    report[n + 2] = state
    if state != USABLE or not bad.size:
        report[n + 1] = bad.size
        return out, report
    t = len(E)
    HE = H[:, E]
    red, T, piv = reduce(HE)                             # red = [I_t ; 0]: rows < t solve, rows >= t must vanish
    assert piv == list(range(t)) and np.array_equal(red[:t], np.eye(t, dtype=np.int64)) and not red[t:].any()
    s = syn[:, bad]
    Ts = gf_plain.apply(T, s)
    solvable = ~Ts[t:].any(axis=0) if t < r else np.ones(bad.size, bool)
    e = Ts[:t]
    # the proof, by the definition
    assert np.array_equal(gf_plain.apply(HE, e[:, solvable]), s[:, solvable])
    for col in np.unique(s[:, ~solvable], axis=1).T:
        assert rank(np.concatenate([HE, col[:, None].astype(np.int64)], axis=1)) == t + 1
    for i, b in enumerate(E):
        hit = solvable & (e[i] != 0)
        out[b, bad[hit]] ^= e[i][hit]
        report[b] = np.count_nonzero(hit)
    report[n + 1] = np.count_nonzero(~solvable)
    return out, report


def restore_stripes(H, stripes, named):
    """[S][n][B] stripes, named [S][n] -> (restored copy, [S][n + 3] reports)."""
    outs, reports = [], []
    for st, flags in zip(stripes, named):
        o, rep = restore(H, st, flags)
        outs.append(o)
        reports.append(rep)
    return np.stack(outs), np.stack(reports)


def brute(H, stripe, flags):
    """The definition by exhaustion, for t <= 2 over tiny inputs: every e in 256^t is tried at every bad position."""
    H = np.asarray(H, dtype=np.int64)
    r, n = H.shape
    state, E = state_of(H, flags)
    t = len(E)
    assert state == USABLE and t <= 2
    out = np.asarray(stripe, dtype=np.uint8).copy()
    syn = gf_plain.apply(H, out)
    report = np.zeros(n + 3, np.int64)
    grid = np.stack(np.meshgrid(*[np.arange(256)] * t, indexing="ij")).reshape(t, -1)      # every e
    images = gf_plain.apply(H[:, E], grid.astype(np.uint8))                                # [r][256^t]
    for x in np.flatnonzero(syn.any(axis=0)):
        report[n] += 1
        match = np.flatnonzero((images == syn[:, x:x + 1]).all(axis=0))
        assert match.size <= 1                                                             # unique: full column rank
        if not match.size:
            report[n + 1] += 1
            continue
        for i, b in enumerate(E):
            if grid[i, match[0]]:
                out[b, x] ^= np.uint8(grid[i, match[0]])
                report[b] += 1
    return out, report
