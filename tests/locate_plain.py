"""Corruption localisation from its definition (test helper, numpy only, on top of tests/gf_plain.py).

For a check matrix H (r x n over GF(2^8) / 0x11d) and one stripe of n blocks of B bytes, with s[x] = H * v[x]:
    x is bad               if s[x] != 0;
    block b explains bad x if s[x] = e * H[:, b] for some e != 0;
    votes[b]     = number of bad positions block b explains, b < n,
    votes[n]     = number of bad positions,
    votes[n + 1] = number of bad positions no single block explains.
One syndrome product, then every candidate block is tested by trying every error value e = 1..255 -- the definition,
not the pivot-row ratio test the kernels use.  `verdict` restates the rule of ecg_locate_verdict.
"""
import numpy as np

import gf_plain

CLEAN, AMBIGUOUS, MULTIPLE = -100, -101, -102


def votes(H, stripe):
    """H: r x n (nested or array); stripe: [n][B] uint8.  Returns the n + 2 counters as an int64 array."""
    H = np.asarray(H, dtype=np.int64)
    r, n = H.shape
    syn = gf_plain.apply(H, stripe)                      # [r][B]
    bad = np.flatnonzero(syn.any(axis=0))
    out = np.zeros(n + 2, np.int64)
    out[n] = bad.size
    if not bad.size:
        return out
    s = syn[:, bad]                                      # [r][nbad]
    explained = np.zeros(bad.size, bool)
    e = np.arange(1, 256)
    for b in range(n):
        if not H[:, b].any():
            continue                                     # a zero column explains nothing
        multiples = gf_plain.TABLE[H[:, b]][:, e]        # [r][255]: e * H[:, b]
        hit = (s[:, :, None] == multiples[:, None, :]).all(axis=0).any(axis=1)
        out[b] = np.count_nonzero(hit)
        explained |= hit
    out[n + 1] = np.count_nonzero(~explained)
    return out


def verdict(v):
    """(status or block id, ids with a vote) of one stripe's n + 2 counters."""
    v = [int(x) for x in v]
    n = len(v) - 2
    ids = [b for b in range(n) if v[b] > 0]
    if v[n] == 0:
        return CLEAN, ids
    full = [b for b in ids if v[b] == v[n]]
    if len(full) > 1:
        return AMBIGUOUS, ids
    if len(full) == 1 and v[n + 1] == 0:
        return full[0], ids
    return MULTIPLE, ids


def proportional_pairs(H):
    """Pairs of columns (a < b) of H that are nonzero multiples of each other, and the number of zero columns."""
    H = np.asarray(H, dtype=np.int64)
    n = H.shape[1]
    e = np.arange(1, 256)
    pairs = 0
    for a in range(n):
        if not H[:, a].any():
            continue
        multiples = gf_plain.TABLE[H[:, a]][:, e]        # [r][255]
        for b in range(a + 1, n):
            pairs += bool((multiples == H[:, b][:, None]).all(axis=0).any())
    zero = sum(1 for b in range(n) if not H[:, b].any())
    return pairs, zero
