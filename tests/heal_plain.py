"""In-place correction from its definition (test helper, numpy only, on top of tests/gf_plain.py and
tests/locate_plain.py).

For a check matrix H (r x n over GF(2^8) / 0x11d), one stripe of n blocks of B bytes with s[x] = H * v[x], and a
candidate set K -- {target} if 0 <= target < n, empty for any other target, every block for target None (ANY mode):
    for every bad x (s[x] != 0) and every b in K with s[x] = e * H[:, b] for some e != 0:  v_b[x] ^= e;
    report[b]     = positions corrected in block b, b < n,
    report[n]     = bad positions,
    report[n + 1] = bad positions left untouched.
One syndrome product, then every candidate is tested against every error value e = 1..255 -- the definition, not the
pivot-row ratio test and the division by the pivot that the kernels use.  Nothing is recomputed between candidates:
every correction comes from the syndromes of the stripe as it was handed in.
"""
import numpy as np

import gf_plain
import locate_plain as LP


def candidates(n, target):
    if target is None:
        return list(range(n))
    return [int(target)] if 0 <= int(target) < n else []


def heal(H, stripe, target=None):
    """H: r x n (nested or array); stripe: [n][B] uint8; target: None (ANY), or a block id (any other integer names
    no block).  Returns (healed [n][B] copy, report: n + 2 counters as an int64 array)."""
    H = np.asarray(H, dtype=np.int64)
    r, n = H.shape
    stripe = np.asarray(stripe, dtype=np.uint8)
    assert stripe.shape[0] == n
    out = stripe.copy()
    syn = gf_plain.apply(H, stripe)                      # [r][B]
    bad = np.flatnonzero(syn.any(axis=0))
    report = np.zeros(n + 2, np.int64)
    report[n] = bad.size
    if not bad.size:
        return out, report
    s = syn[:, bad]                                      # [r][nbad]
    touched = np.zeros(bad.size, bool)
    e = np.arange(1, 256)
    for b in candidates(n, target):
        if not H[:, b].any():
            continue                                     # a zero column explains nothing and is never corrected
        multiples = gf_plain.TABLE[H[:, b]][:, e]        # [r][255]: e * H[:, b]
        match = (s[:, :, None] == multiples[:, None, :]).all(axis=0)    # [nbad][255]
        hit = match.any(axis=1)
        value = e[match.argmax(axis=1)].astype(np.uint8)                # the e that matches (where one does)
        out[b, bad[hit]] ^= value[hit]
        report[b] = np.count_nonzero(hit)
        touched |= hit
    report[n + 1] = np.count_nonzero(~touched)
    return out, report


def heal_stripes(H, stripes, targets=None):
    """[S][n][B] stripes, targets None or one per stripe -> (healed copy, [S][n + 2] reports)."""
    outs, reports = [], []
    for i, st in enumerate(stripes):
        o, rep = heal(H, st, None if targets is None else targets[i])
        outs.append(o)
        reports.append(rep)
    return np.stack(outs), np.stack(reports)


def targets_from_votes(votes):
    """What ecg_heal.targets_from_votes computes, by locate_plain.verdict: the named block, or -1."""
    out = []
    for row in np.asarray(votes):
        status, _ = LP.verdict([int(x) & 0xFFFFFFFF for x in row])
        out.append(status if status >= 0 else -1)
    return np.array(out, dtype=np.int32)
