"""The delta update from its definition (include/ecg_update.h), numpy over tests/gf_plain.py's table (test helper:
imports nothing of the project).

`update` applies records {stripe, col, off, len, in_off} to [S][slots][B] stripes one byte range at a time, exactly as
the definition reads; `check_records` and `traffic_bytes` restate the two host helpers of the library.
"""
import numpy as np

import gf_plain

WRITE, DELTA = 0, 1
APPLIED, BAD_STRIPE, BAD_COL, BAD_RANGE, TOO_LONG, BAD_STAGING = range(6)


def state_of(rec, k_in, B, S, max_len, in_bytes):
    """The state of one record: the first rule it breaks."""
    stripe, col, off, ln, in_off = (int(v) for v in rec)
    if not 0 <= stripe < S:
        return BAD_STRIPE
    if not 0 <= col < k_in:
        return BAD_COL
    if off < 0 or ln < 0 or off + ln > B:
        return BAD_RANGE
    if ln > max_len:
        return TOO_LONG
    if in_off < 0 or in_off + ln > in_bytes:
        return BAD_STAGING
    return APPLIED


def update(G, src_ids, dst_ids, stripes, records, data_in, mode, max_len, delta_out=None):
    """Apply the records in order to stripes ([S][slots][B] uint8, changed in place; column j of G is slot src_ids[j],
    row i slot dst_ids[i]) and to delta_out (uint8, as large as data_in, or None).  Returns the (R, 2) report
    {state, changed}."""
    G = np.asarray(G, dtype=np.int64).reshape(len(dst_ids), len(src_ids))
    S, _, B = stripes.shape
    report = np.zeros((len(records), 2), np.int64)
    for i, rec in enumerate(records):
        st = state_of(rec, len(src_ids), B, S, max_len, data_in.size)
        report[i, 0] = st
        if st != APPLIED:
            continue
        s, col, off, ln, in_off = (int(v) for v in rec)
        new = data_in[in_off:in_off + ln]
        if mode == WRITE:
            delta = stripes[s, src_ids[col], off:off + ln] ^ new
            stripes[s, src_ids[col], off:off + ln] = new
            if delta_out is not None:
                delta_out[in_off:in_off + ln] = delta
        else:
            delta = new.copy()
        report[i, 1] = np.count_nonzero(delta)
        for row in range(len(dst_ids)):
            if G[row, col]:
                stripes[s, dst_ids[row], off:off + ln] ^= gf_plain.TABLE[G[row, col]][delta]
    return report


def legal_records(rng, S, k, B, count, max_len):
    """`count` records per stripe with pairwise disjoint ranges (some touching, some empty) of at most max_len bytes,
    random columns, in scrambled order, their staging ranges packed in another scrambled order with gaps of 0..2
    bytes.  Returns (records [R][5] int64, in_bytes)."""
    recs = []
    for s in range(S):
        cuts = np.sort(rng.choice(B + 1, 2 * count, replace=True))
        for lo, hi in zip(cuts[0::2], cuts[1::2]):
            hi = min(int(hi), int(lo) + max_len)
            recs.append([s, int(rng.integers(0, k)), int(lo), hi - int(lo), 0])
    at = 3
    for i in rng.permutation(len(recs)):
        recs[i][4] = at
        at += recs[i][3] + int(rng.integers(0, 3))
    return np.array([recs[i] for i in rng.permutation(len(recs))], dtype=np.int64), at + 5


def _overlaps(a, b):
    """Two half-open ranges share a byte (an empty range shares none)."""
    return a[0] < a[1] and b[0] < b[1] and a[0] < b[1] and b[0] < a[1]


def check_records(records, k_in, B, S, max_len, in_bytes, with_delta_out=False):
    """-1 if every record is state 0 and the ranges of a stripe (and, with_delta_out, the staging ranges) are pairwise
    disjoint; else the index of the first record that is refused or overlaps a record before it."""
    seen = []
    for i, rec in enumerate(records):
        if state_of(rec, k_in, B, S, max_len, in_bytes) != APPLIED:
            return i
        s, _, off, ln, in_off = (int(v) for v in rec)
        for ps, po, pl, pi in seen:
            if ps == s and _overlaps((off, off + ln), (po, po + pl)):
                return i
            if with_delta_out and _overlaps((in_off, in_off + ln), (pi, pi + pl)):
                return i
        seen.append((s, off, ln, in_off))
    return -1


def traffic_bytes(nnz_per_col, records, mode, with_delta_out=False):
    """The bytes the records move by the definition: per record len * ((3 if WRITE else 1) + with_delta_out +
    2 * nnz[col]); WRITE reads old data and input and writes data, every nonzero row reads and writes its parity."""
    total = 0
    for _, col, _, ln, _ in (tuple(int(v) for v in r) for r in records):
        if ln > 0:
            total += ln * ((3 if mode == WRITE else 1) + (1 if with_delta_out else 0) + 2 * int(nnz_per_col[col]))
    return total
