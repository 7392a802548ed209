"""The update sums from their definition (include/ecg_usum.h), numpy and Python integers over tests/crc32c_plain.py
and tests/gf_plain.py (test helper: imports nothing of the project).

`raw` is the CRC register run from 0 with no final XOR; `shift` multiplies by x^(8 t) mod P by square and multiply,
on Python integers, with crc32c_plain's own one-bit step; `usum` applies records to a sum table exactly as the
definition reads, one record, one block and one piece at a time.
"""
import numpy as np

import crc32c_plain
import gf_plain
import update_plain

DATA, PARITY, BOTH = 1, 2, 3
ONE = 0x80000000                      # x^0: bit 31 is x^0 in the reflected order
_BYTE_STEP = crc32c_plain.TABLE.tolist()   # crc32c_plain's eight one-bit steps of a byte, as Python integers


def raw(data):
    """The remainder of `data` (uint8 array) for initial value 0 and no final XOR."""
    reg = 0
    for byte in np.asarray(data, dtype=np.uint8).tobytes():
        reg = _BYTE_STEP[(reg ^ byte) & 0xFF] ^ (reg >> 8)
    return reg


def mul(a, b):
    """a * b mod P: add b * x^i for every set coefficient x^i of a."""
    p = 0
    for i in range(32):
        if (a >> (31 - i)) & 1:
            p ^= b
        b = crc32c_plain._step(b)
    return p


def shift(a, t):
    """a * x^(8 t) mod P by square and multiply over the bits of t."""
    power = ONE >> 8                  # x^8
    while t:
        if t & 1:
            a = mul(a, power)
        power = mul(power, power)
        t >>= 1
    return a


def pieces(B, piece_bytes):
    return 1 if piece_bytes == 0 else (B + piece_bytes - 1) // piece_bytes


def piece_table(stripes, piece_bytes):
    """crc32c of every block ([S][n][1]) or piece ([S][n][Q]) of [S][n][B] stripes, by crc32c_plain.many."""
    S, n, B = stripes.shape
    if piece_bytes == 0:
        return crc32c_plain.many(stripes)[..., None]
    Q = pieces(B, piece_bytes)
    out = np.zeros((S, n, Q), np.uint32)
    for q in range(Q):
        out[:, :, q] = crc32c_plain.many(stripes[:, :, q * piece_bytes:min((q + 1) * piece_bytes, B)])
    return out


def usum(G, src_ids, dst_ids, sum_ids, sums, records, delta, B, max_len, piece_bytes=0, which=BOTH,
         update_report=None):
    """Apply the records to sums ([S][n_sums][Q] uint32, changed in place; column c is block sum_ids[c]).  delta: the
    uint8 staging buffer that holds delta.  Returns the (R, 2) report {state, nonzero}."""
    G = np.asarray(G, dtype=np.int64).reshape(len(dst_ids), len(src_ids))
    S = sums.shape[0]
    col_of = {int(b): c for c, b in enumerate(sum_ids)}
    report = np.zeros((len(records), 2), np.int64)
    for i, rec in enumerate(records):
        st = int(update_report[i][0]) if update_report is not None else 0
        if st == 0:
            st = update_plain.state_of(rec, len(src_ids), B, S, max_len, delta.size)
        report[i, 0] = st
        if st != 0:
            continue
        s, col, off, ln, in_off = (int(v) for v in rec)
        d = delta[in_off:in_off + ln]
        report[i, 1] = np.count_nonzero(d)
        blocks = [(src_ids[col], 1)] if which & DATA else []
        if which & PARITY:
            blocks += [(dst_ids[row], int(G[row, col])) for row in range(len(dst_ids)) if G[row, col]]
        for b, c in blocks:
            if int(b) not in col_of:
                continue
            a = off
            while a < off + ln:
                q = a // piece_bytes if piece_bytes else 0
                e = min((q + 1) * piece_bytes, B) if piece_bytes else B
                b1 = min(off + ln, e)
                v = shift(raw(gf_plain.TABLE[c][d[a - off:b1 - off]]), e - b1)
                sums[s, col_of[int(b)], q] ^= np.uint32(v)
                a = b1
    return report


def traffic_bytes(nnz_per_col, records, B, piece_bytes, which):
    """len of delta read, and 8 bytes per sum word met (all records taken as applied, every block as recorded)."""
    total = 0
    for _, col, off, ln, _ in (tuple(int(v) for v in r) for r in records):
        if ln > 0 and col >= 0 and off >= 0:
            met = (off + ln - 1) // piece_bytes - off // piece_bytes + 1 if piece_bytes else 1
            total += ln + 8 * met * ((1 if which & DATA else 0) + (int(nnz_per_col[col]) if which & PARITY else 0))
    return total
