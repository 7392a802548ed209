"""GF(2^8) / 0x11d from its definition, and the region product over it (test helper, numpy only).

Written without looking at the oracle or the library: a field element is a polynomial over GF(2) of degree
below 8, multiplication is the carry-less polynomial product reduced by x^8 + x^4 + x^3 + x^2 + 1 (0x11d).
The kernel tests compare the HIP kernels with `apply`; tests/test_gf_plain.py pins this module against the
published antilog table and against the oracle's independently written multiply.
"""
import numpy as np

POLY = 0x11D


def mul(a, b):
    """a * b in GF(2^8)/0x11d by shift-and-xor: add a * x^i for every set bit i of b, reducing as a grows."""
    a &= 0xFF
    b &= 0xFF
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        if a & 0x100:
            a ^= POLY
        b >>= 1
    return r


def _table():
    t = np.zeros((256, 256), np.uint8)
    for a in range(256):
        for b in range(256):
            t[a, b] = mul(a, b)
    return t


TABLE = _table()  # TABLE[c][x] = c * x
TABLE.setflags(write=False)


def apply(coef, inputs):
    """outputs[p] = XOR_j coef[p][j] * inputs[j], bytewise.  coef: m x k (nested or array), inputs: k arrays
    of B uint8 (or a [k][B] array).  Returns a fresh [m][B] uint8 array."""
    c = np.asarray(coef, dtype=np.int64)
    x = np.asarray(inputs, dtype=np.uint8)
    assert c.ndim == 2 and x.ndim == 2 and c.shape[1] == x.shape[0], (c.shape, x.shape)
    assert c.min() >= 0 and c.max() <= 255
    out = np.zeros((c.shape[0], x.shape[1]), np.uint8)
    for p in range(c.shape[0]):
        for j in range(c.shape[1]):
            out[p] ^= TABLE[c[p, j]][x[j]]
    return out
