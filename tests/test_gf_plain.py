"""Pin tests/gf_plain.py, the oracle-independent field definition the kernel sweep compares against (CPU only)."""
import numpy as np

import gf_plain
from test_oracle import EXP_0x11D


def test_module_owes_nothing_to_oracle_or_library():
    import ast
    tree = ast.parse(open(gf_plain.__file__).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
    assert names == {"numpy"}, names


def test_table_matches_published_antilog_sequence():
    x = 1
    for i, e in enumerate(EXP_0x11D):
        assert x == e, i
        x = int(gf_plain.TABLE[x, 2])
    x, order = 2, 1
    while x != 1:
        x = int(gf_plain.TABLE[x, 2])
        order += 1
    assert order == 255  # generator 2 has order 255
    assert int(gf_plain.TABLE[2, 142]) == 1  # 2^-1 = 0x8e under 0x11d
    t = gf_plain.TABLE
    assert np.array_equal(t, t.T)
    assert not t[0].any() and np.array_equal(t[1], np.arange(256, dtype=np.uint8))
    for a in range(1, 256):  # a field: every nonzero row is a permutation of the byte values
        assert np.array_equal(np.sort(t[a]), np.arange(256, dtype=np.uint8)), a


def test_table_equals_oracle_multiply_everywhere(oracle):
    for a in range(256):
        for b in range(256):
            assert int(gf_plain.TABLE[a, b]) == oracle.galois_single_multiply(a, b), (a, b)


def test_apply_equals_oracle_matrix_encode(oracle):
    rng = np.random.default_rng(0x11D)
    for k, m, B in [(1, 1, 1), (3, 2, 17), (10, 4, 1000), (16, 16, 257), (7, 9, 4693)]:
        M = rng.integers(0, 256, (m, k))
        M[0, 0], M[-1, -1] = 0, 1
        data = [rng.integers(0, 256, B, dtype=np.uint8) for _ in range(k)]
        coding = [np.full(B, 0x3C, np.uint8) for _ in range(m)]
        oracle.jerasure_matrix_encode(k, m, [int(c) for c in M.ravel()], data, coding, B)
        got = gf_plain.apply(M, data)
        for i in range(m):
            if M[i].any():  # Jerasure leaves the block of an all-zero row untouched; the product is zero
                assert np.array_equal(got[i], coding[i]), (k, m, B, i)
            else:
                assert not got[i].any()
