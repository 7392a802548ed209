"""tests/restore_plain.py, the plain form the GPU restore tests compare with, checked on the CPU: against exhaustion
over every error vector (t <= 2), against tests/heal_plain.py at t = 1, and on the properties include/ecg_restore.h
states.  Test infrastructure only: nothing here loads a library of the project.
"""
import json
import os

import numpy as np
import pytest

import gf_plain
import heal_plain
import restore_plain as RP

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]


def _check(name):
    c = next(c for c in GOLDEN if c["name"] == name)
    k, m = c["k"], c["m"]
    M = np.asarray(c["matrix"], dtype=np.int64).reshape(m, k)
    return np.concatenate([M, np.eye(m, dtype=np.int64)], axis=1)


def _stripe(H, B, seed):
    """A stripe that satisfies H = [M | I]: random data, parity by the plain product."""
    r, n = H.shape
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, (n - r, B), dtype=np.uint8)
    return np.concatenate([data, gf_plain.apply(H[:, :n - r], data)])


def _flags(n, E):
    f = np.zeros(n, np.uint8)
    f[list(E)] = 1
    return f


def _damage(stripe, blocks, lo, hi, seed):
    rng = np.random.default_rng(seed)
    out = stripe.copy()
    for b in blocks:
        out[b, lo:hi] ^= rng.integers(1, 256, hi - lo, dtype=np.uint8)
    return out


def test_reduce_and_rank():
    H = _check("RS(10,4)")
    assert RP.rank(H) == 4 and RP.rank(H[:, [0, 3, 7, 9]]) == 4 and RP.rank(H[:, [10, 11]]) == 2
    assert RP.rank(np.array([[1, 2], [3, 6]])) == 1              # (3, 6) = 3 * (1, 2)
    red, T, piv = RP.reduce(H[:, [12, 13, 1]])                   # unit columns first: the pivots need a swap
    assert piv == [0, 1, 2] and np.array_equal(gf_plain.apply(T, H[:, [12, 13, 1]].astype(np.uint8)), red)
    for a in range(1, 256):
        assert gf_plain.mul(a, RP.inv(a)) == 1


def test_states():
    H = _check("RS(10,4)")
    n = H.shape[1]
    assert RP.state_of(H, _flags(n, []))[0] == RP.NONE_FLAGGED
    assert RP.state_of(H, _flags(n, [1, 2, 3, 4, 5]))[0] == RP.TOO_MANY
    assert RP.state_of(H, _flags(n, [0, 5, 11, 13]))[0] == RP.USABLE
    Hz = H.copy()
    Hz[:, 3] = 0
    assert RP.state_of(Hz, _flags(n, [3]))[0] == RP.DEPENDENT
    Hd = H.copy()
    Hd[:, 4] = gf_plain.TABLE[7][Hd[:, 2]]
    assert RP.state_of(Hd, _flags(n, [2, 4]))[0] == RP.DEPENDENT
    st = _damage(_stripe(H, 40, 1), [1, 2], 3, 9, 2)
    for flags in (_flags(n, []), _flags(n, [1, 2, 3, 4, 5])):
        out, rep = RP.restore(H, st, flags)
        assert np.array_equal(out, st) and rep[n] == rep[n + 1] == 6 and not rep[:n].any()


@pytest.mark.parametrize("E", [(2,), (11,), (0, 9), (3, 12), (10, 13)])
def test_against_exhaustion(E):
    """RS(10,4), t <= 2, 24 bytes: flagged damage, a flagged but clean block, damage in an unflagged block."""
    H = _check("RS(10,4)")
    n = H.shape[1]
    clean = _stripe(H, 24, 3)
    st = _damage(clean, E[:1], 2, 11, 4)                          # only the first flagged block is damaged ...
    st = _damage(st, [5], 8, 14, 5)                               # ... and unflagged block 5, overlapping it
    got, rep = RP.restore(H, st, _flags(n, E))
    want, wrep = RP.brute(H, st, _flags(n, E))
    assert np.array_equal(got, want) and np.array_equal(rep, wrep)
    assert rep[n] == 12 and rep[n + 1] == 6                       # the guard: block 5's positions are left alone
    assert np.array_equal(got[:, 14:], clean[:, 14:]) and np.array_equal(got[:, :8], clean[:, :8])
    assert np.array_equal(got[:, 8:14], st[:, 8:14])
    for b in E[1:]:
        assert rep[b] == 0


@pytest.mark.parametrize("t", [1, 2, 3, 4])
def test_flagged_damage_comes_back(t):
    H = _check("RS(10,4)")
    n = H.shape[1]
    clean = _stripe(H, 100, 6)
    for E in ([0, 4, 8, 9][:t], [10, 11, 12, 13][:t], [13, 2, 11, 7][:t]):
        st = _damage(clean, E, 10, 77, 7)
        got, rep = RP.restore(H, st, _flags(n, E))
        assert np.array_equal(got, clean)
        assert rep[n] == 67 and rep[n + 1] == 0 and rep[n + 2] == 0 and all(rep[b] == 67 for b in E)


def test_no_guard_at_t_equal_r():
    """t = r: every syndrome is explained; damage in an unflagged block is folded into the flagged ones."""
    H = _check("RS(10,4)")
    n = H.shape[1]
    clean = _stripe(H, 32, 8)
    st = _damage(_damage(clean, [0, 1], 0, 8, 9), [6], 4, 12, 10)
    got, rep = RP.restore(H, st, _flags(n, [0, 1, 2, 3]))
    assert rep[n] == 12 and rep[n + 1] == 0
    assert not gf_plain.apply(H, got).any()                      # a codeword again -- another one
    assert not np.array_equal(got, clean) and np.array_equal(got[6], st[6])
    got2, rep2 = RP.restore(H, st, _flags(n, [0, 1]))            # t = 2: the guard holds
    assert rep2[n + 1] == 8 and np.array_equal(got2[:, :4], clean[:, :4]) and np.array_equal(got2[:, 4:], st[:, 4:])


@pytest.mark.parametrize("name", ["RS(10,4)", "RS(6,2)", "RS(8,1)", "Azure(8,2,2)"])
def test_one_flag_is_the_heal_with_that_target(name):
    H = _check(name)
    r, n = H.shape
    clean = _stripe(H, 64, 11)
    st = _damage(_damage(clean, [1], 5, 30, 12), [n - 1], 20, 50, 13)
    for b in (1, n - 1, 0):
        got, rep = RP.restore(H, st, _flags(n, [b]))
        want, wrep = heal_plain.heal(H, st, b)
        assert np.array_equal(got, want) and np.array_equal(rep[:n + 2], wrep) and rep[n + 2] == RP.USABLE
    Hz = H.copy()
    Hz[:, 2] = 0                                                 # a flagged zero column: state 3, the heal's no-op
    got, rep = RP.restore(Hz, st, _flags(n, [2]))
    want, wrep = heal_plain.heal(Hz, st, 2)
    assert np.array_equal(got, want) and np.array_equal(rep[:n + 2], wrep) and rep[n + 2] == RP.DEPENDENT
