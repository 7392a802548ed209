"""Two-block correction from its definition (test helper, numpy only, on top of tests/gf_plain.py).

For a check matrix H (r x n over GF(2^8) / 0x11d), one stripe of n blocks of B bytes with s[x] = H * v[x], and a
family F of admissible sets -- every set of one or two blocks for target None (ANY2); every single block and every
pair that holds t for a target 0 <= t < n (TARGET2); nothing for any other target:
    for every bad x (s[x] != 0) with an explanation A in F, s[x] = XOR_{a in A} e_a * H[:, a], every e_a != 0:
        v_a[x] ^= e_a for every a in A;
    report[b]     = positions corrected in block b (a pair counts in both), b < n,
    report[n]     = bad positions,
    report[n + 1] = bad positions left untouched,
    report[n + 2] = positions corrected as a pair.
Explanations are found by enumeration: every block a and every value e_a = 1..255 is tried, and what is left of the
syndrome, s ^ e_a * h_a, is looked up among ALL the multiples e_b * h_b of all the columns (a table built once per H)
-- no pivot rows, no minors, no inverses, no ratio test.  `explanations` does the same without the table, by trying
every (e_a, e_b), for hand cases.  Nothing is recomputed between candidates: every correction comes from the syndromes
of the stripe as it was handed in.  `independent` states k-wise independence of the columns by plain rank.
"""
import itertools

import numpy as np

import gf_plain

_E = np.arange(1, 256)
_CACHE = {}


_MUL = gf_plain.TABLE.tolist()                          # plain lists: the ranks below are many and small
_INV = [0] + [row.index(1) for row in _MUL[1:]]


def _inverse(a):
    return _INV[a]


def rank(M):
    """Rank of a matrix over GF(2^8) by Gaussian elimination on a copy."""
    M = [[int(v) for v in row] for row in (M.tolist() if isinstance(M, np.ndarray) else M)]
    rows, cols = len(M), len(M[0]) if M else 0
    rk = 0
    for c in range(cols):
        piv = next((i for i in range(rk, rows) if M[i][c]), None)
        if piv is None:
            continue
        M[rk], M[piv] = M[piv], M[rk]
        scale = _MUL[_INV[M[rk][c]]]
        top = M[rk] = [scale[v] for v in M[rk]]
        for i in range(rk + 1, rows):                   # the rows above keep their pivots: the rank needs no more
            f = M[i][c]
            if f:
                times = _MUL[f]
                M[i] = [v ^ times[w] for v, w in zip(M[i], top)]
        rk += 1
    return rk


def dependent_set(H, k):
    """The first set (in lexicographic order) of min(k, n) columns of H whose rank is below its size, or None when
    every k columns of H are linearly independent."""
    H = np.asarray(H, dtype=np.int64)
    r, n = H.shape
    key = (H.tobytes(), H.shape, k)
    if key not in _CACHE:
        size = min(k, n)
        found = None
        if r < size:
            found = tuple(range(size))                  # more columns than rows
        else:
            columns = H.T.tolist()
            for cols in itertools.combinations(range(n), size):
                if rank([columns[c] for c in cols]) < size:
                    found = cols
                    break
        _CACHE[key] = found
    return _CACHE[key]


def independent(H, k):
    return dependent_set(H, k) is None


def accepts(H, any2):
    """The library's rule: ANY2 needs every 4 columns independent, TARGET2 every 3; 3 <= r <= 8, 2 <= n <= 32."""
    H = np.asarray(H, dtype=np.int64)
    r, n = H.shape
    return 3 <= r <= 8 and 2 <= n <= 32 and independent(H, 4 if any2 else 3)


def family(n, target):
    """(single blocks, pairs) of F."""
    pairs = list(itertools.combinations(range(n), 2))
    if target is None:
        return list(range(n)), pairs
    t = int(target)
    if not 0 <= t < n:
        return [], []
    return list(range(n)), [p for p in pairs if t in p]


def explanations(H, s, target=None):
    """Every explanation in F of one syndrome vector s, as a list of {block: value} dicts, by trying every value (and
    every pair of values): for hand cases, and for showing that a dependent H gives more than one."""
    H = np.asarray(H, dtype=np.int64)
    n = H.shape[1]
    s = np.asarray(s, dtype=np.uint8)
    if not s.any():
        return []
    singles, pairs = family(n, target)
    out = []
    for b in singles:
        mult = gf_plain.TABLE[H[:, b]][:, _E]                                   # [r][255]
        for i in np.flatnonzero((mult == s[:, None]).all(axis=0)):
            out.append({b: int(_E[i])})
    for a, b in pairs:
        ma = gf_plain.TABLE[H[:, a]][:, _E]                                     # [r][255]
        mb = gf_plain.TABLE[H[:, b]][:, _E]
        both = ma[:, :, None] ^ mb[:, None, :]                                  # [r][255][255]
        for i, j in np.argwhere((both == s[:, None, None]).all(axis=0)):
            out.append({a: int(_E[i]), b: int(_E[j])})
    return out


def _pack(v):
    """[r][...] uint8 -> uint64 keys: byte p of a key is row p (r <= 8).  XOR of keys = key of the XOR."""
    v = np.asarray(v, dtype=np.uint64)
    key = np.zeros(v.shape[1:], np.uint64)
    for p in range(v.shape[0]):
        key |= v[p] << np.uint64(8 * p)
    return key


def _tables(H):
    """Per H: keys[b][e - 1] = the key of e * h_b, and the same sorted, with the (b, e) each stands for."""
    key = ("tables", H.tobytes(), H.shape)
    if key not in _CACHE:
        n = H.shape[1]
        keys = np.stack([_pack(gf_plain.TABLE[H[:, b]][:, _E]) for b in range(n)])          # [n][255]
        flat = keys.reshape(-1)
        order = np.argsort(flat, kind="stable")
        _CACHE[key] = (keys, flat[order], (order // 255).astype(np.int64), (order % 255 + 1).astype(np.int64))
    return _CACHE[key]


def _lookup(sorted_keys, want):
    """(found, index into the sorted arrays) of every key of `want`."""
    idx = np.minimum(np.searchsorted(sorted_keys, want), sorted_keys.size - 1)
    return sorted_keys[idx] == want, idx


def heal2(H, stripe, target=None):
    """H: r x n (nested or array), with every 4 (target None) or every 3 columns independent, so that an explanation is
    unique; stripe: [n][B] uint8; target: None (ANY2), or a block id (any other integer admits nothing).
    Returns (healed [n][B] copy, report: n + 3 counters as an int64 array)."""
    H = np.asarray(H, dtype=np.int64)
    r, n = H.shape
    assert 3 <= r <= 8 and independent(H, 4 if target is None else 3), "the explanation would not be unique"
    stripe = np.asarray(stripe, dtype=np.uint8)
    assert stripe.shape[0] == n
    out = stripe.copy()
    syn = gf_plain.apply(H, stripe)                      # [r][B]
    bad = np.flatnonzero(syn.any(axis=0))
    report = np.zeros(n + 3, np.int64)
    report[n] = bad.size
    singles, pairs = family(n, target)
    if not bad.size or not singles:
        report[n + 1] = bad.size
        return out, report
    keys, sorted_keys, who, value = _tables(H)
    S = _pack(syn[:, bad])                               # [nbad]
    touched = np.zeros(bad.size, bool)
    # one block: s = e * h_b
    found, idx = _lookup(sorted_keys, S)
    for b in singles:
        hit = found & (who[idx] == b)
        out[b, bad[hit]] ^= value[idx[hit]].astype(np.uint8)
        report[b] += np.count_nonzero(hit)
    touched |= found
    # two blocks: s ^ e_a * h_a = e_b * h_b, for every a (TARGET2: a = t) and every e_a; b > a names a pair once
    firsts = singles if target is None else [int(target)]
    for a in firsts:
        rest = S[:, None] ^ keys[a][None, :]             # [nbad][255]
        found, idx = _lookup(sorted_keys, rest)
        b_of = who[idx]
        found &= (b_of > a) if target is None else (b_of != a)
        assert not (found.sum(axis=1) > 1).any() and not (found.any(axis=1) & touched).any(), "two explanations"
        rows, cols = np.nonzero(found)
        out[a, bad[rows]] ^= _E[cols].astype(np.uint8)
        out[b_of[rows, cols], bad[rows]] ^= value[idx[rows, cols]].astype(np.uint8)
        report[a] += rows.size
        np.add.at(report, b_of[rows, cols], 1)
        report[n + 2] += rows.size
        touched[rows] = True
    report[n + 1] = np.count_nonzero(~touched)
    return out, report


def heal2_stripes(H, stripes, targets=None):
    """[S][n][B] stripes, targets None or one per stripe -> (healed copy, [S][n + 3] reports)."""
    outs, reports = [], []
    for i, st in enumerate(stripes):
        o, rep = heal2(H, st, None if targets is None else targets[i])
        outs.append(o)
        reports.append(rep)
    return np.stack(outs), np.stack(reports)


def cauchy(r, n, seed=0):
    """A Cauchy matrix 1 / (x_i ^ y_j), r x n, over distinct x_0.., y_0..: every square submatrix is invertible, so
    every min(r, n) columns are independent (MDS).  The elements are drawn by `seed`."""
    assert r + n <= 256
    elems = np.random.default_rng(seed).permutation(256)[:r + n]
    x, y = elems[:r], elems[r:]
    return np.array([[_inverse(int(xi) ^ int(yj)) for yj in y] for xi in x], dtype=np.int64)
