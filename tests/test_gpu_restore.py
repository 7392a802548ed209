"""Named-block restoration on the GPU: the kernels of libecg_restore.so against the definition (tests/restore_plain.py,
which eliminates with row swaps over tests/gf_plain.py's table and proves each answer by the definition) and, where the
flagged blocks hold all the damage, against the stripe as the oracle encoded it.

Every case uploads a guard-band arena (tests/gf_arena.py), runs one call and compares THE WHOLE ARENA with the expected
image -- guard bands, blocks the check does not name and stripes the call does not select included --, the full report,
`counters()` and `last_launch()`: a call that fell back to the byte path alone would show in both.

Every test here loads libecg_restore.so and runs its kernels.
"""
import json
import os

import numpy as np
import pytest

import gf_arena as A
import gf_plain
import restore_plain as RP

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
GUARD = A.GUARD
K, M_ = 10, 4
N = K + M_
THREADS = 128                                              # gf_kernels.hpp kThreads: 16-byte columns per workgroup
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return torch


@pytest.fixture(scope="module")
def restore(ecg):
    import ecg_restore
    ecg_restore.lib()
    return ecg_restore


@pytest.fixture(scope="module")
def rs(oracle):
    """RS(10,4) from the oracle: (matrix as a flat list, H = [matrix | I])."""
    M = oracle.reed_sol_vandermonde_coding_matrix(K, M_)
    H = np.concatenate([np.asarray(M, dtype=np.int64).reshape(M_, K), np.eye(M_, dtype=np.int64)], axis=1)
    return M, H


def _encoded(oracle, M, S, B, seed):
    """[S][14][B] stripes, random data, parity by the oracle's encode."""
    rng = np.random.default_rng(seed)
    out = np.zeros((S, N, B), np.uint8)
    for s in range(S):
        data = [rng.integers(0, 256, B, dtype=np.uint8) for _ in range(K)]
        coding = [np.zeros(B, np.uint8) for _ in range(M_)]
        oracle.jerasure_matrix_encode(K, M_, M, data, coding, B)
        out[s] = np.stack(data + coding)
    return out


def _hit(stripes, s, b, lo, hi, rng):
    """XOR nonzero bytes into [lo, hi) of block b of stripe s."""
    lo, hi = max(lo, 0), min(hi, stripes.shape[2])
    if hi > lo:
        stripes[s, b, lo:hi] ^= rng.integers(1, 256, hi - lo, dtype=np.uint8)


def _arena(stripes, lead=1, pitch=None):
    """The arena image of [S][n][B] stripes: `lead` slots the check does not name (0x77) in front of them."""
    S, n, B = stripes.shape
    img = np.full((S, lead + n, A.pitch(B) if pitch is None else pitch), A.BAND, np.uint8)
    img[:, :lead, GUARD:GUARD + B] = 0x77
    img[:, lead:, GUARD:GUARD + B] = stripes
    return img


def _flags(torch, named):
    return torch.from_numpy(np.ascontiguousarray(named, dtype=np.uint8)).cuda()


def _ints(torch, values):
    return None if values is None else torch.tensor([int(v) for v in values], dtype=torch.int32, device="cuda")


def _geometry(B, rows):
    ncols = B >> 4
    return {"cols_per_wg": THREADS, "wg_per_stripe": -(-ncols // THREADS), "S": rows, "rtiles": 1}


def _run(torch, R, img, B, H, src, named, call, sel=None, shift=0):
    """Upload img (base `shift` bytes past a 16-byte boundary), run call(view, flags, ids) and compare the report, the
    whole arena, the counters and the last launch with the definition.  named[i] are the flags of stripe rows[i].
    Returns (report, expected image, image after), numpy."""
    H = np.asarray(H, dtype=np.int64)
    n = H.shape[1]
    rows = list(range(img.shape[0])) if sel is None else list(sel)
    assert len(set(rows)) == len(rows) == len(named)                    # the ids of a call must be distinct
    want, reports = img.copy(), []
    for i, s in enumerate(rows):
        out, rep = RP.restore(H, img[s][src, GUARD:GUARD + B], named[i])
        want[s][src, GUARD:GUARD + B] = out
        reports.append(rep)
    reports = np.stack(reports)
    d = A.to_dev(torch, img, shift)
    c0, l0 = R.counters(), R.last_launch()
    got = call(A.blocks(d, B), _flags(torch, named), _ints(torch, sel))
    torch.cuda.synchronize()
    c1, l1 = R.counters(), R.last_launch()
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(rows), n + 3)
    g = got.cpu().numpy().astype(np.int64)
    assert np.array_equal(g, reports), (B, shift, sel, g.tolist(), reports.tolist())
    after = d.cpu().numpy()
    flagged = {(s, src[j]) for i, s in enumerate(rows) for j in np.flatnonzero(named[i])}
    A.assert_same(after, want, B, lambda s, slot: (s, slot) in flagged, (B, shift, sel))
    vec = (B & ~15) if shift % 16 == 0 and img.shape[2] % 16 == 0 else 0
    assert c1["launches"] - c0["launches"] == (vec > 0) + (vec < B)
    assert c1["bytes"] - c0["bytes"] == len(rows) * B * n
    if vec:
        assert {f: l1[f] for f in ("cols_per_wg", "wg_per_stripe", "S", "rtiles")} == _geometry(B, len(rows)), l1
    else:
        assert l1 == l0                                                  # a byte-path call leaves the record alone
    return g, want, after


# ---- sizes and set sizes

SETS = {  # per t: stripe 0 data blocks only, stripe 1 coding blocks only (unit columns: the first rows of H_E are
          # zero and the pivots must be searched), stripe 2 mixed
    1: ([3], [12], [13]),
    2: ([0, 9], [11, 13], [4, 10]),
    3: ([1, 5, 8], [10, 12, 13], [2, 11, 12]),
    4: ([0, 3, 6, 9], [10, 11, 12, 13], [7, 10, 5, 13]),
}


@gpu
@pytest.mark.parametrize("B", [1, 15, 16, 17, 1077, 8213])
def test_sizes_and_set_sizes(oracle, torch_cuda, restore, rs, B):
    """RS(10,4), t = 1..4, one launch per t with a different set per stripe.  Each flagged block is damaged in a run of
    its own (the first of a set as a whole), so the masks of a position's blocks differ.  What comes back is the
    oracle's stripe; at t = 1 the heal's TARGET mode gives the same bytes and the same first n + 2 counters."""
    torch = torch_cuda
    import ecg_heal
    M, H = rs
    clean = _encoded(oracle, M, 3, B, 100 + B)
    src = list(range(1, N + 1))
    for t, sets in SETS.items():
        rng = np.random.default_rng(1000 * t + B)
        stripes = clean.copy()
        named = np.zeros((3, N), np.uint8)
        for s, E in enumerate(sets):
            named[s, E] = 1
            for i, b in enumerate(E):
                if i == 0:
                    _hit(stripes, s, b, 0, B, rng)
                else:
                    _hit(stripes, s, b, (B * i) // 5 - 3, (B * (i + 2)) // 5 + 2, rng)
        img = _arena(stripes)
        g, want, after = _run(torch, restore, img, B, H, src, named,
                              lambda v, f, ids: restore.matrix_batch(H, src, v, f, stripe_ids=ids))
        assert np.array_equal(want, _arena(clean))                      # the second ground truth: the oracle's stripe
        assert (g[:, N] == B).all() and not g[:, N + 1:].any()
        for s, E in enumerate(sets):
            assert g[s, E[0]] == B and all(0 < g[s, b] <= B for b in E[1:])
        if t == 1:
            d = A.to_dev(torch, img)
            rep = ecg_heal.matrix_batch(H, src, A.blocks(d, B), targets=_ints(torch, [E[0] for E in sets]))
            torch.cuda.synchronize()
            assert np.array_equal(d.cpu().numpy(), after)
            assert np.array_equal(rep.cpu().numpy(), g[:, :N + 2])


@gpu
def test_encode_and_ec_batch_forms(ecg, oracle, torch_cuda, restore, rs):
    """The [matrix | I] form and the class's own check give what the primitive gives (no leading slot: block b is
    slot b)."""
    torch = torch_cuda
    M, H = rs
    B = 1077
    clean = _encoded(oracle, M, 2, B, 7)
    stripes = clean.copy()
    rng = np.random.default_rng(8)
    named = np.zeros((2, N), np.uint8)
    for s, E in enumerate(([2, 11, 13], [10, 0])):
        named[s, E] = 1
        for i, b in enumerate(E):
            _hit(stripes, s, b, 40 * i, 900 + 40 * i, rng)
    img = _arena(stripes, lead=0)
    src = list(range(N))
    code = ecg.ec_factory(ecg.ECTYPE.RS, ecg.CodingParameters(k=K, m=M_))
    assert np.array_equal(np.asarray(code.check_matrix(), dtype=np.int64).reshape(M_, N), H)
    for call in (lambda v, f, ids: restore.encode_batch(K, M_, M, v, f, stripe_ids=ids),
                 lambda v, f, ids: restore.ec_batch(code, v, f, stripe_ids=ids)):
        _, want, _ = _run(torch, restore, img, B, H, src, named, call)
        assert np.array_equal(want, _arena(clean, lead=0))


# ---- mixed states in one launch

def _azure():
    c = next(c for c in GOLDEN if c["name"] == "Azure(8,2,2)")
    k, m = c["k"], c["m"]
    Cm = np.asarray(c["matrix"], dtype=np.int64).reshape(m, k)
    return k, m, np.concatenate([Cm, np.eye(m, dtype=np.int64)], axis=1)


@gpu
def test_mixed_states_in_one_launch(torch_cuda, restore):
    """Azure-LRC(8,2,2): a scrambled selection of five of eight damaged stripes with a set of its own each -- empty
    (state 1), five flags (state 2), the four data blocks of one local group, whose columns are supported on three
    rows (state 3), and two usable sets.  The unselected stripes and the unusable ones stay as they are."""
    torch = torch_cuda
    k, m, H = _azure()
    n, B, S = k + m, 1077, 8
    lrow = next(p for p in range(m) if np.count_nonzero(H[p, :k]) == 4)  # a local row: four data blocks
    local = [j for j in range(k) if H[lrow, j]]
    assert len(local) == 4 and np.count_nonzero(H[:, local].any(axis=1)) == 3
    rng = np.random.default_rng(31)
    data = rng.integers(0, 256, (S, k, B), dtype=np.uint8)
    clean = np.stack([np.concatenate([d, gf_plain.apply(H[:, :k], d)]) for d in data])
    sel = [6, 1, 4, 3, 0]
    sets = {6: [], 1: [0, 2, 5, 8, 11], 4: local, 3: [1, 6, 9], 0: [7, 10]}
    damaged = {6: [3], 1: [0, 2, 5, 8, 11], 4: local, 3: [1, 6, 9], 0: [7, 10], 2: [4], 5: [0, 9], 7: [11]}
    stripes = clean.copy()
    for s, blocks in damaged.items():
        for i, b in enumerate(blocks):
            _hit(stripes, s, b, 100 * i + s, 500 + 100 * i, rng)
    named = np.zeros((len(sel), n), np.uint8)
    for i, s in enumerate(sel):
        named[i, sets[s]] = 1
    assert [RP.state_of(H, f)[0] for f in named] == [RP.NONE_FLAGGED, RP.TOO_MANY, RP.DEPENDENT, RP.USABLE, RP.USABLE]
    img = _arena(stripes)
    src = list(range(1, n + 1))
    g, want, _ = _run(torch, restore, img, B, H, src, named,
                      lambda v, f, ids: restore.matrix_batch(H, src, v, f, stripe_ids=ids), sel=sel)
    assert g[:, n + 2].tolist() == [1, 2, 3, 0, 0]
    blocks = A.blocks(want, B)[:, 1:]
    for s in range(S):
        assert np.array_equal(blocks[s], clean[s] if s in (3, 0) else stripes[s]), s
    for i in range(3):
        assert g[i, n] == g[i, n + 1] > 0 and not g[i, :n].any()


# ---- the guard, and where it ends

@gpu
def test_guard_below_r_and_none_at_r(oracle, torch_cuda, restore, rs):
    torch = torch_cuda
    M, H = rs
    B = 1077
    clean = _encoded(oracle, M, 1, B, 41)
    rng = np.random.default_rng(42)
    stripes = clean.copy()
    _hit(stripes, 0, 2, 100, 700, rng)
    _hit(stripes, 0, 11, 300, 1000, rng)
    _hit(stripes, 0, 7, 650, 720, rng)                                  # block 7 is flagged by nobody
    img = _arena(stripes)
    src = list(range(1, N + 1))
    call = lambda v, f, ids: restore.matrix_batch(H, src, v, f, stripe_ids=ids)
    named = np.zeros((1, N), np.uint8)
    named[0, [2, 11]] = 1
    g, want, _ = _run(torch, restore, img, B, H, src, named, call)
    got = A.blocks(want, B)[0, 1:]
    assert g[0, N] == 900 and g[0, N + 1] == 70 and g[0, N + 2] == 0 and g[0, 7] == 0
    assert np.array_equal(got[:, 650:720], stripes[0][:, 650:720])      # left byte for byte, the flagged blocks too
    assert np.array_equal(got[:, :650], clean[0][:, :650]) and np.array_equal(got[:, 720:], clean[0][:, 720:])
    assert g[0, 2] == 550 and g[0, 11] == 630                           # 600 and 700 less the 50 / 70 left alone
    named[0, [0, 13]] = 1                                               # t = 4 = r: the guard is gone
    g, want, _ = _run(torch, restore, img, B, H, src, named, call)
    got = A.blocks(want, B)[0, 1:]
    assert g[0, N] == 900 and g[0, N + 1] == 0 and g[0, N + 2] == 0
    assert not gf_plain.apply(H, got).any() and np.array_equal(got[7], stripes[0][7])
    assert not np.array_equal(got[:, 650:720], clean[0][:, 650:720])    # a codeword, not the stored one


# ---- wide checks

def _cauchy(r, n):
    """H[i][j] = 1 / (i ^ (r + j)): every square submatrix is nonsingular, so every r columns are independent."""
    return np.array([[RP.inv(i ^ (r + j)) for j in range(n)] for i in range(r)], dtype=np.int64)


@gpu
def test_wide_check_r8_n128(torch_cuda, restore):
    """A Cauchy check with r = 8, n = 128 (no identity part): flagged ids 0, 63, 64 and 127 (report[b] lives in three
    counter registers, the state in the third) at t = 8 and t = 4."""
    torch = torch_cuda
    r, n, B = 8, 128, 1077
    H = _cauchy(r, n)
    assert RP.rank(H[:, [0, 1, 63, 64, 65, 100, 126, 127]]) == 8
    rng = np.random.default_rng(51)
    _, T, _ = RP.reduce(H[:, n - r:])                                   # T * H[:, last r] = I
    clean = np.zeros((2, n, B), np.uint8)
    for s in range(2):
        clean[s, :n - r] = rng.integers(0, 256, (n - r, B), dtype=np.uint8)
        clean[s, n - r:] = gf_plain.apply(T, gf_plain.apply(H[:, :n - r], clean[s, :n - r]))
    assert not gf_plain.apply(H, clean[0]).any()
    sets = ([0, 1, 63, 64, 65, 100, 126, 127], [0, 63, 64, 127])
    stripes = clean.copy()
    named = np.zeros((2, n), np.uint8)
    for s, E in enumerate(sets):
        named[s, E] = 1
        for i, b in enumerate(E):
            _hit(stripes, s, b, 90 * i, 400 + 90 * i, rng)
    img = _arena(stripes, lead=0)
    src = list(range(n))
    g, want, _ = _run(torch, restore, img, B, H, src, named,
                      lambda v, f, ids: restore.matrix_batch(H, src, v, f, stripe_ids=ids))
    assert np.array_equal(want, _arena(clean, lead=0))
    assert (g[:, [0, 63, 64, 127]] == 400).all() and not g[:, n + 1:].any()


# ---- the byte path alone

@gpu
def test_byte_path_alone(oracle, torch_cuda, restore, rs):
    """Base + 1 and an odd block stride: no block is 16-byte aligned, the byte kernel covers everything."""
    torch = torch_cuda
    M, H = rs
    B = 1077
    clean = _encoded(oracle, M, 2, B, 61)
    rng = np.random.default_rng(62)
    stripes = clean.copy()
    named = np.zeros((2, N), np.uint8)
    for s, E in enumerate(([4, 12, 13], [10, 1])):
        named[s, E] = 1
        for i, b in enumerate(E):
            _hit(stripes, s, b, 300 * i, 300 * i + 500, rng)
    odd = GUARD + B + GUARD + (1 - (B & 1))
    assert odd % 2 == 1
    src = list(range(1, N + 1))
    for img, shift in ((_arena(stripes, pitch=odd), 1), (_arena(stripes, pitch=odd), 0), (_arena(stripes), 1)):
        _, want, _ = _run(torch, restore, img, B, H, src, named,
                          lambda v, f, ids: restore.matrix_batch(H, src, v, f, stripe_ids=ids), shift=shift)
        assert np.array_equal(A.blocks(want, B)[:, 1:], clean)


# ---- flagged but undamaged

@gpu
def test_flagged_but_undamaged_block_stays_unwritten(oracle, torch_cuda, restore, rs):
    """The undamaged block is the FIRST of its set in stripe 0 and the last in stripe 1; stripe 2 is flagged and clean
    altogether."""
    torch = torch_cuda
    M, H = rs
    B = 1077
    clean = _encoded(oracle, M, 3, B, 71)
    rng = np.random.default_rng(72)
    stripes = clean.copy()
    named = np.zeros((3, N), np.uint8)
    named[0, [1, 6, 12]] = 1
    named[1, [3, 10, 13]] = 1
    named[2, [0, 11]] = 1
    for s, b in ((0, 6), (0, 12), (1, 3), (1, 10)):
        _hit(stripes, s, b, 17 * b, 17 * b + 600, rng)
    img = _arena(stripes)
    src = list(range(1, N + 1))
    g, want, _ = _run(torch, restore, img, B, H, src, named,
                      lambda v, f, ids: restore.matrix_batch(H, src, v, f, stripe_ids=ids))
    assert np.array_equal(A.blocks(want, B)[:, 1:], clean)
    assert g[0, 1] == 0 and g[1, 13] == 0 and g[0, 6] == g[0, 12] == g[1, 3] == g[1, 10] == 600
    assert not g[2].any()                                               # clean: no counter, state 0


# ---- the two solvers

@gpu
def test_host_solve_agrees_with_device_solve(ecg, oracle, torch_cuda, restore, rs):
    """ecg_restore.ec (the host's elimination, the plan in the kernel arguments) against matrix_batch (the plan
    kernel's) on the same stripe, both against the definition, for sets of every state RS(10,4) has."""
    torch = torch_cuda
    M, H = rs
    code = ecg.ec_factory(ecg.ECTYPE.RS, ecg.CodingParameters(k=K, m=M_))
    src = list(range(N))
    for B in (1077, 9):
        clean = _encoded(oracle, M, 1, B, 81 + B)
        for E in ([5], [12], [10, 11, 12, 13], [13, 0, 11], [2, 4, 6, 8], [1, 10], [], [0, 1, 2, 3, 4]):
            rng = np.random.default_rng(82 + len(E))
            stripes = clean.copy()
            for i, b in enumerate(E or [3]):
                _hit(stripes, 0, b, (B * i) // 6, (B * (i + 3)) // 6, rng)
            named = np.zeros((1, N), np.uint8)
            named[0, E] = 1
            img = _arena(stripes, lead=0)

            def ec(v, f, ids):
                d, c = [v[0, j] for j in range(K)], [v[0, K + j] for j in range(M_)]
                return restore.ec(code, d, c, B, named[0])

            g1, want, a1 = _run(torch, restore, img, B, H, src, named, ec)
            g2, _, a2 = _run(torch, restore, img, B, H, src, named,
                             lambda v, f, ids: restore.matrix_batch(H, src, v, f, stripe_ids=ids))
            assert np.array_equal(g1, g2) and np.array_equal(a1, a2)
            assert np.array_equal(want, _arena(clean if 0 < len(E) <= M_ else stripes, lead=0))


# ---- the chain: verify -> names_from_sums -> rows -> restore -> verify

def _chain_image(stripes, pitch):
    S, n, B = stripes.shape
    img = np.full((S, n, pitch), A.BAND, np.uint8)
    img[:, :, :B] = stripes
    return img


@gpu
@pytest.mark.parametrize("layout", ["stride_multiple_of_P", "padded_stride"])
def test_chain_from_piece_sums(oracle, torch_cuda, restore, rs, layout):
    """RS(10,4), P = 2048, B = 4 * 2048 + 53.  Piece rows with 2, 3, 4 (the ragged last piece) and 5 damaged blocks:
    the verify answers n for all four and the heal's TARGET mode has nothing to do.  The restore brings the first three
    back exactly and leaves the fourth alone; a second verify shows exactly that row."""
    torch = torch_cuda
    import ecg_heal
    import ecg_psum
    M, H = rs
    P, B, S = 2048, 4 * 2048 + 53, 4
    Q = 5
    clean = _encoded(oracle, M, S, B, 91)
    rng = np.random.default_rng(92)
    stripes = clean.copy()
    rowsets = {(3, 0): [2, 11], (0, 2): [0, 10, 13], (1, 4): [5, 6, 12, 13], (3, 1): [1, 3, 7, 9, 12]}
    for (s, q), E in rowsets.items():
        for i, b in enumerate(E):
            _hit(stripes, s, b, q * P + 5 + 3 * i, q * P + (40 if q == 4 else 1500) + 3 * i, rng)
    pitch = 5 * P if layout == "stride_multiple_of_P" else B + 75
    assert (N * pitch % P == 0) == (layout == "stride_multiple_of_P")
    ids = [3, 0, 1]                                                     # stripe 2 is not selected
    sel = _ints(torch, ids)
    src = list(range(N))
    d_clean = A.to_dev(torch, _chain_image(clean, pitch))
    expected = ecg_psum.pieces_batch(src, d_clean[:, :, :B], P, stripe_ids=sel)
    img = _chain_image(stripes, pitch)
    d = A.to_dev(torch, img)
    view = d[:, :, :B]
    sums, targets, bad = ecg_psum.verify_batch(src, view, P, expected, stripe_ids=sel)
    t, b = targets.cpu().numpy(), bad.cpu().numpy()
    for (s, q), E in rowsets.items():
        assert t[ids.index(s), q] == N and b[ids.index(s), q] == len(E)
    assert (t == N).sum() == 4 and (t == -1).sum() == 3 * Q - 4
    assert ecg_psum.heal_rows(view, targets, P, stripe_ids=sel) == []   # TARGET has no row to heal ...
    ecg_heal.encode_batch(K, M_, M, view, stripe_ids=sel, targets=targets[:, 0].contiguous())
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), img)                         # ... and changes nothing when asked anyway

    named, count = restore.names_from_sums(sums, expected)
    assert np.array_equal(count.cpu().numpy(), b)
    nm = named.cpu().numpy()
    for (s, q), E in rowsets.items():
        assert np.flatnonzero(nm[ids.index(s), q]).tolist() == sorted(E)
    entries = restore.rows(view, sums, expected, P, stripe_ids=sel)
    assert len(entries) == (2 if layout == "stride_multiple_of_P" else 4)
    seen = 0
    for v, row_ids, row_named in entries:
        assert tuple(v.shape[1:]) in ((N, P), (N, 53)) and row_named.dtype == torch.uint8
        rep = restore.encode_batch(K, M_, M, v, row_named, stripe_ids=row_ids).cpu().numpy()
        seen += rep.shape[0]
        for row in rep:
            t_ = int(np.count_nonzero(row[:N]))
            assert (row[N + 2], t_) in ((0, 2), (0, 3), (0, 4), (2, 0)) and (row[N + 1] == 0) == (row[N + 2] == 0)
    assert seen == 4
    torch.cuda.synchronize()
    want = stripes.copy()
    for (s, q), E in rowsets.items():
        if len(E) <= M_:
            want[s, :, q * P:(q + 1) * P] = clean[s, :, q * P:(q + 1) * P]
    assert np.array_equal(d.cpu().numpy(), _chain_image(want, pitch))   # padding and stripe 2 included
    _, targets2, bad2 = ecg_psum.verify_batch(src, view, P, expected, stripe_ids=sel)
    t2, b2 = targets2.cpu().numpy(), bad2.cpu().numpy()
    assert t2[0, 1] == N and b2[0, 1] == 5 and (t2 == -1).sum() == 3 * Q - 1


@gpu
def test_chain_from_block_sums(oracle, torch_cuda, restore, rs):
    """Q = 1: ecg_sum's block sums; stripes with 2, 3, 4 and 5 damaged blocks and a clean one."""
    torch = torch_cuda
    import ecg_sum
    M, H = rs
    B, S = 1077, 5
    clean = _encoded(oracle, M, S, B, 95)
    rng = np.random.default_rng(96)
    stripes = clean.copy()
    sets = {0: [4, 13], 1: [0, 1, 2], 3: [9, 10, 11, 12], 4: [2, 3, 5, 8, 10]}
    for s, E in sets.items():
        for i, b in enumerate(E):
            _hit(stripes, s, b, 50 * i, 50 * i + 800, rng)
    src = list(range(N))
    d_clean = A.to_dev(torch, _arena(clean, lead=0))
    expected = ecg_sum.blocks_batch(src, A.blocks(d_clean, B))
    img = _arena(stripes, lead=0)
    d = A.to_dev(torch, img)
    view = A.blocks(d, B)
    sums, targets, bad = ecg_sum.verify_batch(src, view, expected)
    assert targets.cpu().numpy().tolist() == [N, N, -1, N, N]
    entries = restore.rows(view, sums, expected, None)
    assert sum(int(e[1].numel()) for e in entries) == 4
    for v, row_ids, row_named in entries:
        assert sorted(row_ids.cpu().numpy().tolist()) == [0, 1, 3, 4]
        rep = restore.encode_batch(K, M_, M, v, row_named, stripe_ids=row_ids).cpu().numpy()
        assert sorted(rep[:, N + 2].tolist()) == [0, 0, 0, 2]
    torch.cuda.synchronize()
    want = clean.copy()
    want[4] = stripes[4]
    assert np.array_equal(d.cpu().numpy(), _arena(want, lead=0))
    _, targets2, bad2 = ecg_sum.verify_batch(src, view, expected)
    assert targets2.cpu().numpy().tolist() == [-1, -1, -1, -1, N] and bad2.cpu().numpy().tolist() == [0, 0, 0, 0, 5]


@gpu
def test_rows_refuses_row_ids_past_int32(ecg, torch_cuda, restore):
    """A view whose stripe stride is 2^22 pieces: stripe 512's rows start at 2^31.  No byte of it is touched."""
    torch = torch_cuda
    base = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    stripes = torch.as_strided(base, (513, 2, 1024), (0, 512, 1))           # stride 0: handled per piece index
    expected = torch.zeros((1, 2, 2), dtype=torch.int32, device="cuda")
    sums = expected.clone()
    sums[0, :, 1] = 7                                                        # piece row 1: both columns differ
    got = restore.rows(stripes, sums, expected, 512, stripe_ids=_ints(torch, [512]))
    assert len(got) == 1 and got[0][1].tolist() == [512] and got[0][2].tolist() == [[1, 1]]
    assert tuple(got[0][0].shape) == (513, 2, 512)

    class Wide:                                                              # the shape and strides of a 2^40-byte view
        shape, device = (513, 2, 1024), base.device
        def stride(self, d): return (1 << 31, 512, 1)[d]
        def storage_offset(self): return 0
    with pytest.raises(ecg.EcgError) as e:
        restore.rows(Wide(), sums, expected, 512, stripe_ids=_ints(torch, [512]))
    assert e.value.code == ecg.ECG_EINVAL and "int32" in str(e.value)
    with pytest.raises(ecg.EcgError):                                        # piece sums need their piece size
        restore.rows(stripes, sums, expected, None, stripe_ids=_ints(torch, [512]))


# ---- empty calls

@gpu
def test_empty_calls(ecg, oracle, torch_cuda, restore, rs):
    torch = torch_cuda
    M, H = rs
    B = 100
    stripes = _encoded(oracle, M, 2, B, 99)
    stripes[0, 3, 10:20] ^= 0x5A
    img = _arena(stripes, lead=0)
    d = A.to_dev(torch, img)
    view = A.blocks(d, B)
    c0, l0 = restore.counters(), restore.last_launch()
    none = torch.empty((0,), dtype=torch.int32, device="cuda")
    flags0 = torch.empty((0, N), dtype=torch.uint8, device="cuda")
    assert tuple(restore.encode_batch(K, M_, M, view, flags0, stripe_ids=none).shape) == (0, N + 3)
    assert tuple(restore.matrix_batch(H, list(range(N)), view, flags0, stripe_ids=none).shape) == (0, N + 3)
    flags = torch.ones((2, N), dtype=torch.uint8, device="cuda")
    assert tuple(restore.encode_batch(K, M_, M, view[:, :, :0], flags).shape) == (2, N + 3)       # B = 0
    named, count = restore.names_from_sums(torch.empty((0, N, 3), dtype=torch.int32, device="cuda"),
                                           torch.empty((0, N, 3), dtype=torch.int32, device="cuda"))
    assert tuple(named.shape) == (0, 3, N) and tuple(count.shape) == (0, 3)
    torch.cuda.synchronize()
    assert restore.counters() == c0 and restore.last_launch() == l0
    assert np.array_equal(d.cpu().numpy(), img)
