"""The delta update on the GPU: the kernels of libecg_update.so against the definition (tests/update_plain.py over
tests/gf_plain.py's table) and, for whole stripes, against the oracle's encode of the new data.

Every case uploads a guard-band arena (tests/gf_arena.py) and a band-filled staging and delta buffer, runs one call and
compares THE WHOLE ARENA, THE WHOLE DELTA BUFFER and the full report with the definition, then `counters()` and
`last_launch()`: a store outside a record's range, into a parity whose coefficient is zero or into a refused record's
bytes shows, and so does a call that ran only byte lanes.

Every test here loads libecg_update.so and runs its kernels.
"""
import json
import os

import numpy as np
import pytest

import address_range_cases as AR
import gf_arena as A
import gf_plain
import heal2_plain as P2
import update_plain as UP

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
MATRIX_CODES = [c for c in GOLDEN if "matrix" in c]
GUARD = A.GUARD
K, M_ = 10, 4
N = K + M_
B0 = 4693
THREADS = 128                                              # gf_kernels.hpp kThreads: 16-byte columns per workgroup
MAX_NNZ = 8                                                # update_kernels.hpp kUpdateMaxNnz
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return torch


@pytest.fixture(scope="module")
def update(ecg):
    import ecg_update
    ecg_update.lib()
    return ecg_update


@pytest.fixture(scope="module")
def rs(oracle):
    """RS(10,4) from the oracle, as a flat list."""
    return oracle.reed_sol_vandermonde_coding_matrix(K, M_)


def _encode(oracle, k, m, M, data):
    """[S][k][B] data -> [S][k+m][B] stripes, parity by the oracle's encode."""
    S, _, B = data.shape
    out = np.zeros((S, k + m, B), np.uint8)
    for s in range(S):
        d = [data[s, j].copy() for j in range(k)]
        c = [np.zeros(B, np.uint8) for _ in range(m)]
        oracle.jerasure_matrix_encode(k, m, M, d, c, B)
        out[s] = np.stack(d + c)
    return out


def _plain_stripes(G, k, S, B, seed):
    """[S][k+m][B] stripes, parity by the plain product."""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, (S, k, B), dtype=np.uint8)
    G = np.asarray(G, dtype=np.int64).reshape(-1, k)
    return np.stack([np.concatenate([d, gf_plain.apply(G, d)]) for d in data])


def _arena(stripes, lead=0, pitch=None):
    """The arena image of [S][n][B] stripes: `lead` slots no call names (0x77) in front of them."""
    S, n, B = stripes.shape
    img = np.full((S, lead + n, A.pitch(B) if pitch is None else pitch), A.BAND, np.uint8)
    img[:, :lead, GUARD:GUARD + B] = 0x77
    img[:, lead:, GUARD:GUARD + B] = stripes
    return img


def _geometry(max_len, R, max_nnz):
    cols = (max_len + 30) >> 4
    return {"cols_per_wg": THREADS, "wg_per_record": max(1, -(-cols // THREADS)), "R": R, "max_nnz": max_nnz}


def _staging(rng, in_bytes):
    return rng.integers(0, 256, in_bytes, dtype=np.uint8)


def _run(torch, U, img, B, G, src, dst, recs, data_in, call, mode=UP.WRITE, max_len=None, with_delta=True, shift=0):
    """Upload img (base `shift` bytes past a 16-byte boundary), the staging buffer and a band-filled delta buffer, run
    call(view, records, staging, delta or None) once and compare report, arena, delta buffer, counters and last launch
    with the definition.  Returns (report, expected image, expected delta buffer), numpy."""
    recs = np.asarray(recs, dtype=np.int64).reshape(-1, 5)
    max_len = B if max_len is None else max_len
    G = np.asarray(G, dtype=np.int64).reshape(len(dst), len(src))
    want = img.copy()
    want_delta = np.full(data_in.size, A.BAND, np.uint8)
    want_rep = UP.update(G, src, dst, A.blocks(want, B), recs, data_in, mode, max_len,
                         want_delta if with_delta else None)
    d = A.to_dev(torch, img, shift)
    d_in = torch.from_numpy(data_in).cuda()
    d_delta = torch.full((data_in.size,), A.BAND, dtype=torch.uint8, device="cuda")
    c0, l0 = U.counters(), U.last_launch()
    got = call(A.blocks(d, B), recs, d_in, d_delta if with_delta else None)
    torch.cuda.synchronize()
    c1, l1 = U.counters(), U.last_launch()
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(recs), 2)
    g = got.cpu().numpy().astype(np.int64)
    assert np.array_equal(g, want_rep), (B, shift, np.argwhere(g != want_rep)[:4].tolist(), g[:8].tolist())
    written = {(int(r[0]), b) for r, st in zip(recs, want_rep[:, 0]) if st == 0
               for b in [src[int(r[1])]] + [dst[i] for i in range(len(dst)) if G[i, int(r[1])]]}
    A.assert_same(d.cpu().numpy(), want, B, lambda s, slot: (s, slot) in written, (B, shift, mode))
    got_delta = d_delta.cpu().numpy()
    assert np.array_equal(got_delta, want_delta), ("delta buffer", np.flatnonzero(got_delta != want_delta)[:8])
    assert c1["launches"] - c0["launches"] == (1 if len(recs) else 0)
    assert c1["records"] - c0["records"] == len(recs)
    vec = shift % 16 == 0 and img.shape[2] % 16 == 0 and len(recs) > 0 and max_len > 0
    if vec:
        assert l1 == _geometry(max_len, len(recs), int(np.count_nonzero(G, axis=0).max())), l1
    else:
        assert l1 == l0                                                  # byte lanes only: the record stays
    return g, want, want_delta


def _matrix_call(U, G, src, dst, max_len, mode=UP.WRITE):
    return lambda v, r, i, dl: U.matrix_batch(G, src, dst, v, r, i, mode=mode, max_len=max_len, delta_out=dl)


# ---- 1. alignment classes

OFFS = (0, 1, 15, 16, 17)
LENS = (0, 1, 15, 16, 17, 31, 33, 2048, 2049, None)          # None: B - off


def _in_off(at, off, cls):
    """The first staging offset >= at that is congruent to off mod 16 (cls 0), mod 4 but not mod 16 (1), or at an odd
    distance from it (2)."""
    want = {0: lambda d: d % 16 == 0, 1: lambda d: d % 4 == 0 and d % 16 != 0, 2: lambda d: d % 2 == 1}[cls]
    while not want(at - off):
        at += 1
    return at


@gpu
@pytest.mark.parametrize("length", LENS, ids=[str(v) if v is not None else "to_end" for v in LENS])
def test_alignment_classes(oracle, torch_cuda, update, rs, length):
    """A stripe per off in {0, 1, 15, 16, 17}; short records are repeated 64 bytes apart over all ten columns.
    max_len = B: most workgroups exit early.  One call per staging alignment class."""
    torch = torch_cuda
    S = len(OFFS)
    stripes = _encode(oracle, K, M_, rs, np.random.default_rng(11).integers(0, 256, (S, K, B0), dtype=np.uint8))
    img = _arena(stripes, lead=1)
    src, dst = list(range(1, K + 1)), list(range(K + 1, N + 1))
    for cls in range(3):
        rng = np.random.default_rng(100 + cls)
        recs, at = [], 1
        for s, off in enumerate(OFFS):
            ln = B0 - off if length is None else length
            reps = 10 if ln <= 33 else 1
            for j in range(reps):
                o = off + 64 * j
                at = _in_off(at, o, cls)
                recs.append([s, (s + 3 * j + cls) % K, o, ln, at])
                at += ln
        recs = [recs[i] for i in rng.permutation(len(recs))]
        g, want, _ = _run(torch, update, img, B0, rs, src, dst, recs, _staging(rng, at + 7),
                          _matrix_call(update, rs, src, dst, B0))
        assert not g[:, 0].any()
        new = A.blocks(want, B0)[:, 1:]
        assert np.array_equal(new, _encode(oracle, K, M_, rs, new[:, :K]))     # a codeword again, by the oracle


# ---- 2. a codeword again

@gpu
def test_codeword_again(oracle, torch_cuda, update, rs):
    torch = torch_cuda
    import ecg_scrub
    S = 4
    rng = np.random.default_rng(21)
    stripes = _encode(oracle, K, M_, rs, rng.integers(0, 256, (S, K, B0), dtype=np.uint8))
    recs, in_bytes = UP.legal_records(rng, 3, K, B0, 12, 700)              # stripe 3 is not touched
    assert UP.check_records(recs, K, B0, S, 700, in_bytes, True) == -1
    img = _arena(stripes)
    data_in = _staging(rng, in_bytes)
    d = {}

    def call(v, r, i, dl):
        d["view"] = v
        return update.encode_batch(K, M_, rs, v, r, i, max_len=700, delta_out=dl)

    g, want, _ = _run(torch, update, img, B0, rs, list(range(K)), list(range(K, N)), recs, data_in, call, max_len=700)
    assert not g[:, 0].any() and g[:, 1].sum() > 0
    new = A.blocks(want, B0)
    assert np.array_equal(new, _encode(oracle, K, M_, rs, new[:, :K]))
    counts = ecg_scrub.encode_batch(K, M_, rs, d["view"]).cpu().numpy()
    touched = update.touched_stripes(recs, torch.from_numpy(g.astype(np.int32)))
    assert touched.dtype == torch.int32 and touched.is_cuda and touched.cpu().tolist() == [0, 1, 2]
    assert not counts[touched.cpu().numpy()].any() and not counts.any()


# ---- 3. records that share a 16-byte column

@gpu
def test_shared_columns(torch_cuda, update, rs):
    """256 stripes of 64 bytes.  Pairs of touching records cut a 16-byte column at every position 1..15, triples at
    [0,a) [a,b) [b,16), in the same block and in different blocks: every workgroup stores bytes of a column that
    another workgroup also stores to.  One call, once: a whole-column read-modify-write would drop bytes."""
    torch = torch_cuda
    S, B = 256, 64
    stripes = _plain_stripes(rs, K, S, B, 31)
    groups = []                                                            # lists of cut points inside one column
    for p in range(1, 16):
        groups += [[0, p, 16]] * 2
    groups += [[0, a, b, 16] for a in range(1, 15) for b in range(a + 1, 16)]
    recs, at = [], 0
    for i, cuts in enumerate(groups):
        s, q = divmod(i, 4)                                                # four columns per stripe
        same = i % 2 == 0                                                  # one block, or a block per piece
        for t, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
            col = (i % K) if same else (i + 1 + 3 * t) % K
            recs.append([s, col, 16 * q + lo, hi - lo, at])
            at += hi - lo + (i + t) % 3
    assert recs[-1][0] < S and UP.check_records(recs, K, B, S, 16, at, True) == -1
    rng = np.random.default_rng(32)
    recs = [recs[i] for i in rng.permutation(len(recs))]
    g, want, _ = _run(torch, update, _arena(stripes), B, rs, list(range(K)), list(range(K, N)), recs,
                      _staging(rng, at), lambda v, r, i, dl: update.encode_batch(K, M_, rs, v, r, i, max_len=16,
                                                                                 delta_out=dl), max_len=16)
    assert not g[:, 0].any()
    new = A.blocks(want, B)
    assert np.array_equal(new[:, K:], np.stack([gf_plain.apply(np.asarray(rs).reshape(M_, K), d) for d in new[:, :K]]))


# ---- 4. refused records

@gpu
def test_refused_records(oracle, torch_cuda, update, rs):
    torch = torch_cuda
    S, max_len = 3, 600
    rng = np.random.default_rng(41)
    stripes = _encode(oracle, K, M_, rs, rng.integers(0, 256, (S, K, B0), dtype=np.uint8))
    legal, in_bytes = UP.legal_records(rng, S, K, B0, 5, max_len)
    bad = [[S, 0, 0, 16, 0], [-1, 0, 0, 16, 0], [0, K, 32, 16, 0], [1, -1, 32, 16, 0], [0, 0, -16, 32, 0],
           [0, 0, 16, -1, 0], [2, 3, B0 - 15, 16, 0], [1, 2, 0, max_len + 1, 0], [0, 1, 64, 32, -1],
           [0, 1, 64, 32, in_bytes - 31], [7, K + 1, -1, B0 + 1, -1]]
    states = [1, 1, 2, 2, 3, 3, 3, 4, 5, 5, 1]
    recs = np.concatenate([legal, np.array(bad, dtype=np.int64)])
    order = rng.permutation(len(recs))
    recs = recs[order]
    g, want, want_delta = _run(torch, update, _arena(stripes, lead=1), B0, rs, list(range(1, K + 1)),
                               list(range(K + 1, N + 1)), recs, _staging(rng, in_bytes),
                               lambda v, r, i, dl: update.matrix_batch(rs, list(range(1, K + 1)),
                                                                       list(range(K + 1, N + 1)), v, r, i,
                                                                       max_len=max_len, delta_out=dl), max_len=max_len)
    where = {int(o): p for p, o in enumerate(order)}
    assert [int(g[where[len(legal) + i], 0]) for i in range(len(bad))] == states
    assert not any(g[where[len(legal) + i], 1] for i in range(len(bad)))
    assert not g[[where[i] for i in range(len(legal))], 0].any()
    first = update.check_records(recs, K, B0, S, max_len, in_bytes, True)
    assert first == int(np.flatnonzero(g[:, 0])[0]) == UP.check_records(recs, K, B0, S, max_len, in_bytes, True)
    for i in range(len(recs)):                                             # record by record: the device's state
        alone = update.check_records(recs[i:i + 1], K, B0, S, max_len, in_bytes)
        assert (alone == 0) == (g[i, 0] != 0)
    assert update.touched_stripes(recs, torch.from_numpy(g.astype(np.int32))).cpu().tolist() == [0, 1, 2]


# ---- 5. DELTA mode

@gpu
def test_delta_mode(ecg, oracle, torch_cuda, update, rs):
    torch = torch_cuda
    S = 3
    rng = np.random.default_rng(51)
    stripes = _encode(oracle, K, M_, rs, rng.integers(0, 256, (S, K, B0), dtype=np.uint8))
    recs, in_bytes = UP.legal_records(rng, S, K, B0, 8, 900)
    img = _arena(stripes)
    src, dst = list(range(K)), list(range(K, N))
    data_in = _staging(rng, in_bytes)
    g, want, delta = _run(torch, update, img, B0, rs, src, dst, recs, data_in, _matrix_call(update, rs, src, dst, B0))
    covered = np.zeros(in_bytes, bool)
    for _, _, _, ln, in_off in recs:
        covered[in_off:in_off + ln] = True
    fed = np.where(covered, delta, 0x5A).astype(np.uint8)                  # delta where WRITE wrote it, junk elsewhere
    g2, want2, _ = _run(torch, update, img, B0, rs, src, dst, recs, fed,
                        _matrix_call(update, rs, src, dst, B0, mode=UP.DELTA), mode=UP.DELTA, with_delta=False)
    assert np.array_equal(g2, g)
    assert np.array_equal(A.blocks(want2, B0)[:, :K], stripes[:, :K])      # data blocks bit-identical
    assert np.array_equal(A.blocks(want2, B0)[:, K:], A.blocks(want, B0)[:, K:])
    d = A.to_dev(torch, img)
    with pytest.raises(ecg.EcgError) as e:                                 # DELTA has no delta to give back
        update.matrix_batch(rs, src, dst, A.blocks(d, B0), recs, torch.from_numpy(fed).cuda(), mode=UP.DELTA,
                            delta_out=torch.zeros(in_bytes, dtype=torch.uint8, device="cuda"))
    assert e.value.code == ecg.ECG_EINVAL and b"ECG_UPDATE_DELTA" in ecg.lib().ecg_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), img)


# ---- 6. idempotence

@gpu
def test_new_equal_to_old_changes_nothing(oracle, torch_cuda, update, rs):
    torch = torch_cuda
    S = 3
    rng = np.random.default_rng(61)
    stripes = _encode(oracle, K, M_, rs, rng.integers(0, 256, (S, K, B0), dtype=np.uint8))
    recs, in_bytes = UP.legal_records(rng, S, K, B0, 8, 1200)
    data_in = _staging(rng, in_bytes)
    for s, col, off, ln, in_off in recs:
        data_in[in_off:in_off + ln] = stripes[s, col, off:off + ln]
    img = _arena(stripes)
    src, dst = list(range(K)), list(range(K, N))
    g, want, delta = _run(torch, update, img, B0, rs, src, dst, recs, data_in, _matrix_call(update, rs, src, dst, B0))
    assert np.array_equal(want, img) and not g.any()
    covered = np.zeros(in_bytes, bool)
    for _, _, _, ln, in_off in recs:
        covered[in_off:in_off + ln] = True
    assert not delta[covered].any() and (delta[~covered] == A.BAND).all()  # zeros inside the ranges only


# ---- 7. zero coefficients and wide codes through the ec forms

@gpu
@pytest.mark.parametrize("c", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_ec_batch_on_every_golden_code(ecg, torch_cuda, update, c):
    """Codes whose class defines an encoding matrix with at most 8 nonzeros per column are updated and scrub clean
    through the class's own check; every other code is refused."""
    torch = torch_cuda
    import ecg_scrub
    code = ecg.ec_factory(c["type"], ecg.CodingParameters(**c["params"]))
    k, m, B, S = code.k, code.m, 1077, 3
    rng = np.random.default_rng(70 + k + m)
    G = np.asarray(c["matrix"], dtype=np.int64).reshape(m, k) if "matrix" in c else None
    recs, in_bytes = UP.legal_records(rng, S, k, B, 4, 400)
    if G is None or np.count_nonzero(G, axis=0).max() > MAX_NNZ:
        d = A.to_dev(torch, A.blank(S, k + m, B))
        with pytest.raises(ecg.EcgError) as e:
            update.ec_batch(code, A.blocks(d, B), recs, torch.zeros(in_bytes, dtype=torch.uint8, device="cuda"))
        assert e.value.code == ecg.ECG_EINVAL
        return
    assert code.make_encoding_matrix() == [int(v) for v in G.reshape(-1)]
    stripes = _plain_stripes(G, k, S, B, 71)
    d = {}

    def call(v, r, i, dl):
        d["view"] = v
        return update.ec_batch(code, v, r, i, max_len=400, delta_out=dl)

    g, want, _ = _run(torch, update, _arena(stripes), B, G, list(range(k)), list(range(k, k + m)), recs,
                      _staging(rng, in_bytes), call, max_len=400)
    assert not g[:, 0].any()
    assert not ecg_scrub.ec_batch(code, d["view"]).cpu().numpy().any()


@gpu
def test_ec_on_one_stripe(ecg, oracle, torch_cuda, update, rs):
    """ecg_update_ec: one record through the block pointers of an RS(10,4) stripe, the record in the kernel
    arguments; a column out of range is state 2 and moves nothing."""
    torch = torch_cuda
    code = ecg.ec_factory(ecg.ECTYPE.RS, ecg.CodingParameters(k=K, m=M_))
    rng = np.random.default_rng(75)
    stripes = _encode(oracle, K, M_, rs, rng.integers(0, 256, (1, K, B0), dtype=np.uint8))
    img = _arena(stripes)
    src, dst = list(range(K)), list(range(K, N))
    for col, off, ln, mode, state in ((3, 17, 2500, UP.WRITE, 0), (9, 0, B0, UP.WRITE, 0), (0, 4000, 5, UP.DELTA, 0),
                                      (K, 16, 64, UP.WRITE, 2), (2, B0 - 10, 11, UP.WRITE, 3)):
        def ec(v, r, i, dl):
            data, coding = [v[0, j] for j in range(K)], [v[0, K + j] for j in range(M_)]
            return update.ec(code, data, coding, B0, col, off, i, mode=mode, delta_out=dl)

        g, _, _ = _run(torch, update, img, B0, rs, src, dst, [[0, col, off, ln, 0]], _staging(rng, ln), ec, mode=mode,
                       max_len=min(ln, B0), with_delta=mode == UP.WRITE)
        assert g[0, 0] == state


# ---- 8. unaligned layouts

@gpu
def test_unaligned_layout(oracle, torch_cuda, update, rs):
    """Base + 1 and an odd pitch: no block is 16-byte aligned, every byte takes the byte lanes; the results are those
    of the aligned layout and last_launch stays as it was."""
    torch = torch_cuda
    S = 3
    rng = np.random.default_rng(81)
    stripes = _encode(oracle, K, M_, rs, rng.integers(0, 256, (S, K, B0), dtype=np.uint8))
    recs, in_bytes = UP.legal_records(rng, S, K, B0, 6, 1500)
    data_in = _staging(rng, in_bytes)
    odd = GUARD + B0 + GUARD + (1 - (B0 & 1))
    assert odd % 2 == 1
    src, dst = list(range(1, K + 1)), list(range(K + 1, N + 1))
    got = []
    for img, shift in ((_arena(stripes, lead=1), 0), (_arena(stripes, lead=1), 1), (_arena(stripes, lead=1, pitch=odd), 0),
                       (_arena(stripes, lead=1, pitch=odd), 1)):
        g, want, delta = _run(torch, update, img, B0, rs, src, dst, recs, data_in, _matrix_call(update, rs, src, dst, B0),
                              shift=shift)
        got.append((g, A.blocks(want, B0).copy(), delta))
    for g, blocks, delta in got[1:]:
        assert np.array_equal(g, got[0][0]) and np.array_equal(blocks, got[0][1]) and np.array_equal(delta, got[0][2])


# ---- 9. the primitive with scrambled ids

@gpu
def test_permuted_primitive(torch_cuda, update, rs):
    """src_ids / dst_ids in scrambled block order over 16 slots, two of which the matrix does not name."""
    torch = torch_cuda
    S, B = 3, 1077
    rng = np.random.default_rng(91)
    slots = [int(v) for v in rng.permutation(16)]
    src, dst, unnamed = slots[:K], slots[K:N], slots[N:]
    G = np.asarray(rs, dtype=np.int64).reshape(M_, K)
    plain = _plain_stripes(rs, K, S, B, 92)
    img = A.blank(S, 16, B, fill=0x77)
    for j in range(K):
        A.blocks(img, B)[:, src[j]] = plain[:, j]
    for i in range(M_):
        A.blocks(img, B)[:, dst[i]] = plain[:, K + i]
    recs, in_bytes = UP.legal_records(rng, S, K, B, 6, 500)
    g, want, _ = _run(torch, update, img, B, G, src, dst, recs, _staging(rng, in_bytes),
                      _matrix_call(update, G, src, dst, 500), max_len=500)
    new = A.blocks(want, B)
    assert (new[:, unnamed] == 0x77).all()
    for s in range(S):
        assert np.array_equal(new[s][dst], gf_plain.apply(G, new[s][src]))


# ---- 10. addresses past 2^32

@gpu
@pytest.mark.parametrize("shift", AR.SHIFTS_A, ids=["aligned", "shifted"])
def test_addresses_past_4gib(torch_cuda, update, shift):
    """Part A's layout of tests/address_range_cases.py: two stripes of six 4693-byte blocks whose strides put the
    blocks past 2^31, 2^32 and 2^33 in a 24.1 GiB arena of which only the twelve windows are ever touched.  k = 2,
    m = 4 Cauchy; the records hit both stripes' last data block and with it every parity, the last block included."""
    torch = torch_cuda
    k, m, n, B = AR.K, AR.R, AR.N, AR.B_A
    CM = P2.cauchy(m, k)
    flat = [int(v) for v in CM.reshape(-1)]
    clean, _ = AR.stripes_a(gf_plain.apply, CM, False)
    rng = np.random.default_rng(101)
    recs = np.array([[1, 1, 17, 2100, 3], [0, 1, B - 900, 900, 2200], [1, 0, 3000, 1693, 3200], [0, 0, 5, 11, 5000],
                     [1, 1, 2117, 16, 5100]], dtype=np.int64)
    in_bytes = 5200
    assert UP.check_records(recs, k, B, AR.S_A, B, in_bytes, True) == -1
    data_in = _staging(rng, in_bytes)
    want = clean.copy()
    want_delta = np.full(in_bytes, A.BAND, np.uint8)
    want_rep = UP.update(CM, list(range(k)), list(range(k, n)), want, recs, data_in, UP.WRITE, B, want_delta)
    assert np.array_equal(want[:, k:], np.stack([gf_plain.apply(CM, d) for d in want[:, :k]]))
    arena = torch.empty(AR.ARENA_A, dtype=torch.uint8, device="cuda")
    try:
        for (_, _, lo, hi), row in zip(AR.windows_a(shift), AR.image_a(clean)):
            arena[lo:hi].copy_(torch.from_numpy(row.copy()))
        view = arena.as_strided((AR.S_A, n, B), (AR.SS_A, AR.BS_A, 1), AR.BASE_A + shift)
        d_delta = torch.full((in_bytes,), A.BAND, dtype=torch.uint8, device="cuda")
        got = update.encode_batch(k, m, flat, view, recs, torch.from_numpy(data_in).cuda(), delta_out=d_delta)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want_rep)
        after = np.stack([arena[lo:hi].cpu().numpy() for _, _, lo, hi in AR.windows_a(shift)])
        assert np.array_equal(after, AR.image_a(want)), np.argwhere(after != AR.image_a(want))[:4].tolist()
        assert np.array_equal(d_delta.cpu().numpy(), want_delta)
    finally:
        del arena
        torch.cuda.empty_cache()


# ---- 11. batch scope and stream

@gpu
def test_batch_scope_flushes_first_and_side_stream_orders(ecg, oracle, torch_cuda, update, rs):
    torch = torch_cuda
    B = 1077
    rng = np.random.default_rng(111)
    data = rng.integers(0, 256, (1, K, B), dtype=np.uint8)
    stripes = _encode(oracle, K, M_, rs, data)
    stale = stripes.copy()
    stale[:, K:] = 0x11                                                    # parities not yet encoded
    recs, in_bytes = UP.legal_records(rng, 1, K, B, 6, 300)
    data_in = _staging(rng, in_bytes)
    want = stripes.copy()
    UP.update(rs, list(range(K)), list(range(K, N)), want, recs, data_in, UP.WRITE, 300)
    code = ecg.ec_factory(ecg.ECTYPE.RS, ecg.CodingParameters(k=K, m=M_))
    d = A.to_dev(torch, _arena(stale))
    v = A.blocks(d, B)
    d_in = torch.from_numpy(data_in).cuda()
    with ecg.batch():                                                      # the encode is recorded, not launched ...
        code.encode([v[0, j] for j in range(K)], [v[0, K + j] for j in range(M_)], B)
        rep = update.encode_batch(K, M_, rs, v, recs, d_in, max_len=300)  # ... until this call flushes the scope
    torch.cuda.synchronize()
    assert not rep.cpu().numpy()[:, 0].any()
    assert np.array_equal(d.cpu().numpy(), _arena(want))

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                          # upload, update and read back on one stream
        d2 = A.to_dev(torch, _arena(stripes))
        d_in2 = torch.from_numpy(data_in).cuda()
        rep2 = update.encode_batch(K, M_, rs, A.blocks(d2, B), recs, d_in2, max_len=300)
        after = d2.clone()
    side.synchronize()
    assert np.array_equal(after.cpu().numpy(), _arena(want)) and np.array_equal(rep2.cpu().numpy(), rep.cpu().numpy())
