"""The degraded range read on the GPU: the kernels of libecg_dread.so against the definition (tests/dread_plain.py over
tests/gf_plain.py's table), bit for bit.

Every case uploads a guard-band arena (tests/gf_arena.py) whose lost blocks are filled with garbage and an answer buffer
filled with a canary, runs one call and compares THE WHOLE ANSWER BUFFER, the full report and THE WHOLE ARENA (which
must be unchanged) with the definition, then `counters()` and `last_launch()`: a store outside a record's range or into
a refused record's bytes shows, a read of a lost block shows, and so does a call that ran only byte lanes.  The
definition's answers are themselves compared with the bytes the lost blocks held before they were lost.

Every test here loads libecg_dread.so and runs its kernels.
"""
import contextlib
import json
import os

import numpy as np
import pytest

import address_range_cases as AR
import dread_plain as DP
import gf_arena as A
import gf_plain
import heal2_plain as P2

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
GUARD = A.GUARD
CANARY, GARBAGE = 0xC9, 0xEE
B0, S0 = 4096 + 48, 6
THREADS = 128                                              # gf_kernels.hpp kThreads: the fewest columns per workgroup
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return torch


@pytest.fixture(scope="module")
def dread(ecg):
    import ecg_dread
    ecg_dread.lib()
    return ecg_dread


@contextlib.contextmanager
def _cols_per_wg(ecg, cpw):
    saved = ecg.get_option(ecg.ECG_OPT_COLS_PER_WG)
    try:
        ecg.set_option(ecg.ECG_OPT_COLS_PER_WG, cpw)
        yield
    finally:
        ecg.set_option(ecg.ECG_OPT_COLS_PER_WG, saved)


def _golden(name):
    return next(c for c in GOLDEN if c["name"] == name)


def _check(name):
    c = _golden(name)
    return c["k"], c["m"], DP.check_of(c["matrix"], c["k"], c["m"])


RS_CODES = ((4, 2), (10, 4))                                 # the setup of every test that names no other
RS_IDS = ["RS(4,2)", "RS(10,4)"]


def _rs(oracle, km):
    """(k, m, H = [M | I]) with M the oracle's Vandermonde coding matrix."""
    k, m = km
    return k, m, DP.check_of(oracle.reed_sol_vandermonde_coding_matrix(k, m), k, m)


def _codewords(H, k, S, B, seed):
    """[S][n][B] stripes under H = [G | I], parity by the plain product."""
    data = np.random.default_rng(seed).integers(0, 256, (S, k, B), dtype=np.uint8)
    return np.stack([np.concatenate([d, gf_plain.apply(H[:, :k], d)]) for d in data])


def _arena(stripes, lost, src=None, slots=None, pitch=None):
    """The arena image of [S][n][B] stripes, column j in slot src[j], lost blocks filled with garbage, slots no column
    names with 0x77."""
    S, n, B = stripes.shape
    src = list(range(n)) if src is None else src
    img = np.full((S, n if slots is None else slots, A.pitch(B) if pitch is None else pitch), A.BAND, np.uint8)
    img[:, :, GUARD:GUARD + B] = 0x77
    held = stripes.copy()
    held[np.asarray(lost).astype(bool)] = GARBAGE
    for j in range(n):
        img[:, src[j], GUARD:GUARD + B] = held[:, j]
    return img


def _geometry(ecg, max_len, R, max_reads):
    cols = (max_len + 30) >> 4
    cpw = ecg.get_option(ecg.ECG_OPT_COLS_PER_WG) or THREADS
    if cols < cpw:
        cpw = max(THREADS, -(-cols // THREADS) * THREADS)
    return {"cols_per_wg": cpw, "wg_per_record": max(1, -(-cols // cpw)), "R": R, "max_reads": max_reads}


def _pack(ranges, classes=(0,), gap=3):
    """out_off for lengths `ranges`: record i starts at the first offset past the previous answer (and a gap of canary)
    that is classes[i % len(classes)] mod 16.  Returns (offsets, out_bytes)."""
    at, offs = 1, []
    for i, ln in enumerate(ranges):
        while at % 16 != classes[i % len(classes)]:
            at += 1
        offs.append(at)
        at += ln + gap
    return offs, at + 5


def _run(torch, ecg, D, img, B, H, src, lost, recs, out_bytes, call, max_len=None, shift=0, truth=None):
    """Upload img (base `shift` bytes past a 16-byte boundary) and a canary-filled answer buffer, run
    call(view, lost, records, out) once and compare report, answer buffer, arena, counters and last launch with the
    definition.  truth: the [S][n][B] stripes before the loss -- an answered record's bytes are theirs.  Returns the
    report, numpy."""
    recs = np.asarray(recs, dtype=np.int64).reshape(-1, 5)
    max_len = B if max_len is None else max_len
    H = np.asarray(H, dtype=np.int64).reshape(-1, len(src))
    lost = np.asarray(lost).astype(bool)
    want_out = np.full(out_bytes, CANARY, np.uint8)
    want_rep = DP.dread(H, src, A.blocks(img, B), lost, recs, max_len, want_out)
    if truth is not None:
        for (s, col, off, ln, at), st in zip(recs.tolist(), want_rep[:, 0]):
            if st == 0:
                assert np.array_equal(want_out[at:at + ln], truth[s, col, off:off + ln]), (s, col, off, ln)
    d = A.to_dev(torch, img, shift)
    d_out = torch.full((out_bytes,), CANARY, dtype=torch.uint8, device="cuda")
    c0, l0 = D.counters(), D.last_launch()
    out, got = call(A.blocks(d, B), lost, recs, d_out)
    torch.cuda.synchronize()
    c1, l1 = D.counters(), D.last_launch()
    assert out is d_out and got.dtype == torch.int32 and tuple(got.shape) == (len(recs), 2)
    g = got.cpu().numpy().astype(np.int64)
    assert np.array_equal(g, want_rep), (B, shift, np.argwhere(g != want_rep)[:4].tolist(), g[:8].tolist())
    got_out = d_out.cpu().numpy()
    assert np.array_equal(got_out, want_out), ("answer buffer", np.flatnonzero(got_out != want_out)[:8].tolist())
    assert np.array_equal(d.cpu().numpy(), img), "the arena changed"
    assert c1["launches"] - c0["launches"] == (1 if len(recs) else 0)
    assert c1["records"] - c0["records"] == len(recs)
    if shift % 16 == 0 and img.shape[2] % 16 == 0 and len(recs) > 0 and max_len > 0:
        assert l1 == _geometry(ecg, max_len, len(recs), int(np.count_nonzero(H.any(axis=0)))), l1
    else:
        assert l1 == l0                                                  # byte lanes only, or nothing: the record stays
    return g


def _lost_by_stripe(n, counts, seed):
    """[len(counts)][n] flags: stripe s loses counts[s] columns."""
    rng = np.random.default_rng(seed)
    lost = np.zeros((len(counts), n), bool)
    for s, t in enumerate(counts):
        lost[s, rng.choice(n, t, replace=False)] = True
    return lost


# ---- 1. alignment classes

@gpu
@pytest.mark.parametrize("cpw", (128, 256))
@pytest.mark.parametrize("km", RS_CODES, ids=RS_IDS)
def test_alignment_classes(ecg, oracle, torch_cuda, dread, km, cpw):
    """off % 16 in {0, 5} x out_off % 16 in {0, 9} x nine lengths around a column and a chunk, lost and present
    columns alike, in one call per geometry: at 128 columns per workgroup the longest records span three workgroups."""
    torch = torch_cuda
    k, m, H = _rs(oracle, km)
    n, chunk = k + m, 16 * cpw
    stripes = _codewords(H, k, S0, B0, 11)
    lost = _lost_by_stripe(n, [0, 1, m, 2, 1, m][:S0], 12)
    recs, lens, classes = [], [], []
    i = 0
    for offc in (0, 5):
        for outc in (0, 9):
            for ln in (0, 1, 15, 16, 17, chunk - 1, chunk, chunk + 1, None):
                s = 1 + i % (S0 - 1)                                     # stripes 1..5 are degraded
                col = int(np.flatnonzero(lost[s])[i % lost[s].sum()]) if i % 3 else (i * 7) % n
                off = offc + 16 * (i % 5)
                ln = B0 - off if ln is None else min(ln, B0 - off)
                recs.append([s, col, off, ln, 0])
                lens.append(ln)
                classes.append(outc)
                i += 1
    offs, out_bytes = _pack(lens, classes)
    for rec, at in zip(recs, offs):
        rec[4] = at
    assert DP.check_records(recs, n, B0, S0, B0, out_bytes) == -1
    order = np.random.default_rng(13).permutation(len(recs))
    recs = [recs[i] for i in order]
    matrix = [int(v) for v in H[:, :k].reshape(-1)]
    with _cols_per_wg(ecg, cpw):
        g = _run(torch, ecg, dread, _arena(stripes, lost), B0, H, list(range(n)), lost, recs, out_bytes,
                 lambda v, f, r, o: dread.encode_batch(k, m, matrix, v, f, r, o, max_len=B0), truth=stripes)
        assert dread.last_launch()["wg_per_record"] == -(-((B0 + 30) >> 4) // cpw) > 1
    assert not g[:, 0].any() and set(g[:, 1].tolist()) == {1, k}


# ---- 2. mixed stripes in one call

@gpu
@pytest.mark.parametrize("km", RS_CODES, ids=RS_IDS)
def test_mixed_stripes(torch_cuda, ecg, oracle, dread, km):
    """t = 0 (copies), t = 1, t = r, lost parities only, and present blocks read from degraded stripes."""
    torch = torch_cuda
    k, m, H = _rs(oracle, km)
    n = k + m
    stripes = _codewords(H, k, S0, B0, 21)
    lost = np.zeros((S0, n), bool)
    lost[1, 3] = True                                                    # t = 1
    lost[2, :m] = True                                                   # t = r, data
    lost[3, k:] = True                                                   # the parities
    lost[4, [0, k]] = True
    lost[5, list(range(k - m + 1, k)) + [n - 1]] = True                  # t = r, mixed
    rng = np.random.default_rng(22)
    recs, want_reads = [], []
    for s in range(S0):
        cols = sorted(set(np.flatnonzero(lost[s]).tolist() + [0, k - 1, n - 1]))
        for col in cols:
            off = int(rng.integers(0, B0 - 700))
            recs.append([s, col, off, int(rng.integers(1, 700)), 0])
            want_reads.append(k if lost[s, col] else 1)
    offs, out_bytes = _pack([r[3] for r in recs], classes=(0, 9, 4))
    for rec, at in zip(recs, offs):
        rec[4] = at
    g = _run(torch, ecg, dread, _arena(stripes, lost), B0, H, list(range(n)), lost, recs, out_bytes,
             lambda v, f, r, o: dread.matrix_batch(H, list(range(n)), v, f, r, o, max_len=700), max_len=700,
             truth=stripes)
    assert not g[:, 0].any() and g[:, 1].tolist() == want_reads


# ---- 3. an LRC answers from the local group

@gpu
def test_lrc_local_group(torch_cuda, ecg, dread):
    """Azure(8,2,2) with five lost blocks, more than its four parities: a block that is alone in its local group is
    answered from the group (reads 4); a block of the group that lost three is state 6 and nothing is written."""
    torch = torch_cuda
    k, m, H = _check("Azure(8,2,2)")
    n, B, S = k + m, B0, 2
    local = [q for q in range(m) if np.count_nonzero(H[q, :k]) == k // 2]
    assert len(local) == 2
    group = [np.flatnonzero(H[q, :k]).tolist() for q in local]
    glob = [k + q for q in range(m) if q not in local]
    stripes = _codewords(H, k, S, B, 31)
    lost = np.zeros((S, n), bool)
    lost[0, [group[0][1]] + group[1][:3] + [glob[0]]] = True
    assert lost[0].sum() == 5
    recs = [[0, group[0][1], 100, 1000, 0], [0, group[1][0], 100, 1000, 0], [0, group[1][3], 5, 333, 0],
            [1, 2, 0, 64, 0], [0, glob[0], 7, 90, 0]]
    offs, out_bytes = _pack([r[3] for r in recs], classes=(9, 0))
    for rec, at in zip(recs, offs):
        rec[4] = at
    g = _run(torch, ecg, dread, _arena(stripes, lost), B, H, list(range(n)), lost, recs, out_bytes,
             lambda v, f, r, o: dread.matrix_batch(H, list(range(n)), v, f, r, o, max_len=1000), max_len=1000,
             truth=stripes)
    # the lost global parity is the all-ones row: the sum of the two local parities, which survive -- two reads
    assert not H[glob[0] - k, :k].tolist().count(0) and g.tolist() == [[0, 4], [6, 0], [0, 1], [0, 1], [0, 2]]


# ---- 4. refused records

@gpu
@pytest.mark.parametrize("km", RS_CODES, ids=RS_IDS)
def test_refused_records(torch_cuda, ecg, oracle, dread, km):
    """Every state 1-6 in one batch beside answered records; the refused records' canaries stay."""
    torch = torch_cuda
    k, m, H = _rs(oracle, km)
    n, max_len = k + m, 600
    stripes = _codewords(H, k, S0, B0, 41)
    lost = np.zeros((S0, n), bool)
    lost[0, [2, n - 1]] = True
    lost[1, :m + 1] = True                                               # m + 1 lost: none of them is recoverable
    good = [[0, 2, 17, 600, 0], [0, n - 1, 0, 16, 0], [2, 1, 4000, 144, 0], [1, n - 1, 300, 31, 0], [0, 0, 0, 0, 0]]
    offs, out_bytes = _pack([r[3] for r in good] + [64] * 12, classes=(0, 9))
    for rec, at in zip(good, offs):
        rec[4] = at
    at = offs[len(good):]
    bad = [[S0, 0, 0, 16, at[0]], [-1, 0, 0, 16, at[1]], [0, n, 32, 16, at[2]], [1, -1, 32, 16, at[3]],
           [0, 0, -16, 32, at[4]], [0, 0, 16, -1, at[5]], [2, 3, B0 - 15, 16, at[6]], [3, 2, 0, max_len + 1, at[7]],
           [0, 1, 64, 32, -1], [0, 1, 64, 32, out_bytes - 31], [1, 1, 64, 64, at[8]], [1, 0, 0, 1, at[9]],
           [7, n + 1, -1, B0 + 1, -1]]
    states = [1, 1, 2, 2, 3, 3, 3, 4, 5, 5, 6, 6, 1]
    recs = np.array(good + bad, dtype=np.int64)
    order = np.random.default_rng(42).permutation(len(recs))
    g = _run(torch, ecg, dread, _arena(stripes, lost), B0, H, list(range(n)), lost, recs[order], out_bytes,
             lambda v, f, r, o: dread.matrix_batch(H, list(range(n)), v, f, r, o, max_len=max_len), max_len=max_len,
             truth=stripes)
    where = {int(o): p for p, o in enumerate(order)}
    assert [int(g[where[len(good) + i], 0]) for i in range(len(bad))] == states
    assert not any(g[where[len(good) + i], 1] for i in range(len(bad)))
    assert g[[where[i] for i in range(len(good))]].tolist() == [[0, k], [0, k], [0, 1], [0, 1], [0, 1]]
    first = dread.check_records(recs[order], n, B0, S0, max_len, out_bytes)
    assert first == DP.check_records(recs[order], n, B0, S0, max_len, out_bytes)
    assert first == int(np.flatnonzero((g[:, 0] != 0) & (g[:, 0] != 6))[0])      # state 6 is not the helper's to see


# ---- 5. a wide check

@gpu
def test_wide_check(torch_cuda, ecg, dread):
    """k = 120, m = 8: n = 128 columns, so the plan's lanes hold two columns each, and a 120-source loop."""
    torch = torch_cuda
    k, m, B, S = 120, 8, 256, 2
    n = k + m
    CM = P2.cauchy(m, k)
    H = DP.check_of(CM, k, m)
    stripes = _codewords(H, k, S, B, 51)
    lost = np.zeros((S, n), bool)
    lost[0, [1, 40, 63, 64, 70, 100, 121, 127]] = True                   # t = 8, either side of lane 64
    lost[1, [64, 119, 120]] = True
    recs = [[0, 1, 0, 256, 0], [0, 64, 3, 250, 0], [0, 127, 16, 48, 0], [0, 63, 0, 17, 0], [0, 121, 255, 1, 0],
            [0, 65, 5, 77, 0], [1, 119, 0, 256, 0], [1, 120, 9, 100, 0], [1, 127, 0, 256, 0]]
    offs, out_bytes = _pack([r[3] for r in recs], classes=(0, 9))
    for rec, at in zip(recs, offs):
        rec[4] = at
    g = _run(torch, ecg, dread, _arena(stripes, lost), B, H, list(range(n)), lost, recs, out_bytes,
             lambda v, f, r, o: dread.encode_batch(k, m, [int(v) for v in CM.reshape(-1)], v, f, r, o), truth=stripes)
    assert g.tolist() == [[0, k]] * 5 + [[0, 1]] + [[0, k]] * 2 + [[0, 1]]


# ---- 6. every golden code through the class's own check

@gpu
@pytest.mark.parametrize("c", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_ec_batch_on_every_golden_code(ecg, torch_cuda, dread, c):
    """Classes whose check has at most 8 rows answer through ecg_ec_check_matrix; the others are refused."""
    torch = torch_cuda
    code = ecg.ec_factory(c["type"], ecg.CodingParameters(**c["params"]))
    k, m, B, S = code.k, code.m, 1077, 3
    n = k + m
    if m > 8:
        d = A.to_dev(torch, A.blank(S, n, B))
        with pytest.raises(ecg.EcgError) as e:
            dread.ec_batch(code, A.blocks(d, B), np.zeros((S, n), bool), [[0, 0, 0, 8, 0]], 64)
        assert e.value.code == ecg.ECG_EINVAL and b"dread: r = " in ecg.lib().ecg_last_error()
        return
    H = np.asarray(code.check_matrix(), dtype=np.int64).reshape(m, n)
    rng = np.random.default_rng(60 + n)
    if "matrix" in c:
        assert np.array_equal(H, DP.check_of(c["matrix"], k, m))
        stripes = _codewords(H, k, S, B, 61)
    else:                                                                # no matrix: the class's own encode
        dev = torch.from_numpy(rng.integers(0, 256, (S, n, B), dtype=np.uint8)).cuda()
        for s in range(S):
            code.encode([dev[s, j] for j in range(k)], [dev[s, k + j] for j in range(m)], B)
        torch.cuda.synchronize()
        stripes = dev.cpu().numpy()
    assert not np.stack([gf_plain.apply(H, st) for st in stripes]).any()
    lost = _lost_by_stripe(n, [1, 2, min(m, 3)], 62)
    recs = []
    for s in range(S):
        for col in sorted(set(np.flatnonzero(lost[s]).tolist() + [int(rng.integers(0, n))])):
            off = int(rng.integers(0, B - 400))
            recs.append([s, col, off, int(rng.integers(1, 400)), 0])
    offs, out_bytes = _pack([r[3] for r in recs], classes=(0, 9, 2))
    for rec, at in zip(recs, offs):
        rec[4] = at
    g = _run(torch, ecg, dread, _arena(stripes, lost), B, H, list(range(n)), lost, recs, out_bytes,
             lambda v, f, r, o: dread.ec_batch(code, v, f, r, o, max_len=400), max_len=400, truth=stripes)
    assert (g[:, 0] == 0).any()


# ---- 7. unaligned layouts

@gpu
@pytest.mark.parametrize("km", RS_CODES, ids=RS_IDS)
def test_unaligned_layout(torch_cuda, ecg, oracle, dread, km):
    """Base + 1 and an odd pitch: no block is 16-byte aligned, every byte takes the byte lanes; the answers are those
    of the aligned layout and last_launch stays as it was."""
    torch = torch_cuda
    k, m, H = _rs(oracle, km)
    n, S = k + m, 3
    stripes = _codewords(H, k, S, B0, 71)
    lost = _lost_by_stripe(n, [1, m, 2], 72)
    rng = np.random.default_rng(73)
    recs = []
    for s in range(S):
        for col in np.flatnonzero(lost[s]).tolist() + [int(rng.integers(0, n))]:
            off = int(rng.integers(0, B0 - 1500))
            recs.append([s, col, off, int(rng.integers(1, 1500)), 0])
    offs, out_bytes = _pack([r[3] for r in recs], classes=(0, 9))
    for rec, at in zip(recs, offs):
        rec[4] = at
    odd = GUARD + B0 + GUARD + (1 - (B0 & 1))
    assert odd % 2 == 1
    call = lambda v, f, r, o: dread.matrix_batch(H, list(range(n)), v, f, r, o, max_len=1500)
    got = [_run(torch, ecg, dread, _arena(stripes, lost, pitch=pitch), B0, H, list(range(n)), lost, recs, out_bytes,
                call, max_len=1500, shift=shift, truth=stripes)
           for pitch, shift in ((None, 0), (None, 1), (odd, 0), (odd, 1))]
    assert all(np.array_equal(g, got[0]) for g in got[1:]) and not got[0][:, 0].any()


# ---- 8. the primitive with scrambled ids

@gpu
@pytest.mark.parametrize("km", RS_CODES, ids=RS_IDS)
def test_permuted_src_ids(torch_cuda, ecg, oracle, dread, km):
    """src_ids in scrambled block order over 16 slots, two of which the check does not name."""
    torch = torch_cuda
    k, m, H = _rs(oracle, km)
    n, S, B = k + m, 3, B0
    rng = np.random.default_rng(81)
    slots = [int(v) for v in rng.permutation(16)]
    src = slots[:n]
    stripes = _codewords(H, k, S, B, 82)
    lost = _lost_by_stripe(n, [2, m, 1], 83)
    recs = []
    for s in range(S):
        for col in np.flatnonzero(lost[s]).tolist() + [int(rng.integers(0, n))]:
            off = int(rng.integers(0, B - 500))
            recs.append([s, col, off, int(rng.integers(1, 500)), 0])
    offs, out_bytes = _pack([r[3] for r in recs], classes=(9, 0))
    for rec, at in zip(recs, offs):
        rec[4] = at
    g = _run(torch, ecg, dread, _arena(stripes, lost, src=src, slots=16), B, H, src, lost, recs, out_bytes,
             lambda v, f, r, o: dread.matrix_batch(H, src, v, f, r, o, max_len=500), max_len=500, truth=stripes)
    assert not g[:, 0].any()


# ---- 9. addresses past 2^32

@gpu
@pytest.mark.parametrize("shift", AR.SHIFTS_A, ids=["aligned", "shifted"])
def test_addresses_past_4gib(torch_cuda, dread, shift):
    """Part A's layout of tests/address_range_cases.py: two stripes of six 4693-byte blocks whose strides put the
    blocks past 2^31, 2^32 and 2^33 in a 24.1 GiB arena of which only the twelve windows are ever touched.  k = 2,
    m = 4 Cauchy; the lost blocks are rebuilt from survivors that include both stripes' last block."""
    torch = torch_cuda
    k, m, n, B = AR.K, AR.R, AR.N, AR.B_A
    CM = P2.cauchy(m, k)
    H = DP.check_of(CM, k, m)
    clean, _ = AR.stripes_a(gf_plain.apply, CM, False)
    lost = np.zeros((AR.S_A, n), bool)
    lost[0, [0, 2, 3, 4]] = True                                         # survivors: blocks 1 and 5
    lost[1, [1, 4]] = True
    held = clean.copy()
    held[lost] = GARBAGE
    recs = np.array([[1, 1, 17, 2100, 3], [0, 0, B - 900, 900, 2200], [1, 4, 3000, 1693, 3200], [0, 4, 5, 11, 5000],
                     [1, 5, 2117, 16, 5100], [0, 3, 0, B, 5200]], dtype=np.int64)
    out_bytes = 5200 + B + 9
    assert DP.check_records(recs, n, B, AR.S_A, B, out_bytes) == -1
    want_out = np.full(out_bytes, CANARY, np.uint8)
    want_rep = DP.dread(H, list(range(n)), held, lost, recs, B, want_out)
    assert want_rep.tolist() == [[0, 2], [0, 2], [0, 2], [0, 2], [0, 1], [0, 2]]
    for s, col, off, ln, at in recs.tolist():
        assert np.array_equal(want_out[at:at + ln], clean[s, col, off:off + ln])
    arena = torch.empty(AR.ARENA_A, dtype=torch.uint8, device="cuda")
    try:
        for (_, _, lo, hi), row in zip(AR.windows_a(shift), AR.image_a(held)):
            arena[lo:hi].copy_(torch.from_numpy(row.copy()))
        view = arena.as_strided((AR.S_A, n, B), (AR.SS_A, AR.BS_A, 1), AR.BASE_A + shift)
        d_out = torch.full((out_bytes,), CANARY, dtype=torch.uint8, device="cuda")
        _, got = dread.encode_batch(k, m, [int(v) for v in CM.reshape(-1)], view, lost, recs, d_out)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want_rep)
        assert np.array_equal(d_out.cpu().numpy(), want_out)
        after = np.stack([arena[lo:hi].cpu().numpy() for _, _, lo, hi in AR.windows_a(shift)])
        assert np.array_equal(after, AR.image_a(held)), np.argwhere(after != AR.image_a(held))[:4].tolist()
    finally:
        del arena
        torch.cuda.empty_cache()


# ---- 10. nothing to move

@gpu
@pytest.mark.parametrize("km", RS_CODES, ids=RS_IDS)
def test_max_len_zero_and_no_records(torch_cuda, ecg, oracle, dread, km):
    """max_len == 0: records with len > 0 are state 4, empty ones are answered with their plan's reads, no byte moves
    and last_launch stays.  R == 0: no launch at all."""
    torch = torch_cuda
    k, m, H = _rs(oracle, km)
    n, S, B = k + m, 2, B0
    stripes = _codewords(H, k, S, B, 91)
    lost = np.zeros((S, n), bool)
    lost[0, [1, 2]] = True
    lost[1, [0] + list(range(n - m, n))] = True                          # m + 1 lost
    recs = [[0, 1, 5, 0, 3], [0, 1, 5, 1, 3], [1, 0, 0, 0, 0], [1, 1, B, 0, 64], [0, 3, 0, 16, 20]]
    call = lambda v, f, r, o: dread.matrix_batch(H, list(range(n)), v, f, r, o, max_len=0)
    g = _run(torch, ecg, dread, _arena(stripes, lost), B, H, list(range(n)), lost, recs, 64, call, max_len=0)
    assert g.tolist() == [[0, k], [4, 0], [6, 0], [0, 1], [4, 0]]
    g = _run(torch, ecg, dread, _arena(stripes, lost), B, H, list(range(n)), lost, np.zeros((0, 5), np.int64), 64, call,
             max_len=0)
    assert g.shape == (0, 2)
    d = A.to_dev(torch, _arena(stripes, lost))
    out, rep = dread.encode_batch(k, m, [int(v) for v in H[:, :k].reshape(-1)], A.blocks(d, B), lost, [[0, 1, 5, 0, 0]], 0)
    torch.cuda.synchronize()
    assert out.numel() == 0 and rep.cpu().tolist() == [[0, k]]           # an answer buffer of no bytes at all


# ---- 11. batch scope and stream

@gpu
@pytest.mark.parametrize("km", RS_CODES, ids=RS_IDS)
def test_batch_scope_flushes_first_and_side_stream_orders(ecg, oracle, torch_cuda, dread, km):
    torch = torch_cuda
    k, m, H = _rs(oracle, km)
    n, B = k + m, B0
    stripes = _codewords(H, k, 1, B, 101)
    stale = stripes.copy()
    stale[:, k:] = 0x11                                                  # parities not yet encoded
    lost = np.zeros((1, n), bool)
    lost[0, [2, n - 2]] = True
    recs = [[0, 2, 10, 900, 0], [0, n - 2, 0, B, 1000], [0, n - 1, 5, 50, 5200]]
    out_bytes = 5300
    want = np.full(out_bytes, CANARY, np.uint8)
    want_rep = DP.dread(H, list(range(n)), _arena(stripes, lost)[:, :, GUARD:GUARD + B], lost, recs, B, want)
    code = ecg.ec_factory(ecg.ECTYPE.RS, ecg.CodingParameters(k=k, m=m))
    assert np.array_equal(np.asarray(code.check_matrix(), dtype=np.int64).reshape(m, n), H)
    matrix = [int(v) for v in H[:, :k].reshape(-1)]
    img = _arena(stale, np.zeros((1, n), bool))                          # every data block present for the encode
    d = A.to_dev(torch, img)
    v = A.blocks(d, B)
    d_out = torch.full((out_bytes,), CANARY, dtype=torch.uint8, device="cuda")
    with ecg.batch():                                                    # the encode is recorded, not launched ...
        code.encode([v[0, j] for j in range(k)], [v[0, k + j] for j in range(m)], B)
        _, rep = dread.encode_batch(k, m, matrix, v, lost, recs, d_out)  # ... until this call flushes the scope
    torch.cuda.synchronize()
    assert np.array_equal(rep.cpu().numpy(), want_rep) and np.array_equal(d_out.cpu().numpy(), want)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                        # upload, read and copy back on one stream
        d2 = A.to_dev(torch, _arena(stripes, lost))
        out2 = torch.full((out_bytes,), CANARY, dtype=torch.uint8, device="cuda")
        _, rep2 = dread.encode_batch(k, m, matrix, A.blocks(d2, B), lost, recs, out2)
        after = out2.clone()
    side.synchronize()
    assert np.array_equal(after.cpu().numpy(), want) and np.array_equal(rep2.cpu().numpy(), want_rep)
