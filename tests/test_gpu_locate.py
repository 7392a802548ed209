"""Corruption localisation on the GPU: every gf_locate_kernel / gf_locate_byte_kernel of libecg_locate.so against
the definition (tests/locate_plain.py), which tries every error value for every candidate block instead of the
kernels' pivot-row ratio test.

Shapes are the smallest at which the kernels can go wrong: B = 4693 (gf_kernel_cases.B_MAIN: two full 2 KiB
workgroup chunks, a partial third whose last wave is partly past the end, a 5-byte tail), B = 5 (byte path only),
S = 3 strided stripes with 64-byte bands of 0xC3 around every block and a block the check does not name.  Stripes
that satisfy their check are built with tests/gf_plain.py (or the oracle's encode), never with the library's own
encode; damage is sparse, so the reference stays cheap: stripe 0 is clean, stripe 1 has single bytes at the column,
chunk and tail edges in the first, a middle and the last block, stripe 2 two blocks damaged at one position, a run
in one block and a tail byte in another.

A check H = [C | I] over consecutive blocks folds only C through the tables; the same check with its columns
reversed is a general H over the same stripes, every column through the tables.  The sweep runs both on every R,
with k covering every load-batch branch and remainder, and a zero column in each form.

INLINE (pointers in the kernel arguments) is reached through ecg_locate.ec, whose matrix is the handle's own:
RS(k, r) gives [C | I] checks of r = 1..8 rows, PC(k1, 1, k2, 1) general ones of r = 3..8.

Wide checks (n = 62..65, 126..128; tests/check_geometry_cases.py wide_plan) damage every block, so that the counters of
all three registers, every word of the packed pivots and the whole ratio program are compared with the definition.
The launch geometries (workgroup -> chunk maps, column-loop lengths) are tests/test_gpu_check_geometry.py's.
"""
import json
import os

import numpy as np
import pytest

import check_geometry_cases as G
import gf_kernel_cases as C
import gf_plain
import locate_plain as LP

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
MATRIX_CODES = [c for c in GOLDEN if "matrix" in c]   # RS, ERS and the LRC family
GUARD, BAND = 64, 0xC3
S3 = 3
K_SWEEP = (1, 2, 3, 4, 5, 7, 9, 14)   # every load-batch branch and remainder (batches of 4 and 2)
B_MAIN, B_BYTES = C.B_MAIN, C.B_BYTES
POSITIONS = (0, 15, 16, 2047, 2048, B_MAIN - 6, B_MAIN - 1)   # column, chunk and tail edges of B_MAIN
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return torch


@pytest.fixture(scope="module")
def locate(ecg):
    import ecg_locate
    ecg_locate.lib()
    return ecg_locate


@pytest.fixture(scope="module")
def scrub(ecg):
    import ecg_scrub
    ecg_scrub.lib()
    return ecg_scrub


# ---- arenas

def _pitch(B):
    return (GUARD + B + GUARD + 15) & ~15  # every block 16-byte aligned in an aligned arena


def _arena(blocks):
    """[S][slots][pitch] host image of [S][slots][B] block bytes inside bands of 0xC3."""
    S, slots, B = blocks.shape
    img = np.full((S, slots, _pitch(B)), BAND, np.uint8)
    img[:, :, GUARD:GUARD + B] = blocks
    return img


def _to_dev(torch, img, shift=0):
    flat = torch.empty(img.size + 16, dtype=torch.uint8, device="cuda")
    view = flat[shift:shift + img.size]
    view.copy_(torch.from_numpy(img.reshape(-1)))
    return view.view(img.shape)


def _consistent(Cm, S, B, seed):
    """[S][k + r][B] stripes with H = [Cm | I] satisfied: random data, gf_plain's product as parity."""
    r, k = Cm.shape
    rng = np.random.default_rng(seed)
    out = np.zeros((S, k + r, B), np.uint8)
    for s in range(S):
        out[s, :k] = rng.integers(0, 256, (k, B), dtype=np.uint8)
        out[s, k:] = gf_plain.apply(Cm, out[s, :k])
    return out


def _damage(stripes, seed):
    """Sparse damage, in place, by the module's plan (stripe 0 stays clean).  Works for any block size."""
    S, n, B = stripes.shape
    rng = np.random.default_rng(seed)
    trio = (0, n // 2, n - 1)
    pos = [p for p in POSITIONS if p < B] if B >= 64 else list(range(B))
    for i, p in enumerate(pos):
        stripes[1, trio[i % 3], p] ^= rng.integers(1, 256, dtype=np.uint8)
    if S > 2:
        mid = B // 2
        stripes[2, 0, mid] ^= 0x5A                               # two blocks at one position
        stripes[2, n - 1, mid] ^= 0xC3
        lo, hi = (B // 3, min(B // 3 + 40, mid)) if B >= 64 else (0, 1)
        stripes[2, n // 2, lo:hi] ^= rng.integers(1, 256, hi - lo, dtype=np.uint8)  # a run that crosses columns
        stripes[2, min(1, n - 1), B - 1] ^= 0x01                 # and the last tail byte


def _check_call(torch, locate, img, d, B, shift, H, src, call, sel=None, memo=None):
    """Run `call`, compare its votes with the definition row by row of the selection, the arena with what was
    uploaded, and the counters with the declared launches and bytes.  Returns the votes (numpy).  memo: a dict that
    keeps the definition's votes per stripe between calls over the same H and image."""
    H = np.asarray(H, dtype=np.int64)
    n = H.shape[1]
    rows = list(range(img.shape[0])) if sel is None else list(sel)
    c0 = locate.counters()
    got = call()
    torch.cuda.synchronize()
    c1 = locate.counters()
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(rows), n + 2)
    memo = {} if memo is None else memo
    for s in set(rows) - set(memo):
        memo[s] = LP.votes(H, img[s][src, GUARD:GUARD + B])
    want = np.stack([memo[s] for s in rows])
    g = got.cpu().numpy().astype(np.int64)
    assert np.array_equal(g, want), (H.shape, B, shift, sel, g, want)
    assert np.array_equal(d.cpu().numpy(), img), "the locate wrote to its inputs"
    vec = (B & ~15) if shift % 16 == 0 else 0
    assert c1["launches"] - c0["launches"] == (vec > 0) + (vec < B)
    assert c1["bytes"] - c0["bytes"] == len(rows) * B * n
    return g


def _sel(torch, ids):
    return None if ids is None else torch.tensor(list(ids), dtype=torch.int32, device="cuda")


def _strided_case(torch, locate, r, k, B, shift=0, sels=(None,), zero_col=False):
    """One random C (r x k): H = [C | I] over blocks 1.., then the same check with its columns reversed (a general
    H).  zero_col: column 0 of C is zeroed -- damage in that block is invisible, and it is never a candidate."""
    Cm = C.matrix(C._case("strided", 0, r, k, B_MAIN))
    if zero_col:
        Cm[:, 0] = 0
    stripes = _consistent(Cm, S3, B, 1000 * r + 10 * k + B)
    _damage(stripes, 7 * r + k)
    n = k + r
    blocks = np.concatenate([np.full((S3, 1, B), 0x77, np.uint8), stripes], axis=1)   # slot 0 is not named
    img = _arena(blocks)
    d = _to_dev(torch, img, shift)
    view = d[:, :, GUARD:GUARD + B]
    H = np.concatenate([Cm, np.eye(r, dtype=np.int64)], axis=1)
    src = list(range(1, n + 1))
    for ids in sels:
        g = _check_call(torch, locate, img, d, B, shift, H, src,
                        lambda: locate.matrix_batch(H, src, view, stripe_ids=_sel(torch, ids)), sel=ids)
        clean_row = 0 if ids is None else list(ids).index(0)
        assert not g[clean_row].any()                            # the clean stripe's row is all zero
        Hr, srcr = H[:, ::-1].copy(), src[::-1]
        gr = _check_call(torch, locate, img, d, B, shift, Hr, srcr,
                         lambda: locate.matrix_batch(Hr, srcr, view, stripe_ids=_sel(torch, ids)), sel=ids)
        assert np.array_equal(gr[:, :n], g[:, n - 1::-1][:, :n]) and np.array_equal(gr[:, n:], g[:, n:])
        if zero_col:
            assert not g[:, 0].any()


@gpu
@pytest.mark.parametrize("r", range(1, 9), ids=[f"r{r}" for r in range(1, 9)])
def test_every_r_strided(torch_cuda, locate, r):
    for k in K_SWEEP:
        _strided_case(torch_cuda, locate, r, k, B_MAIN)
    _strided_case(torch_cuda, locate, r, 7, B_BYTES)
    _strided_case(torch_cuda, locate, r, 5, B_MAIN, zero_col=True)
    _strided_case(torch_cuda, locate, r, 3, B_MAIN, sels=([2, 0],))


def _inline_codes(ecg, r):
    F, P = ecg.ec_factory, ecg.CodingParameters
    out = [(F(ecg.ECTYPE.RS, P(k=3 + r % 5, m=r)), True)]
    if r >= 3:
        k1 = r // 2
        out.append((F(ecg.ECTYPE.PC, P(k1=k1, m1=1, k2=r - 1 - k1, m2=1)), False))
    return out


@gpu
@pytest.mark.parametrize("r", range(1, 9), ids=[f"r{r}" for r in range(1, 9)])
def test_every_r_inline(ecg, torch_cuda, locate, r):
    torch = torch_cuda
    for code, ident in _inline_codes(ecg, r):
        k, m = code.k, code.m
        assert m == r
        n = k + m
        H = np.asarray(code.check_matrix(), dtype=np.int64)
        assert np.array_equal(H[:, k:], np.eye(m, dtype=np.int64)) == ident
        for B in (B_MAIN, B_BYTES):
            # [C | I]: a stripe with random data; a product code's check reads parities too: the zero stripe
            stripes = _consistent(H[:, :k], 3, B, 77 * r + B) if ident else np.zeros((3, n, B), np.uint8)
            _damage(stripes, 5 * r + B)
            for s in range(3):
                img = _arena(np.concatenate([np.full((1, 1, B), 0x77, np.uint8), stripes[s:s + 1]], axis=1))
                d = _to_dev(torch, img)
                blocks = [d[0, 1 + b, GUARD:GUARD + B] for b in range(n)]
                _check_call(torch, locate, img, d, B, 0, H, list(range(1, n + 1)),
                            lambda: locate.ec(code, blocks[:k], blocks[k:], B))


# ---- planted single bytes, garbage, selection

RS64 = next(c for c in GOLDEN if c["name"] == "RS(6,4)")


def _rs64(S, B, seed):
    M = np.asarray(RS64["matrix"], dtype=np.int64).reshape(4, 6)
    return M, _consistent(M, S, B, seed)


def _planted(torch, locate, shift):
    k, m, B = 6, 4, B_MAIN
    n = k + m
    assert B == 4693 and POSITIONS[-2] == (B & ~15) - 1
    M, stripes = _rs64(S3, B, 64)
    img = _arena(np.concatenate([np.zeros((S3, 1, B), np.uint8), stripes], axis=1))
    d = _to_dev(torch, img, shift)
    view = d[:, 1:, GUARD:GUARD + B]  # slot 0 is not named
    flat = [int(v) for v in M.reshape(-1)]
    assert not locate.encode_batch(k, m, flat, view).cpu().numpy().any()  # clean: nothing written
    for block in (0, 4, n - 1):
        for pos in POSITIONS:
            d[1, 1 + block, GUARD + pos] ^= 0x21
            got = locate.encode_batch(k, m, flat, view).cpu().numpy()
            d[1, 1 + block, GUARD + pos] ^= 0x21
            want = np.zeros((S3, n + 2), np.int32)
            want[1, block] = want[1, n] = 1
            assert np.array_equal(got, want), (block, pos, got)
            assert locate.verdict(got[1]) == (block, [block]) and locate.verdict(got[0]) == (LP.CLEAN, [])
    assert np.array_equal(d.cpu().numpy(), img)


@gpu
def test_planted_single_bytes(torch_cuda, locate):
    _planted(torch_cuda, locate, 0)


@gpu
def test_unaligned_base_runs_the_byte_kernel(torch_cuda, locate):
    """The arena shifted by one byte: no block is 16-byte aligned, one byte-kernel launch covers everything
    (_check_call counts the launches)."""
    _planted(torch_cuda, locate, 1)
    for r, k in ((1, 4), (4, 7), (8, 3)):
        _strided_case(torch_cuda, locate, r, k, B_MAIN, shift=1, sels=(None, [2, 0]))


@gpu
def test_whole_block_garbage_and_selection(torch_cuda, locate):
    """Stripe 0 clean, stripe 1 with data block 3 replaced by garbage, stripe 2 with parity block 8 replaced; every
    selection returns its rows in its own order, and a stripe that is not selected contributes nothing."""
    torch = torch_cuda
    k, m, B = 6, 4, B_MAIN
    n = k + m
    M, stripes = _rs64(S3, B, 67)
    rng = np.random.default_rng(9)
    stripes[1, 3] = rng.integers(0, 256, B, dtype=np.uint8)
    stripes[2, 8] = rng.integers(0, 256, B, dtype=np.uint8)
    img = _arena(stripes)
    d = _to_dev(torch, img)
    view = d[:, :, GUARD:GUARD + B]
    flat = [int(v) for v in M.reshape(-1)]
    H = np.concatenate([M, np.eye(m, dtype=np.int64)], axis=1)
    full, memo = None, {}
    for ids in (None, [2, 0], [1], [0], [1, 1, 2]):
        g = _check_call(torch, locate, img, d, B, 0, H, list(range(n)),
                        lambda: locate.encode_batch(k, m, flat, view, stripe_ids=_sel(torch, ids)), sel=ids,
                        memo=memo)
        if ids is None:
            full = g
            assert not g[0].any() and g[1, 3] == g[1, n] > 0.98 * B and g[2, 8] == g[2, n] > 0.98 * B
            assert [locate.verdict(row)[0] for row in g] == [LP.CLEAN, 3, 8]
        else:
            assert np.array_equal(g, full[ids])


@gpu
def test_votes_are_overwritten_not_accumulated(torch_cuda, locate):
    torch = torch_cuda
    k, m, B = 6, 4, B_MAIN
    n = k + m
    M, stripes = _rs64(S3, B, 65)
    flat = [int(v) for v in M.reshape(-1)]
    d = torch.from_numpy(stripes).cuda()
    out = torch.full((S3, n + 2), -1, dtype=torch.int32, device="cuda")  # 0xFFFFFFFF
    assert locate.encode_batch(k, m, flat, d, out=out) is out
    assert not out.cpu().numpy().any()
    _damage(stripes, 3)
    H = np.concatenate([M, np.eye(m, dtype=np.int64)], axis=1)
    want = np.stack([LP.votes(H, stripes[s]) for s in range(S3)])
    assert want[1:].any()
    d.copy_(torch.from_numpy(stripes))
    for _ in range(2):
        out.fill_(-1)
        locate.encode_batch(k, m, flat, d, out=out)
        assert np.array_equal(out.cpu().numpy(), want)
    two = torch.full((2, n + 2), 7, dtype=torch.int32, device="cuda")
    locate.encode_batch(k, m, flat, d, stripe_ids=_sel(torch, [2, 0]), out=two)
    assert np.array_equal(two.cpu().numpy(), want[[2, 0]])


@gpu
def test_locate_flushes_the_batch_scope(ecg, torch_cuda, locate):
    """A dev_matrix_encode recorded in a batch scope, then a locate of the same blocks inside the scope: the locate
    flushes the scope first, so it sees the encode's result (no bad position), not the stale parity."""
    torch = torch_cuda
    k, m, B = 6, 4, B_MAIN
    M, stripes = _rs64(1, B, 66)
    flat = [int(v) for v in M.reshape(-1)]
    want_parity = stripes[0, k:].copy()
    stripes[0, k:] = 0xA5  # stale
    d = torch.from_numpy(stripes).cuda()
    assert locate.encode_batch(k, m, flat, d).cpu().numpy()[0, k + m] > 0.9 * B  # stale parity: bad nearly everywhere
    with ecg.batch():
        ecg.dev_matrix_encode(k, m, flat, [d[0, j] for j in range(k)], [d[0, k + j] for j in range(m)], B)
        votes = locate.encode_batch(k, m, flat, d)
    torch.cuda.synchronize()
    assert not votes.cpu().numpy().any()
    assert np.array_equal(d[0, k:].cpu().numpy(), want_parity)


# ---- the ErasureCode facade

@gpu
@pytest.mark.parametrize("c", MATRIX_CODES, ids=[c["name"] for c in MATRIX_CODES])
def test_facade(ecg, oracle, torch_cuda, locate, c):
    """Stripe 0 as the oracle encoded it, stripe 1 + b with a byte range and the last byte of block b damaged:
    ec_batch's votes equal the definition's and the verdict names block b (RS(8,1), r = 1: every block ties); ec
    over one stripe's pointers agrees."""
    from oracle import ec_ref as E
    torch = torch_cuda
    B = B_MAIN
    ref = E.ec_factory(c["type"], E.CodingParameters(**c["params"]))
    code = ecg.ec_factory(c["type"], ecg.CodingParameters(**c["params"]))
    k, m = code.k, code.m
    n = k + m
    rng = np.random.default_rng(k * 100 + m)
    data = [rng.integers(0, 256, B, dtype=np.uint8) for _ in range(k)]
    coding = E.zeros(m, B)
    ref.encode(data, coding, B)
    clean = np.stack(data + list(coding))
    stripes = np.repeat(clean[None], n + 1, axis=0)
    for b in range(n):
        lo = (37 * b) % (B - 40)
        stripes[1 + b, b, lo:lo + 40] ^= rng.integers(1, 256, 40, dtype=np.uint8)
        stripes[1 + b, b, B - 1] ^= 0x01  # and the last tail byte
    H = np.asarray(code.check_matrix(), dtype=np.int64)
    want = np.stack([LP.votes(H, stripes[s]) for s in range(n + 1)])
    d = torch.from_numpy(stripes).cuda()
    got = locate.ec_batch(code, d).cpu().numpy()
    assert np.array_equal(got, want), c["name"]
    assert locate.verdict(got[0]) == (LP.CLEAN, [])
    for b in range(n):
        assert got[1 + b, n] == 41 and got[1 + b, n + 1] == 0
        if m == 1:
            assert locate.verdict(got[1 + b]) == (LP.AMBIGUOUS, list(range(n)))
        else:
            assert locate.verdict(got[1 + b]) == (b, [b]), (c["name"], b, got[1 + b])
    sel = _sel(torch, [n, 1])
    assert np.array_equal(locate.ec_batch(code, d, stripe_ids=sel).cpu().numpy(), want[[n, 1]])
    for s in (0, 1, n):
        one = locate.ec(code, [d[s, j] for j in range(k)], [d[s, k + j] for j in range(m)], B).cpu().numpy()
        assert np.array_equal(one[0], want[s]), (c["name"], s)
    assert np.array_equal(d.cpu().numpy(), stripes)


@gpu
@pytest.mark.parametrize("name", ["PC(4,2,2,1)", "PC(4,1,4,1)"])
def test_larger_codes_are_refused(ecg, torch_cuda, locate, name):
    """r > 8 (PC(4,1,4,1) has r = 9): ECG_EINVAL with the reason, nothing launched."""
    torch = torch_cuda
    c = next(g for g in GOLDEN if g["name"] == name)
    code = ecg.ec_factory(c["type"], ecg.CodingParameters(**c["params"]))
    assert code.m > 8
    n = code.k + code.m
    d = torch.zeros((2, n, 64), dtype=torch.uint8, device="cuda")
    l0 = locate.counters()["launches"]
    with pytest.raises(ecg.EcgError) as e:
        locate.ec_batch(code, d)
    assert e.value.code == ecg.ECG_EINVAL and f"r = {code.m}".encode() in ecg.lib().ecg_last_error()
    with pytest.raises(ecg.EcgError) as e:
        locate.ec(code, [d[0, j] for j in range(code.k)], [d[0, code.k + j] for j in range(code.m)], 64)
    assert e.value.code == ecg.ECG_EINVAL
    assert locate.counters()["launches"] == l0


# ---- wide checks: n + 2 counters in three registers per lane (counter 64 j + i in lane i of register j), pivot rows
# eight per word, r x n ratio tables, 128 pointers in the kernel arguments.  Plans: check_geometry_cases.wide_plan,
# checked against the definition by tests/test_check_geometry_cases.py.

def _wide_reference(n, r):
    """(C, stripes [3][n][B_MAIN], votes [3][n + 2] by the definition) of a wide case, worked out once."""
    def make():
        Cm, stripes = G.wide_stripes(gf_plain.apply, n, r)
        H = np.concatenate([Cm, np.eye(r, dtype=np.int64)], axis=1)
        return Cm, stripes, np.stack([LP.votes(H, stripes[s]) for s in range(3)])
    return G.memo(("wide", n, r), make)


def _wide_strided(torch, locate, n, r, shift=0):
    """H = [C | I] over n blocks, then the same check with its columns reversed (a general H: all n columns through
    the tables, pivots and ratios in the opposite words)."""
    Cm, stripes, votes = _wide_reference(n, r)
    B = B_MAIN
    img = _arena(np.concatenate([np.full((S3, 1, B), 0x77, np.uint8), stripes], axis=1))   # slot 0 is not named
    d = _to_dev(torch, img, shift)
    view = d[:, :, GUARD:GUARD + B]
    H = np.concatenate([Cm, np.eye(r, dtype=np.int64)], axis=1)
    src = list(range(1, n + 1))
    g = _check_call(torch, locate, img, d, B, shift, H, src, lambda: locate.matrix_batch(H, src, view),
                    memo={s: votes[s] for s in range(S3)})
    assert not g[0].any() and g[1, n] > 0 and g[2, n] > g[1, n]
    Hr, srcr = H[:, ::-1].copy(), src[::-1]
    _check_call(torch, locate, img, d, B, shift, Hr, srcr, lambda: locate.matrix_batch(Hr, srcr, view),
                memo={s: np.concatenate([votes[s][n - 1::-1], votes[s][n:]]) for s in range(S3)})


@gpu
@pytest.mark.parametrize("n,r", G.WIDE_CASES, ids=[f"n{n}-r{r}" for n, r in G.WIDE_CASES])
def test_wide_checks_strided(torch_cuda, locate, n, r):
    _wide_strided(torch_cuda, locate, n, r)


@gpu
def test_wide_check_through_the_byte_kernel(torch_cuda, locate):
    """n = 128, r = 8 with the arena shifted by one byte: tally<8, 1> credits all three registers."""
    _wide_strided(torch_cuda, locate, 128, 8, shift=1)


@gpu
@pytest.mark.parametrize("k,m", G.WIDE_INLINE, ids=[f"RS({k},{m})" for k, m in G.WIDE_INLINE])
def test_wide_checks_inline(ecg, torch_cuda, locate, k, m):
    """ecg_locate.ec over k + m = 128 (and 64) block pointers in the kernel arguments, the handle's own check."""
    torch = torch_cuda
    code = ecg.ec_factory(ecg.ECTYPE.RS, ecg.CodingParameters(k=k, m=m))
    n, B = k + m, B_MAIN
    H = np.asarray(code.check_matrix(), dtype=np.int64)
    assert H.shape == (m, n) and np.array_equal(H[:, k:], np.eye(m, dtype=np.int64))
    stripes = G.consistent(gf_plain.apply, H[:, :k], S3, B, 300 + n)
    G.apply_plan(stripes, G.wide_plan(n, m, seed=1))
    for s in range(S3):
        img = _arena(np.concatenate([np.full((1, 1, B), 0x77, np.uint8), stripes[s:s + 1]], axis=1))
        d = _to_dev(torch, img)
        blocks = [d[0, 1 + b, GUARD:GUARD + B] for b in range(n)]
        g = _check_call(torch, locate, img, d, B, 0, H, list(range(1, n + 1)),
                        lambda: locate.ec(code, blocks[:k], blocks[k:], B))
        if s:
            assert (g[0, :n] > 0).all() and g[0, n] >= sum(G.block_count(b) for b in range(n))
        else:
            assert not g.any()


@gpu
def test_n_129_is_refused(ecg, torch_cuda, locate):
    """RS(121, 8) has n = 129 > 128: ECG_EINVAL from both forms, nothing launched."""
    torch = torch_cuda
    k, m = G.WIDE_REFUSED
    code = ecg.ec_factory(ecg.ECTYPE.RS, ecg.CodingParameters(k=k, m=m))
    d = torch.zeros((2, k + m, 64), dtype=torch.uint8, device="cuda")
    l0 = locate.counters()["launches"]
    with pytest.raises(ecg.EcgError) as e:
        locate.ec(code, [d[0, j] for j in range(k)], [d[0, k + j] for j in range(m)], 64)
    assert e.value.code == ecg.ECG_EINVAL and b"n = 129" in ecg.lib().ecg_last_error()
    with pytest.raises(ecg.EcgError) as e:
        locate.ec_batch(code, d)
    assert e.value.code == ecg.ECG_EINVAL
    assert locate.counters()["launches"] == l0


# ---- an all-zero matrix row: encode_check leaves its H row and its parity column zero

@gpu
def test_all_zero_matrix_row(torch_cuda, locate):
    """encode_batch with row 1 of the RS(6,4) matrix zeroed: parity block k + 1 is checked by no row, so it is no
    candidate and damage in it is invisible; everything else is located as by the definition over that H."""
    torch = torch_cuda
    k, m, B = 6, 4, B_MAIN
    n = k + m
    M = np.asarray(RS64["matrix"], dtype=np.int64).reshape(m, k).copy()
    M[1] = 0
    stripes = _consistent(M, S3, B, 68)
    assert not stripes[:, k + 1].any()
    H = np.concatenate([M, np.eye(m, dtype=np.int64)], axis=1)
    H[1, k + 1] = 0
    for i, p in enumerate(POSITIONS):
        stripes[1, k + 1, p] ^= 0x10 + i                            # stripe 1: the unchecked block only
        stripes[2, (0, n // 2, n - 1)[i % 3], p] ^= 0x21 + i        # stripe 2: a data block, two checked parities
    stripes[2, k + 1, 100:140] ^= 0x5A                              # and the unchecked one
    img = _arena(stripes)
    d = _to_dev(torch, img)
    view = d[:, :, GUARD:GUARD + B]
    flat = [int(v) for v in M.reshape(-1)]
    g = _check_call(torch, locate, img, d, B, 0, H, list(range(n)), lambda: locate.encode_batch(k, m, flat, view))
    assert not g[0].any() and not g[1].any()
    assert g[2, n] == len(POSITIONS) and g[2, n + 1] == 0 and not g[:, k + 1].any()
    assert [int(v) for v in g[2, [0, n // 2, n - 1]]] == [3, 2, 2]


# ---- scrub -> dirty -> locate -> verdict -> decode -> re-scrub

@gpu
def test_end_to_end_repair(ecg, torch_cuda, scrub, locate):
    torch = torch_cuda
    c = next(g for g in GOLDEN if g["name"] == "RS(10,4)")
    k, m, S, B = 10, 4, 8, B_MAIN
    n = k + m
    M = [int(v) for v in c["matrix"]]
    original = _consistent(np.asarray(M, dtype=np.int64).reshape(m, k), S, B, 104)
    damaged = original.copy()
    rng = np.random.default_rng(11)
    damaged[2, 3, 100:2300] = rng.integers(0, 256, 2200, dtype=np.uint8)      # a data block, across a chunk edge
    damaged[5, 7, [0, 2048, B - 1]] ^= np.array([1, 0x80, 0xFF], np.uint8)    # a data block, single bytes
    damaged[6, 12, B - 40:] ^= 0x3C                                           # a parity block, into the tail
    d = torch.from_numpy(damaged).cuda()
    counts = scrub.encode_batch(k, m, M, d)
    sel = locate.dirty(counts)
    assert sel.dtype == torch.int32 and sel.is_cuda and sel.cpu().tolist() == [2, 5, 6]
    votes = locate.encode_batch(k, m, M, d, stripe_ids=sel).cpu().numpy()
    named = []
    for row in votes:
        block, ids = locate.verdict(row)
        assert block >= 0 and ids == [block]
        named.append(block)
    assert named == [3, 7, 12]
    for s, block in zip(sel.cpu().tolist(), named):
        ecg.decode_batch(k, m, M, int(all(v == 1 for v in M[:k])), [[block]], d[s:s + 1])  # in place
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), original)
    again = scrub.encode_batch(k, m, M, d)
    assert not again.cpu().numpy().any()
    assert locate.dirty(again).numel() == 0
