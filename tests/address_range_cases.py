"""Layouts, damage plans and expected-result builders for the address-range tests of the check and checksum libraries
(helper of tests/test_address_range_cases.py and tests/test_gpu_address_range.py; numpy only, imports nothing of the
project: the plain references are handed in).

Every kernel of libecg_scrub, libecg_locate, libecg_heal, libecg_heal2 and libecg_sum forms an address as
base + stripe * sstride + block_id * bstride + offset.  The three parts put each term of that sum, and the report row
index beside it, where a 32-bit product, a 31-bit column count or a 16-bit row index gives another number:

  A  a sparse arena: two stripes of six 4693-byte blocks whose strides put the block offsets past 2^31, 2^32 and 2^33;
  B  one stripe of six blocks of 2^31 - 1 bytes: offsets inside a block up to the limit, counters up to 2^31 - 1;
  C  65 600 selected stripes of 53 bytes: report rows past 2^16.

One code serves all three: H = [C | I] with C a 4 x 2 Cauchy matrix (k = 2, r = 4, n = 6), through the library's
`encode_batch` (the stored blocks 2..5 are addressed as ident_base + q) and, with its six columns in the order PERM,
through `matrix_batch` (all six through the tables).
"""
import numpy as np

K, R, N = 2, 4, 6
PERM = (3, 0, 5, 1, 4, 2)               # matrix_batch's column order: its last four columns are no identity
GUARD, BAND = 64, 0xC3
K_THREADS = 128                          # gf_kernels.hpp kThreads
CHUNK = 16 * K_THREADS                   # 2 KiB of every block per workgroup at the default geometry


def check_matrix(Cm):
    """H = [Cm | I], r x (k + r)."""
    Cm = np.asarray(Cm, dtype=np.int64)
    assert Cm.shape == (R, K)
    return np.concatenate([Cm, np.eye(R, dtype=np.int64)], axis=1)


def permuted(H):
    """(H with its columns in the order PERM, the src_ids that go with it)."""
    return np.asarray(H)[:, list(PERM)].copy(), list(PERM)


def in_column_order(rows, cols, extra):
    """Per-block counters [..., n + extra] of the stripes' own block order -> the order a call with src_ids = cols
    reports them in: column j is block cols[j]; the `extra` totals stay behind them."""
    rows = np.asarray(rows)
    return np.concatenate([rows[..., list(cols)], rows[..., N:N + extra]], axis=-1)


# ---------------------------------------------------------------------------------------------------------------------
# Part A: a sparse arena

B_A = 4693                                               # 293 columns: chunks of 128, 128 and 37, and a 5-byte tail
VEC_A = B_A & ~15
CHUNKS_A = tuple((lo, min(lo + CHUNK, VEC_A)) for lo in range(0, VEC_A, CHUNK))
S_A = 2
BS_A = (1 << 31) + 4096                                  # block stride
SS_A = N * BS_A + 8192                                   # stripe stride
BASE_A = 64                                              # storage offset of the aligned view
ARENA_A = S_A * SS_A + 256                               # bytes of the 1-D arena, about 24.1 GiB
SHIFTS_A = (0, 1)                                        # the view as it is, and moved up by one byte (unaligned)
FIRST_A = {0: 1, 1: 4}                                   # a stripe's damaged block: a table column, a stored parity
SECOND_A = {0: 5, 1: 0}                                  # heal2: the stripe's second damaged block


def offset_a(s, b, shift=0):
    """Arena offset of byte 0 of block b of stripe s."""
    return BASE_A + shift + s * SS_A + b * BS_A


def windows_a(shift=0):
    """[(s, b, lo, hi)]: the twelve arena ranges that hold a block inside its two guard bands."""
    return [(s, b, offset_a(s, b, shift) - GUARD, offset_a(s, b, shift) + B_A + GUARD)
            for s in range(S_A) for b in range(N)]


def chunk_count_a(s, w):
    """Damaged positions of chunk w of stripe s's first damaged block: no two chunks and no two stripes alike."""
    return 3 + s + 5 * w


def plan_a(pair, seed=4693):
    """[(stripe, block, positions, values)].  Per stripe, block FIRST_A[s]: chunk_count_a(s, w) positions in every
    2 KiB chunk w, one of them in the chunk's first and one in its last 16-byte column, and one tail byte.  pair
    (heal2): block SECOND_A[s] is damaged too -- at every other position of the first block (pairs), stripe 1's tail
    byte among them, and at two positions of its own per chunk (single-block damage in a second block)."""
    rng = np.random.default_rng(seed)
    plan = []
    for s in range(S_A):
        pos = []
        for w, (lo, hi) in enumerate(CHUNKS_A):
            first = lo + int(rng.integers(0, 16))
            last = hi - 16 + int(rng.integers(0, 16))
            inner = lo + 16 + rng.choice(hi - lo - 32, chunk_count_a(s, w) - 2, replace=False)
            pos += [first, last] + [int(p) for p in inner]
        tail = VEC_A + 1 + s
        pos = np.array(sorted(pos) + [tail], dtype=np.int64)
        assert len(set(pos.tolist())) == pos.size
        plan.append((s, FIRST_A[s], pos, rng.integers(1, 256, pos.size, dtype=np.uint8)))
        if pair:
            shared = pos[1::2]                                       # stripe 1 has an even count: its tail byte is one
            own = []
            for lo, hi in CHUNKS_A:
                free = np.setdiff1d(np.arange(lo, hi), pos)
                own += [int(p) for p in rng.choice(free, 2, replace=False)]
            both = np.array(sorted(shared.tolist() + own), dtype=np.int64)
            plan.append((s, SECOND_A[s], both, rng.integers(1, 256, both.size, dtype=np.uint8)))
    return plan


def apply_plan(stripes, plan):
    """XOR a plan's values into [S][n][B] stripes, in place."""
    for s, b, pos, val in plan:
        stripes[s, b, pos] ^= val


def stripes_a(apply, Cm, pair):
    """(clean, damaged): [S_A][n][B_A] stripes consistent with H = [Cm | I] -- random data and `apply`
    (tests/gf_plain.py apply, handed in) of Cm as the parity, never the library's own encode -- and the same damaged by
    plan_a."""
    rng = np.random.default_rng(77)
    clean = np.zeros((S_A, N, B_A), np.uint8)
    for s in range(S_A):
        clean[s, :K] = rng.integers(0, 256, (K, B_A), dtype=np.uint8)
        clean[s, K:] = apply(Cm, clean[s, :K])
    damaged = clean.copy()
    apply_plan(damaged, plan_a(pair))
    return clean, damaged


def image_a(stripes):
    """[12][GUARD + B_A + GUARD] window images, in windows_a's order: the block inside its bands."""
    img = np.full((S_A * N, GUARD + B_A + GUARD), BAND, np.uint8)
    img[:, GUARD:GUARD + B_A] = stripes.reshape(S_A * N, B_A)
    return img


# ---------------------------------------------------------------------------------------------------------------------
# Part B: blocks of 2^31 - 1 bytes

B_B = (1 << 31) - 1
PITCH_B = 1 << 31
VEC_B = B_B & ~15                                        # 2^31 - 16: the vector path; the byte path takes 15 bytes
RANGES_B = ((0, 5 * CHUNK + 37), ((1 << 30) - 1000, (1 << 30) + 3000), (B_B - 4099, B_B))
RANGES_B_BYTES = sum(hi - lo for lo, hi in RANGES_B)
FILLS_B = {1: 0x5A, 4: 0xC3}                             # the constant a damaged block is filled with
COLS_PER_WG_B = 1 << 20                                  # the second geometry: column loops of 8192 iterations
REPLICA = 21                                             # one 16-byte column and a 5-byte tail


def replica_b(blocks):
    """[n][REPLICA] stripe: all zero (consistent with every linear check), the named blocks at their constant."""
    st = np.zeros((N, REPLICA), np.uint8)
    for b in blocks:
        st[b] = FILLS_B[b]
    return st


def scaled_b(counters, nbytes):
    """The replica rule: the damage is the same at every byte position, so every counter of the replica is 0 or
    REPLICA, and the counter of `nbytes` damaged positions is 0 or nbytes."""
    counters = np.asarray(counters, dtype=np.int64)
    assert np.isin(counters, (0, REPLICA)).all(), counters
    return counters // REPLICA * nbytes


# ---------------------------------------------------------------------------------------------------------------------
# Part C: many small stripes

S_C = 65600                                              # selected stripes: 32 * 2050
EXTRA_C = 8                                              # the backing tensor holds S_C + 8
B_C, PITCH_C = 53, 64                                    # three columns and a 5-byte tail
FIXED_C = (0, 1, 7, 8, 255, 256, 32767, 32768, 65535, 65536, 65599)
UNSELECTED_C = S_C + 3                                   # damaged, never selected
MAP_C = (2, 4)                                           # the second run's ECG_OPT_GRID_MAP, ECG_OPT_MAP_GROUP
# selection position -> stripe: damaged stripes at the first row, either side of row 2^16 and at the last row
PINS_C = {0: 65599, 65535: 65536, 65536: 7, S_C - 1: 32768}


def damaged_ids_c():
    """The damaged stripes, in the order that sets their amount of damage: the fixed ids, a seeded handful more, and
    last the one outside the selection."""
    rng = np.random.default_rng(53)
    rest = np.setdiff1d(np.arange(S_C), np.array(FIXED_C))
    more = sorted(int(v) for v in rng.choice(rest, 28, replace=False))
    return list(FIXED_C) + more + [UNSELECTED_C]


def plan_c():
    """[(stripe id, block, positions, values)]: stripe i of damaged_ids_c gets 1 + i damaged bytes in block id % n."""
    rng = np.random.default_rng(5353)
    plan = []
    for i, sid in enumerate(damaged_ids_c()):
        pos = np.sort(rng.choice(B_C, 1 + i, replace=False))
        plan.append((sid, sid % N, pos, rng.integers(1, 256, pos.size, dtype=np.uint8)))
    return plan


def stripes_c():
    """{stripe id: [n][B_C] damaged stripe}; every other stripe is all zero."""
    out = {}
    for sid, b, pos, val in plan_c():
        st = np.zeros((N, B_C), np.uint8)
        st[b, pos] ^= val
        out[sid] = st
    return out


def image_c():
    """The host image of the backing tensor, [S_C + EXTRA_C][n][PITCH_C]: zero but for the damage."""
    img = np.zeros((S_C + EXTRA_C, N, PITCH_C), np.uint8)
    for sid, st in stripes_c().items():
        img[sid, :, :B_C] = st
    return img


def selection_c():
    """A seeded permutation of 0..S_C - 1 (distinct: safe for the two heals) with PINS_C swapped into place."""
    sel = np.random.default_rng(65600).permutation(S_C).astype(np.int64)
    for p, sid in PINS_C.items():
        q = int(np.flatnonzero(sel == sid)[0])
        sel[p], sel[q] = sel[q], sel[p]
    return sel


def rows_c(sel, per_stripe, width):
    """[len(sel)][width] expected result of a call over the selection: per_stripe[id] for the damaged stripes, zero
    rows for all others."""
    want = np.zeros((len(sel), width), np.int64)
    where = {int(s): p for p, s in enumerate(sel)}
    for sid, row in per_stripe.items():
        if sid in where:
            want[where[sid]] = row
    return want


# ---- references worked out once per process and shared between the tests that need them: {key: value}
_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]
