"""Launch geometries and damage plans for the scrub and locate kernels (helper of tests/test_check_geometry_cases.py,
tests/test_gpu_check_geometry.py and the wide-check tests of tests/test_gpu_scrub.py / tests/test_gpu_locate.py;
numpy only, imports nothing of the project).

Geometry.  `expected_geometry` mirrors the host rule of launch_scrub / launch_locate / launch_heal
(csrc/launch_rule.hpp plan_vector_path, the one copy all three call), which turns the options ECG_OPT_GRID_MAP,
ECG_OPT_MAP_GROUP and ECG_OPT_COLS_PER_WG into the launch descriptor's grid_map, map_group, cols_per_wg and
wg_per_stripe.  GEOMETRY_CASES lists launches that between them take every branch of wg_coords
(gf_device.hpp) and the column loops for one, two and three iterations; `last_launch()` of either library must
report what the table says.

Damage.  A workgroup -> chunk map that is no bijection skips one 2 KiB chunk and visits another twice, and a counter
that does not survive the column loop loses one iteration's worth.  A test sees either only if every chunk holds
damage and no two chunks of a stripe, and no two stripes, hold the same amount: `geometry_plan`.  `wide_plan` is the
plan of the wide locate checks (n up to 128): damage in every block, once inside a single wave and once spread out.
"""
from collections import namedtuple

import numpy as np

# ---- the kernels' constants, mirrored (source: erasure-codes-prototype_amd/csrc/)
K_THREADS = 128                  # gf_kernels.hpp kThreads (ECG_TPB): threads, and default 16-byte columns, per workgroup
B_MAIN = 4693                    # 293 columns: chunks of 128, 128 and 37 columns by default, and a 5-byte tail
VEC_BYTES = B_MAIN & ~15         # 4688: what the vector kernels cover
CHUNK = 16 * K_THREADS           # 2 KiB of every block per workgroup at the default
CHUNKS = tuple((lo, min(lo + CHUNK, VEC_BYTES)) for lo in range(0, VEC_BYTES, CHUNK))
WAVE_BYTES = 16 * 64             # one wave's 64 columns


def expected_geometry(S, B, grid_map, map_group, cols_per_wg):
    """{grid_map, map_group, cols_per_wg, wg_per_stripe, S} of the vector-path launch over S stripes of B bytes with
    the three options set as given (csrc/launch_rule.hpp plan_vector_path, which launch_scrub, launch_locate and
    launch_heal call when vec_bytes > 0)."""
    ncols = (B & ~15) >> 4                                   # const long long ncols = vec_bytes >> 4;
    cpw = cols_per_wg                                        # long long cpw = get_option(ECG_OPT_COLS_PER_WG);
    if cpw <= 0:                                             # if (cpw <= 0) cpw = kThreads;
        cpw = K_THREADS
    if ncols < cpw:                                          # if (ncols < cpw) cpw = ceil(ncols / kThreads) * kThreads;
        cpw = ((ncols + K_THREADS - 1) // K_THREADS) * K_THREADS
    wps = (ncols + cpw - 1) // cpw                           # a.wg_per_stripe = (ncols + cpw - 1) / cpw;
    gx = S * wps                                             # const long long gx = a.S * a.wg_per_stripe;
    gm = grid_map                                            # long long gm = get_option(ECG_OPT_GRID_MAP);
    if gm == 3:                                              # if (gm == 3) gm = 1;
        gm = 1
    G = map_group                                            # long long G = get_option(ECG_OPT_MAP_GROUP);
    while G > 1 and S % (8 * G) != 0:                        # while (G > 1 && a.S % (8 * G) != 0) G >>= 1;
        G >>= 1
    if gm == 2 and S % (8 * G) != 0:                         # if (gm == 2 && a.S % (8 * G) != 0) gm = 1;
        gm = 1
    gm = 1 if (gm == 1 and gx % 8 == 0) else 2 if gm == 2 else 0   # a.grid_map = ...
    return {"grid_map": gm, "map_group": G, "cols_per_wg": cpw, "wg_per_stripe": wps, "S": S}


# S: the stripes of the launch (the locate's S_sel).  grid_map / map_group / cols_per_wg: the options.  launch: the
# (grid_map, map_group, wg_per_stripe) the call must launch with.  mid_clean: stripe 1 leaves its middle 2 KiB clean.
Geometry = namedtuple("Geometry", "S grid_map map_group cols_per_wg launch mid_clean")

GEOMETRY_CASES = (
    Geometry(3, 3, 1, 0, (0, 1, 3), False),       # gx = 9: no multiple of 8, the linear map
    Geometry(8, 3, 1, 0, (1, 1, 3), False),       # the auto rule: XCD-contiguous
    Geometry(8, 0, 1, 0, (0, 1, 3), False),       # linear on request
    Geometry(8, 2, 1, 0, (2, 1, 3), False),       # stripe s on XCD group s % 8
    Geometry(16, 2, 2, 0, (2, 2, 3), False),      # runs of two stripes
    Geometry(16, 2, 4, 0, (2, 2, 3), False),      # G = 4 does not tile 16 stripes over 8 groups: reduced to 2
    Geometry(32, 2, 4, 0, (2, 4, 3), False),      # runs of four
    Geometry(24, 2, 64, 0, (2, 1, 3), False),     # G reduced all the way to 1
    Geometry(12, 2, 1, 0, (0, 1, 3), False),      # 12 % 8 != 0: map 2 -> 1, gx = 36: -> 0
    Geometry(12, 3, 1, 256, (1, 1, 2), False),    # gx = 24; a stripe's first workgroup runs its column loop twice
    Geometry(8, 3, 1, 1024, (1, 1, 1), True),     # cols_per_wg clamps to 384: three iterations, the last partial
    Geometry(8, 2, 1, 1024, (2, 1, 1), True),
)
EXTRA_STRIPES = 8   # the locate's backing tensor holds S + 8 stripes, of which the selection names S


def geometry_id(g):
    return f"S{g.S}-map{g.grid_map}-G{g.map_group}-cpw{g.cols_per_wg}"


def selection(g):
    """The locate's stripe selection of a geometry case: S ids out of S + EXTRA_STRIPES, scrambled, stripe 1 among
    them, one id twice."""
    rng = np.random.default_rng(100 * g.S + g.cols_per_wg + g.grid_map)
    ids = [int(v) for v in rng.permutation(g.S + EXTRA_STRIPES)]
    ids.remove(1)
    sel = ids[:g.S - 2]
    sel.insert(len(sel) // 2, 1)
    sel.append(sel[0])                                        # the duplicate
    assert len(sel) == g.S and len(set(sel)) == g.S - 1
    return sel


def chunk_count(s, w):
    """Damaged positions of chunk w of stripe s: differs between the chunks of a stripe and between stripes."""
    return 2 + s + 32 * w


def geometry_plan(S, n, mid_clean, seed=2024):
    """[(stripe, block, positions, values)]: per stripe s, damage in block s % n only (so the locate has a candidate
    that explains it): chunk_count(s, w) positions in every 2 KiB chunk w, among them one in the chunk's first and one
    in its last 16-byte column; odd stripes also one tail byte.  mid_clean: stripe 1 has no damage in its middle
    chunk (with one workgroup per stripe: a loop iteration that finds nothing between two that do)."""
    rng = np.random.default_rng(seed + 1000 * S + n + int(mid_clean))
    plan = []
    for s in range(S):
        pos = []
        for w, (lo, hi) in enumerate(CHUNKS):
            if mid_clean and s == 1 and w == 1:
                continue
            first = lo + int(rng.integers(0, 16))
            last = hi - 16 + int(rng.integers(0, 16))
            inner = lo + 16 + rng.choice(hi - lo - 32, chunk_count(s, w) - 2, replace=False)
            pos += [first, last] + [int(p) for p in inner]
        if s % 2:
            pos.append(VEC_BYTES + s % (B_MAIN - VEC_BYTES))
        pos = np.array(sorted(pos), dtype=np.int64)
        assert len(set(pos.tolist())) == pos.size
        plan.append((s, s % n, pos, rng.integers(1, 256, pos.size, dtype=np.uint8)))
    return plan


def apply_plan(stripes, plan):
    """XOR a plan's values into [S][n][B] stripes, in place."""
    for s, b, pos, val in plan:
        stripes[s, b, pos] ^= val


def consistent(apply, Cm, S, B, seed):
    """[S][k + r][B] stripes that satisfy H = [Cm | I]: random data, and `apply` (tests/gf_plain.py apply, handed in:
    this module imports nothing) of Cm as the parity.  Never the library's own encode."""
    Cm = np.asarray(Cm, dtype=np.int64)
    r, k = Cm.shape
    rng = np.random.default_rng(seed)
    out = np.zeros((S, k + r, B), np.uint8)
    for s in range(S):
        out[s, :k] = rng.integers(0, 256, (k, B), dtype=np.uint8)
        out[s, k:] = apply(Cm, out[s, :k])
    return out


def geometry_stripes(apply, Cm, g):
    """[S + EXTRA_STRIPES][n][B_MAIN] stripes of a geometry case: consistent with H = [Cm | I], then damaged by
    geometry_plan.  The scrub checks the first S of them, the locate the S that `selection` names."""
    total = g.S + EXTRA_STRIPES
    stripes = consistent(apply, Cm, total, B_MAIN, 9000 + total)
    apply_plan(stripes, geometry_plan(total, sum(np.asarray(Cm).shape), g.mid_clean))
    return stripes


# ---- wide locate checks: n + 2 counters in three registers per lane, pivot rows eight per word
WIDE_N = (62, 63, 64, 65, 126, 127, 128)          # r = 8: n + 1 either side of 64 and of 128
WIDE_R = (1, 2, 5)                                # at n = 64 and n = 128
WIDE_CASES = tuple((n, 8) for n in WIDE_N) + tuple((n, r) for n in (64, 128) for r in WIDE_R)
WIDE_INLINE = ((120, 8), (56, 8))                 # RS(k, m) with k + m = 128 and 64: the per-stripe form
WIDE_REFUSED = (121, 8)                           # n = 129
WIDE_EDGES = (0, 15, 16, 1023, 1024, 2047, 2048, 4095, 4096, VEC_BYTES - 1, VEC_BYTES, B_MAIN - 1)
WIDE_DOUBLES = 4                                  # positions where blocks 0 and n - 1 are both damaged
ONE_WAVE = (WAVE_BYTES, 2 * WAVE_BYTES)           # the second wave of the first chunk


def block_count(b):
    return 1 + b % 5


def wide_matrix(n, r):
    """C (r x (n - r)) of the wide case's check H = [C | I]: seeded random nonzero bytes; from r = 2 on a zero on top
    of column 1 (its pivot row is 1) and column n - r - 2 zero down to its last row (pivot row r - 1, kept in a high
    word of the packed pivots); a 1 in the last place."""
    k = n - r
    M = np.random.default_rng(31 * n + r).integers(1, 256, (r, k), dtype=np.int64)
    if r >= 2:
        M[0, 1] = 0
        M[:r - 1, k - 2] = 0
    M[r - 1, k - 1] = 1
    return M


def wide_stripes(apply, n, r):
    """(C, [3][n][B_MAIN] stripes): consistent with H = [C | I], then damaged by wide_plan."""
    Cm = wide_matrix(n, r)
    stripes = consistent(apply, Cm, 3, B_MAIN, 5000 + 10 * n + r)
    apply_plan(stripes, wide_plan(n, r))
    return Cm, stripes


def wide_plan(n, r, seed=0):
    """Plans of stripes 1 and 2 of a wide case (stripe 0 stays clean), as apply_plan takes them.
    Stripe 1, "one wave": block b damaged at block_count(b) positions, no position twice, all in ONE_WAVE: one
    candidate test credits counters in every register.  Stripe 2, "spread": as many positions per block, drawn from
    the chunk, column and tail edges and from all over the block, plus WIDE_DOUBLES positions where blocks 0 and n - 1
    are both damaged (which no single block explains when three columns of H are independent)."""
    rng = np.random.default_rng(7919 * n + 104729 * r + seed)
    total = sum(block_count(b) for b in range(n))
    owner = np.concatenate([np.full(block_count(b), b) for b in range(n)])
    plan = []
    lo, hi = ONE_WAVE
    assert total <= hi - lo
    pos = lo + rng.choice(hi - lo, total, replace=False)
    for b in range(n):
        p = np.sort(pos[owner == b])
        plan.append((1, b, p, rng.integers(1, 256, p.size, dtype=np.uint8)))
    rest = np.setdiff1d(np.arange(B_MAIN), np.array(WIDE_EDGES))
    pos = np.concatenate([np.array(WIDE_EDGES), rng.choice(rest, total + WIDE_DOUBLES - len(WIDE_EDGES),
                                                            replace=False)])
    pos, both = pos[:total], pos[total:]
    pos = rng.permutation(pos)                                # the edges go to whichever block
    for b in range(n):
        p = np.sort(pos[owner == b])
        plan.append((2, b, p, rng.integers(1, 256, p.size, dtype=np.uint8)))
    for b in (0, n - 1):
        plan.append((2, b, np.sort(both), rng.integers(1, 256, both.size, dtype=np.uint8)))
    return plan


# ---- references worked out once per process and shared between the tests that need them: {key: value}
_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]
