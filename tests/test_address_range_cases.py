"""The cases of tests/address_range_cases.py, checked against the plain references alone (no GPU, no library): the one
code is accepted by every library's rule, part A's blocks lie where a 32-bit product goes wrong and overlap nothing,
part B's replica rule holds for every reference, and part C's selection and damage tell every stripe apart -- so that
an address, a column count or a report row formed in too few bits changes a number the GPU tests compare."""
import numpy as np

import address_range_cases as AR
import check_geometry_cases as G
import crc32c_plain as CP
import gf_plain
import heal2_plain as P2
import heal_plain as HP
import locate_plain as LP

CM = P2.cauchy(AR.R, AR.K)
H = AR.check_matrix(CM)


def test_the_code_is_accepted_by_every_library():
    assert H.shape == (4, 6) and (CM != 0).all()           # a damaged data block shows in all four check rows
    assert P2.accepts(H, True) and P2.accepts(H, False)     # heal2 ANY2 and TARGET2
    assert LP.proportional_pairs(H) == (0, 0)               # heal ANY
    Hp, src = AR.permuted(H)
    assert sorted(src) == list(range(6)) and not np.array_equal(Hp[:, 2:], np.eye(4, dtype=np.int64))
    assert np.array_equal(Hp[:, [src.index(b) for b in range(6)]], H)
    rows = np.arange(16).reshape(2, 8)
    assert AR.in_column_order(rows, src, 2).tolist() == [[3, 0, 5, 1, 4, 2, 6, 7], [11, 8, 13, 9, 12, 10, 14, 15]]


# ---- part A

def test_sparse_offsets_cross_every_power_and_overlap_nothing():
    assert AR.BS_A == 2 ** 31 + 4096 and AR.SS_A == 6 * AR.BS_A + 8192 and AR.ARENA_A == 2 * AR.SS_A + 256
    assert 24.0 < AR.ARENA_A / 2 ** 30 < 24.2
    assert AR.BS_A % 16 == 0 and AR.SS_A % 16 == 0 and AR.BASE_A % 16 == 0
    off = AR.offset_a
    # through block_id * bstride alone (stripe 0): blocks 1, 2 and 4; the ident blocks 2..5 all lie past 2^32
    assert off(0, 0) < 2 ** 31 < off(0, 1) < 2 ** 32 < off(0, 2) and off(0, 3) < 2 ** 33 < off(0, 4)
    # through stripe * sstride (stripe 1), before any block stride is added
    assert 1 * AR.SS_A > 2 ** 33
    # what a product masked to 32 bits would address instead lies elsewhere, and inside the arena (block 1 of stripe 0
    # fits 32 bits unsigned: it goes wrong only under a sign extension)
    for s in range(AR.S_A):
        for b in range(0 if s else 2, AR.N):
            masked = AR.BASE_A + ((s * AR.SS_A) & 0xFFFFFFFF) + ((b * AR.BS_A) & 0xFFFFFFFF)
            assert masked != off(s, b) and masked + AR.B_A < AR.ARENA_A
    for shift in AR.SHIFTS_A:
        w = sorted((lo, hi) for _, _, lo, hi in AR.windows_a(shift))
        assert len(w) == 12 and w[0][0] >= 0 and w[-1][1] <= AR.ARENA_A
        assert all(a[1] <= b[0] for a, b in zip(w, w[1:]))                  # blocks and guard bands are disjoint
        assert all(hi - lo == AR.B_A + 2 * AR.GUARD for lo, hi in w)
        assert all((lo + AR.GUARD) % 16 == shift for lo, hi in w)           # the shifted view is unaligned everywhere


def test_sparse_plans_damage_every_chunk_differently():
    assert AR.B_A == G.B_MAIN and AR.CHUNKS_A == G.CHUNKS
    for pair in (False, True):
        clean, damaged = AR.stripes_a(gf_plain.apply, CM, pair)
        totals = set()
        for s in range(AR.S_A):
            assert not gf_plain.apply(H, clean[s]).any()
            hit = sorted(int(b) for b in np.flatnonzero((clean[s] != damaged[s]).any(axis=1)))
            assert hit == sorted([AR.FIRST_A[s]] + ([AR.SECOND_A[s]] if pair else []))
            diff = clean[s, AR.FIRST_A[s]] != damaged[s, AR.FIRST_A[s]]
            per = [int(np.count_nonzero(diff[lo:hi])) for lo, hi in AR.CHUNKS_A]
            assert per == [AR.chunk_count_a(s, w) for w in range(3)] and len(set(per)) == 3
            for lo, hi in AR.CHUNKS_A:
                assert diff[lo:lo + 16].any() and diff[hi - 16:hi].any()    # the chunk's first and last column
            assert np.count_nonzero(diff[AR.VEC_A:]) == 1                   # one tail byte
            totals.add(tuple(per))
        assert len(totals) == AR.S_A
        if not pair:
            for s in range(AR.S_A):
                v = LP.votes(H, damaged[s])
                assert v[AR.FIRST_A[s]] == v[AR.N] > 0 and v[AR.N + 1] == 0
        else:
            healed, reports = P2.heal2_stripes(H, damaged)
            assert np.array_equal(healed, clean)
            for s in range(AR.S_A):
                assert reports[s, AR.N + 2] > 6 and reports[s, AR.N + 1] == 0
                assert reports[s, AR.FIRST_A[s]] > reports[s, AR.N + 2] < reports[s, AR.SECOND_A[s]]
            tails = [int(np.count_nonzero((clean[s] != damaged[s])[:, AR.VEC_A:].any(axis=1))) for s in range(AR.S_A)]
            assert tails == [1, 2]                                          # stripe 1's tail byte is a pair


# ---- part B

def test_replica_rule_holds_for_every_reference():
    assert AR.B_B == 2 ** 31 - 1 and AR.VEC_B == 2 ** 31 - 16 and AR.B_B - AR.VEC_B == 15
    assert AR.RANGES_B_BYTES == 5 * 2048 + 37 + 4000 + 4099
    assert all(0 <= lo < hi <= AR.B_B for lo, hi in AR.RANGES_B)
    assert AR.RANGES_B[1][0] < 2 ** 30 < AR.RANGES_B[1][1] and AR.RANGES_B[2][0] < AR.VEC_B
    assert len({hi - lo for lo, hi in AR.RANGES_B}) == 3
    one, two = AR.replica_b([1]), AR.replica_b([1, 4])
    counts = np.array([np.count_nonzero(row) for row in gf_plain.apply(H, one)])
    assert counts.tolist() == [21, 21, 21, 21]
    assert LP.votes(H, one).tolist() == [0, 21, 0, 0, 0, 0, 21, 0]
    healed, report = HP.heal(H, one)
    assert report.tolist() == [0, 21, 0, 0, 0, 0, 21, 0] and not healed.any()
    healed, report = P2.heal2(H, two)
    assert report.tolist() == [0, 21, 0, 0, 21, 0, 21, 0, 21] and not healed.any()
    assert AR.scaled_b(report, AR.B_B).tolist() == [0, AR.B_B, 0, 0, AR.B_B, 0, AR.B_B, 0, AR.B_B]
    assert AR.scaled_b(report, AR.B_B).max() < 2 ** 31                      # positive in the int32 report
    # the two geometries the read-only libraries run at
    e = G.expected_geometry(1, AR.B_B, 3, 1, 0)
    assert (e["grid_map"], e["cols_per_wg"], e["wg_per_stripe"]) == (1, 128, 2 ** 20)
    e = G.expected_geometry(1, AR.B_B, 3, 1, AR.COLS_PER_WG_B)
    assert (e["grid_map"], e["cols_per_wg"], e["wg_per_stripe"]) == (1, 2 ** 20, 128)
    assert AR.COLS_PER_WG_B // AR.K_THREADS == 8192


# ---- part C

def test_dense_selection_and_damage_tell_every_stripe_apart():
    assert AR.S_C == 32 * 2050 and AR.S_C % 32 == 0 and AR.S_C > 2 ** 16
    ids = AR.damaged_ids_c()
    assert len(ids) == len(set(ids)) == 40 and set(AR.FIXED_C) < set(ids)
    assert [i for i in ids if i >= AR.S_C] == [AR.UNSELECTED_C] and AR.UNSELECTED_C < AR.S_C + AR.EXTRA_C
    sel = AR.selection_c()
    assert sel.shape == (AR.S_C,) and np.array_equal(np.sort(sel), np.arange(AR.S_C))     # distinct, all of them
    assert not np.array_equal(sel, np.arange(AR.S_C))
    assert all(sel[p] == sid for p, sid in AR.PINS_C.items())
    assert {0, 2 ** 16 - 1, 2 ** 16, AR.S_C - 1} <= set(AR.PINS_C) and set(AR.PINS_C.values()) < set(ids)
    stripes = AR.stripes_c()
    assert sorted(stripes) == sorted(ids)
    for i, sid in enumerate(ids):
        assert np.count_nonzero(stripes[sid]) == np.count_nonzero(stripes[sid][sid % AR.N]) == 1 + i
    assert any(st[:, 48:].any() for st in stripes.values()) and any(st[:, :48].any() for st in stripes.values())
    for rows in (np.stack([[np.count_nonzero(r) for r in gf_plain.apply(H, stripes[s])] for s in ids]),
                 np.stack([LP.votes(H, stripes[s]) for s in ids]),
                 np.stack([HP.heal(H, stripes[s])[1] for s in ids]),
                 np.stack([P2.heal2(H, stripes[s])[1] for s in ids])):
        assert len({tuple(r) for r in rows.tolist()}) == len(ids) and rows.any(axis=1).all()
    assert all(not HP.heal(H, stripes[s])[0].any() and not P2.heal2(H, stripes[s])[0].any() for s in ids)
    img = AR.image_c()
    assert img.shape == (AR.S_C + 8, 6, 64) and not img[:, :, AR.B_C:].any()
    assert sorted(int(s) for s in np.flatnonzero(img.any(axis=(1, 2)))) == sorted(ids)
    want = AR.rows_c(sel, {s: LP.votes(H, stripes[s]) for s in ids}, AR.N + 2)
    assert np.count_nonzero(want.any(axis=1)) == 39 and want[[0, 65535, 65536, AR.S_C - 1]].any(axis=1).all()
    sums = CP.many(np.stack([stripes[s] for s in ids]))
    assert CP.bitwise(bytes(AR.B_C)) not in set(int(v) for s, row in zip(ids, sums) for v in [row[s % AR.N]])
    # the two geometries
    e = G.expected_geometry(AR.S_C, AR.B_C, 3, 1, 0)
    assert (e["grid_map"], e["map_group"], e["cols_per_wg"], e["wg_per_stripe"]) == (1, 1, 128, 1)
    e = G.expected_geometry(AR.S_C, AR.B_C, *AR.MAP_C, 0)
    assert (e["grid_map"], e["map_group"], e["wg_per_stripe"]) == (2, 4, 1)
