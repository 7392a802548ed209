"""The plans of tests/check_geometry_cases.py, checked against the references alone (no GPU, no library): the case
table agrees with the mirrored host rule and covers every branch, every 2 KiB chunk of every stripe holds its own
amount of damage, and the wide locate plans put a nonzero count in every counter -- so that a map that skips a chunk,
a counter lost between loop iterations or a counter credited to the wrong register changes a number the GPU tests
compare."""
import json
import os

import numpy as np
import pytest

import check_geometry_cases as G
import gf_plain
import locate_plain as LP

HERE = os.path.dirname(os.path.abspath(__file__))
RS64 = next(c for c in json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"] if c["name"] == "RS(6,4)")
M64 = np.asarray(RS64["matrix"], dtype=np.int64).reshape(4, 6)
H64 = np.concatenate([M64, np.eye(4, dtype=np.int64)], axis=1)


def test_table_agrees_with_the_mirrored_host_rule():
    assert G.B_MAIN == 4693 and G.CHUNKS == ((0, 2048), (2048, 4096), (4096, 4688))
    for g in G.GEOMETRY_CASES:
        e = G.expected_geometry(g.S, G.B_MAIN, g.grid_map, g.map_group, g.cols_per_wg)
        assert (e["grid_map"], e["map_group"], e["wg_per_stripe"]) == g.launch, g
        assert e["S"] == g.S and e["cols_per_wg"] * e["wg_per_stripe"] >= 293 and e["cols_per_wg"] % 128 == 0
        assert g.S + G.EXTRA_STRIPES <= 40
    launches = [g.launch for g in G.GEOMETRY_CASES]
    assert {l[0] for l in launches} == {0, 1, 2}
    assert {l[1] for l in launches if l[0] == 2} == {1, 2, 4}
    assert {l[2] for l in launches} == {1, 2, 3}
    # the twelve rows of the issue's table, in its order
    assert [(g.S, g.grid_map, g.map_group, g.cols_per_wg) for g in G.GEOMETRY_CASES] == [
        (3, 3, 1, 0), (8, 3, 1, 0), (8, 0, 1, 0), (8, 2, 1, 0), (16, 2, 2, 0), (16, 2, 4, 0), (32, 2, 4, 0),
        (24, 2, 64, 0), (12, 2, 1, 0), (12, 3, 1, 256), (8, 3, 1, 1024), (8, 2, 1, 1024)]
    assert [g.mid_clean for g in G.GEOMETRY_CASES] == [g.cols_per_wg == 1024 for g in G.GEOMETRY_CASES]
    assert G.expected_geometry(8, G.B_MAIN, 3, 1, 1024)["cols_per_wg"] == 384


def test_selections_are_scrambled_with_one_duplicate():
    for g in G.GEOMETRY_CASES:
        sel = G.selection(g)
        assert len(sel) == g.S and len(set(sel)) == g.S - 1 and 1 in sel
        assert all(0 <= s < g.S + G.EXTRA_STRIPES for s in sel)
        assert sel != sorted(sel)


@pytest.mark.parametrize("g", G.GEOMETRY_CASES, ids=G.geometry_id)
def test_every_chunk_holds_its_own_amount_of_damage(g):
    stripes = G.memo(("geometry", g.S, g.mid_clean), lambda: G.geometry_stripes(gf_plain.apply, M64, g))
    totals = set()
    for s in range(stripes.shape[0]):
        bad = gf_plain.apply(H64, stripes[s]).any(axis=0)
        per = [int(np.count_nonzero(bad[lo:hi])) for lo, hi in G.CHUNKS]
        if g.mid_clean and s == 1:
            assert per[1] == 0 and per[0] > 0 and per[2] > 0
        else:
            assert all(per) and len(set(per)) == len(per), (s, per)
            assert per == [G.chunk_count(s, w) for w in range(3)]
        for w, (lo, hi) in enumerate(G.CHUNKS):
            if per[w]:
                assert bad[lo:lo + 16].any() and bad[hi - 16:hi].any()      # the chunk's first and last column
        assert int(np.count_nonzero(bad[G.VEC_BYTES:])) == s % 2            # odd stripes: one tail byte
        votes = LP.votes(H64, stripes[s])
        assert votes[s % 10] == votes[10] == np.count_nonzero(bad) and votes[11] == 0   # one explaining candidate
        totals.add(tuple(per))
    assert len(totals) == stripes.shape[0]                                  # no two stripes alike


def wide_reference(n, r):
    """(C, stripes, votes [3][n + 2]) of a wide case, the votes by the definition; shared with the GPU tests."""
    def make():
        Cm, stripes = G.wide_stripes(gf_plain.apply, n, r)
        H = np.concatenate([Cm, np.eye(r, dtype=np.int64)], axis=1)
        return Cm, stripes, np.stack([LP.votes(H, stripes[s]) for s in range(3)])
    return G.memo(("wide", n, r), make)


@pytest.mark.parametrize("n,r", G.WIDE_CASES, ids=[f"n{n}-r{r}" for n, r in G.WIDE_CASES])
def test_wide_plans_reach_every_counter(n, r):
    Cm, stripes, votes = wide_reference(n, r)
    assert Cm.shape == (r, n - r) and votes.shape == (3, n + 2)
    assert not votes[0].any()                                               # the clean stripe
    total = sum(G.block_count(b) for b in range(n))
    assert votes[1, n] == total and votes[2, n] == total + G.WIDE_DOUBLES
    lo, hi = G.ONE_WAVE
    H = np.concatenate([Cm, np.eye(r, dtype=np.int64)], axis=1)
    bad = gf_plain.apply(H, stripes[1]).any(axis=0)
    assert bad[lo:hi].sum() == total and hi - lo == 1024 and lo % 1024 == 0   # all inside one wave's bytes
    bad = np.flatnonzero(gf_plain.apply(H, stripes[2]).any(axis=0))
    assert set(G.WIDE_EDGES) <= set(bad.tolist())
    if r < 2:
        return
    for s in (1, 2):
        assert (votes[s, :n] > 0).all() and votes[s, n] > 0, (s, votes[s])
    assert votes[2, n + 1] > 0
    for s in (1, 2):
        for edge in (63, 127):                                              # the last counter of a register and the next
            if edge + 1 < n + 2:
                assert votes[s, edge] != votes[s, edge + 1], (s, edge, votes[s])
