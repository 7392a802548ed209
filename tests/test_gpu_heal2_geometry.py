"""The heal2 kernels at every launch geometry: each row of check_geometry_cases.GEOMETRY_CASES sets ECG_OPT_GRID_MAP /
ECG_OPT_MAP_GROUP / ECG_OPT_COLS_PER_WG and runs ecg_heal2.encode_batch, ANY2, over a scrambled selection of S
DISTINCT stripes out of S + 8.  Every 2 KiB chunk of every stripe holds the geometry plan's own amount of single-block
damage (tests/test_check_geometry_cases.py checks the plan) and, on top of it, pair damage: two positions per chunk,
one of them in the chunk's last column, in two blocks that differ from stripe to stripe.  The test compares

  - `last_launch()` with the geometry the table names, so that the case cannot quietly run the linear map;
  - the report with tests/heal2_plain.py, exactly, and the `counters()` deltas with the declared traffic;
  - the WHOLE arena with the definition's image: the selected stripes healed, the other eight still damaged byte for
    byte, guard bands and the unnamed block untouched.

A chunk that a workgroup -> chunk map skips stays damaged, and a chunk visited twice is read-modify-written by two
workgroups.
"""
import json
import os

import numpy as np
import pytest

import check_geometry_cases as G
import gf_plain
import heal2_plain as P

HERE = os.path.dirname(os.path.abspath(__file__))
RS64 = next(c for c in json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"] if c["name"] == "RS(6,4)")
K, M, N, B = 6, 4, 10, G.B_MAIN
M64 = np.asarray(RS64["matrix"], dtype=np.int64).reshape(M, K)
H64 = np.concatenate([M64, np.eye(M, dtype=np.int64)], axis=1)
GUARD, BAND = 64, 0xC3
PITCH = (GUARD + B + GUARD + 15) & ~15
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return torch


@pytest.fixture(scope="module")
def heal2(ecg):
    import ecg_heal2
    ecg_heal2.lib()
    return ecg_heal2


def distinct_selection(g):
    """S distinct ids out of S + EXTRA_STRIPES, scrambled, stripe 1 (the one with a clean middle chunk) among them."""
    rng = np.random.default_rng(300 * g.S + g.cols_per_wg + g.grid_map)
    ids = [int(v) for v in rng.permutation(g.S + G.EXTRA_STRIPES)]
    ids.remove(1)
    sel = ids[:g.S - 1]
    sel.insert(len(sel) // 2, 1)
    assert len(sel) == g.S == len(set(sel))
    return sel


def pair_positions(s, taken=()):
    """Two positions per 2 KiB chunk for stripe s's pair damage: one early in the chunk, one in its last column, moved
    on past the positions in `taken` (the stripe's single-block damage: a third block there would hide the pair)."""
    out = []
    for lo, hi in G.CHUNKS:
        early = lo + 32 + s % 29
        while early in taken:
            early += 1
        last = next(p for i in range(16) for p in [hi - 16 + (15 - s % 16 - i) % 16] if p not in taken)
        out += [early, last]
    return out


def pair_blocks(s):
    return (s + 1) % N, (s + 4) % N


def _reference(g):
    """(stripes [S + 8][n][B], healed, reports [S + 8][n + 3]) of a case, ANY2, by the definition."""
    def make():
        stripes = G.geometry_stripes(gf_plain.apply, M64, g).copy()
        rng = np.random.default_rng(17 + g.S)
        plan = G.geometry_plan(stripes.shape[0], N, g.mid_clean)
        for s in range(stripes.shape[0]):
            a, b = pair_blocks(s)
            taken = {int(p) for ps, _, pos, _ in plan if ps == s for p in pos}
            for p in pair_positions(s, taken):
                stripes[s, a, p] ^= rng.integers(1, 256, dtype=np.uint8)
                stripes[s, b, p] ^= rng.integers(1, 256, dtype=np.uint8)
        healed, reports = P.heal2_stripes(H64, stripes)
        return stripes, healed, reports
    return G.memo(("heal2-geometry-reference", g.S, g.mid_clean), make)


def test_selections_are_distinct_and_references_hold_pairs():
    """No GPU: the selections hold no id twice, and in the definition's image every chunk of every stripe has pairs
    that were corrected."""
    for g in G.GEOMETRY_CASES:
        sel = distinct_selection(g)
        assert len(set(sel)) == g.S and 1 in sel and max(sel) < g.S + G.EXTRA_STRIPES
    g = G.GEOMETRY_CASES[0]
    stripes, healed, reports = _reference(g)
    assert len(pair_positions(0)) == 2 * len(G.CHUNKS) and len(set(pair_positions(5))) == 6
    for s in range(g.S + G.EXTRA_STRIPES):
        assert reports[s, N + 2] == 2 * len(G.CHUNKS) and reports[s, N] > reports[s, N + 2] and reports[s, N + 1] == 0
        assert reports[s, :N].sum() - reports[s, N + 2] + reports[s, N + 1] == reports[s, N]
        for lo, hi in G.CHUNKS:
            a, b = pair_blocks(s)
            assert np.count_nonzero(healed[s, a, lo:hi] != stripes[s, a, lo:hi]) == 2


@gpu
@pytest.mark.parametrize("g", G.GEOMETRY_CASES, ids=G.geometry_id)
def test_geometry(ecg, torch_cuda, heal2, g):
    torch = torch_cuda
    stripes, healed, reports = _reference(g)
    sel = distinct_selection(g)
    total = g.S + G.EXTRA_STRIPES
    img = np.full((total, N + 1, PITCH), BAND, np.uint8)
    img[:, 0, GUARD:GUARD + B] = 0x77                    # slot 0 of every stripe is not named
    img[:, 1:, GUARD:GUARD + B] = stripes
    want = img.copy()
    want[sel, 1:, GUARD:GUARD + B] = healed[sel]
    d = torch.from_numpy(img).cuda()
    view = d[:, 1:, GUARD:GUARD + B]
    ids = torch.tensor(sel, dtype=torch.int32, device="cuda")
    flat = [int(v) for v in M64.reshape(-1)]
    e = G.expected_geometry(g.S, B, g.grid_map, g.map_group, g.cols_per_wg)
    assert (e["grid_map"], e["map_group"], e["wg_per_stripe"]) == g.launch
    options = {ecg.ECG_OPT_GRID_MAP: g.grid_map, ecg.ECG_OPT_MAP_GROUP: g.map_group,
               ecg.ECG_OPT_COLS_PER_WG: g.cols_per_wg}
    saved = {o: ecg.get_option(o) for o in options}
    try:
        for o, v in options.items():
            ecg.set_option(o, v)
        c0 = heal2.counters()
        got = heal2.encode_batch(K, M, flat, view, stripe_ids=ids)
        torch.cuda.synchronize()
        c1 = heal2.counters()
        assert heal2.last_launch() == dict(e, rtiles=1)
    finally:
        for o, v in saved.items():
            ecg.set_option(o, v)
    assert c1["launches"] - c0["launches"] == 2          # the vector kernel and the byte kernel of the 5-byte tail
    assert c1["bytes"] - c0["bytes"] == g.S * B * N
    assert got.dtype == torch.int32
    got = got.cpu().numpy().astype(np.int64)
    assert np.array_equal(got, reports[sel]), (got, reports[sel])
    assert len({tuple(row) for row in got}) == g.S       # every selected stripe has a report of its own
    after = d.cpu().numpy()
    if not np.array_equal(after, want):
        diff = np.argwhere(after != want)
        raise AssertionError((len(diff), diff[:8].tolist()))
    # the stripes outside the selection are as damaged as they were
    rest = sorted(set(range(total)) - set(sel))
    assert np.array_equal(after[rest], img[rest]) and (reports[rest, N] > 0).all()
