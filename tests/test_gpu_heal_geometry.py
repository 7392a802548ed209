"""The heal kernels at every launch geometry: each row of check_geometry_cases.GEOMETRY_CASES sets ECG_OPT_GRID_MAP /
ECG_OPT_MAP_GROUP / ECG_OPT_COLS_PER_WG and runs ecg_heal.encode_batch, ANY mode, over a scrambled selection of S
DISTINCT stripes out of S + 8 whose every 2 KiB chunk holds its own amount of damage
(tests/test_check_geometry_cases.py checks the plan), and compares

  - `last_launch()` with the geometry the table names, so that the case cannot quietly run the linear map;
  - the report with tests/heal_plain.py, exactly, and the `counters()` deltas with the declared traffic;
  - the WHOLE arena with the definition's image: the selected stripes healed, the other eight still damaged byte for
    byte, guard bands and the unnamed block untouched.

For the two read-only passes a workgroup -> chunk map that is no bijection loses or doubles a count; here the chunk it
skips stays damaged, and a chunk visited twice is read-modify-written by two workgroups.
"""
import json
import os

import numpy as np
import pytest

import check_geometry_cases as G
import gf_plain
import heal_plain as HP

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
def heal(ecg):
    import ecg_heal
    ecg_heal.lib()
    return ecg_heal


def distinct_selection(g):
    """S distinct ids out of S + EXTRA_STRIPES, scrambled, stripe 1 (the one with a clean middle chunk) among them."""
    rng = np.random.default_rng(200 * g.S + g.cols_per_wg + g.grid_map)
    ids = [int(v) for v in rng.permutation(g.S + G.EXTRA_STRIPES)]
    ids.remove(1)
    sel = ids[:g.S - 1]
    sel.insert(len(sel) // 2, 1)
    assert len(sel) == g.S == len(set(sel))
    return sel


def _reference(g):
    """(stripes [S + 8][n][B], healed [S + 8][n][B], reports [S + 8][n + 2]) of a case, ANY mode, by the definition."""
    def make():
        stripes = G.memo(("geometry", g.S, g.mid_clean), lambda: G.geometry_stripes(gf_plain.apply, M64, g))
        healed, reports = HP.heal_stripes(H64, stripes)
        return stripes, healed, reports
    return G.memo(("heal-geometry-reference", g.S, g.mid_clean), make)


def test_selections_are_distinct_and_references_heal():
    """No GPU: the selections this module hands the library hold no id twice, and the definition restores every
    stripe of the plan (one damaged block per stripe) to a stripe that satisfies the check."""
    for g in G.GEOMETRY_CASES:
        sel = distinct_selection(g)
        assert len(set(sel)) == g.S and 1 in sel and max(sel) < g.S + G.EXTRA_STRIPES
    g = G.GEOMETRY_CASES[0]
    stripes, healed, reports = _reference(g)
    for s in range(g.S + G.EXTRA_STRIPES):
        assert not gf_plain.apply(H64, healed[s]).any()
        assert reports[s, s % N] == reports[s, N] > 0 and reports[s, N + 1] == 0
        assert np.count_nonzero(healed[s] != stripes[s]) == reports[s, N]


@gpu
@pytest.mark.parametrize("g", G.GEOMETRY_CASES, ids=G.geometry_id)
def test_geometry(ecg, torch_cuda, heal, g):
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
        c0 = heal.counters()
        got = heal.encode_batch(K, M, flat, view, stripe_ids=ids)
        torch.cuda.synchronize()
        c1 = heal.counters()
        assert heal.last_launch() == dict(e, rtiles=1)
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
    # the selected stripes satisfy the check again, the others are as damaged as they were
    rest = sorted(set(range(total)) - set(sel))
    assert np.array_equal(after[rest], img[rest]) and (reports[rest, N] > 0).all()
