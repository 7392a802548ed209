"""The scrub and locate kernels at every launch geometry: each row of check_geometry_cases.GEOMETRY_CASES sets
ECG_OPT_GRID_MAP / ECG_OPT_MAP_GROUP / ECG_OPT_COLS_PER_WG, runs both libraries over stripes whose every 2 KiB chunk
holds its own amount of damage (tests/test_check_geometry_cases.py checks the plan), and compares

  - the counts with tests/gf_plain.py and the votes with tests/locate_plain.py, exactly;
  - `last_launch()` with the geometry the table names, so that the case cannot quietly run the linear map;
  - the arena with what was uploaded, guard bands included, and the `counters()` deltas with the declared traffic.

The scrub runs RS(6,4) as [C | I], the same check with its columns reversed (a general H) and a 17-row GENERAL H whose
rows are combinations of the RS check's (three row tiles on gridDim.y, still zero on consistent stripes).  The locate
runs the first two through a scrambled selection with a duplicate out of S + 8 stripes: the launch stripe picks the
votes row, the selection the stripe that is read.
"""
import json
import os

import numpy as np
import pytest

import check_geometry_cases as G
import gf_plain
import locate_plain as LP

HERE = os.path.dirname(os.path.abspath(__file__))
RS64 = next(c for c in json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"] if c["name"] == "RS(6,4)")
K, M, N, B = 6, 4, 10, G.B_MAIN
M64 = np.asarray(RS64["matrix"], dtype=np.int64).reshape(M, K)
H64 = np.concatenate([M64, np.eye(M, dtype=np.int64)], axis=1)
# 17 rows, each a combination of the RS check's four: zero on every stripe that satisfies the RS check
H17 = gf_plain.apply(np.random.default_rng(17).integers(1, 256, (17, M)), H64.astype(np.uint8)).astype(np.int64)
GUARD, BAND = 64, 0xC3
PITCH = (GUARD + B + GUARD + 15) & ~15
SRC = list(range(1, N + 1))          # slot 0 of every stripe is not named
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return torch


@pytest.fixture(scope="module")
def scrub(ecg):
    import ecg_scrub
    ecg_scrub.lib()
    return ecg_scrub


@pytest.fixture(scope="module")
def locate(ecg):
    import ecg_locate
    ecg_locate.lib()
    return ecg_locate


def _reference(g):
    """(stripes [S + 8][n][B], counts {check: [S + 8][r]}, votes [S + 8][n + 2]) of a case, by the definitions."""
    def make():
        stripes = G.memo(("geometry", g.S, g.mid_clean), lambda: G.geometry_stripes(gf_plain.apply, M64, g))
        counts = {name: np.array([[np.count_nonzero(row) for row in gf_plain.apply(H, st)] for st in stripes])
                  for name, H in (("ci", H64), ("h17", H17))}
        votes = np.stack([LP.votes(H64, st) for st in stripes])
        return stripes, counts, votes
    return G.memo(("geometry-reference", g.S, g.mid_clean), make)


def _upload(torch, stripes):
    S = stripes.shape[0]
    img = np.full((S, N + 1, PITCH), BAND, np.uint8)
    img[:, 0, GUARD:GUARD + B] = 0x77
    img[:, 1:, GUARD:GUARD + B] = stripes
    return img, torch.from_numpy(img).cuda()


def _expected(g, rtiles):
    e = G.expected_geometry(g.S, B, g.grid_map, g.map_group, g.cols_per_wg)
    assert (e["grid_map"], e["map_group"], e["wg_per_stripe"]) == g.launch
    return dict(e, rtiles=rtiles)


def _run(torch, lib, call, img, d, geometry, nbytes):
    """One call: its result (numpy), after checking the launch geometry, the arena and the traffic counters."""
    c0 = lib.counters()
    got = call()
    torch.cuda.synchronize()
    c1 = lib.counters()
    assert lib.last_launch() == geometry
    assert np.array_equal(d.cpu().numpy(), img), "the call wrote to its inputs"
    assert c1["launches"] - c0["launches"] == 2          # the vector kernel and the byte kernel of the 5-byte tail
    assert c1["bytes"] - c0["bytes"] == nbytes
    assert got.dtype == torch.int32
    return got.cpu().numpy().astype(np.int64)


@gpu
@pytest.mark.parametrize("g", G.GEOMETRY_CASES, ids=G.geometry_id)
def test_geometry(ecg, torch_cuda, scrub, locate, g):
    torch = torch_cuda
    stripes, counts, votes = _reference(g)
    img, d = _upload(torch, stripes)
    view = d[:, :, GUARD:GUARD + B]
    S = g.S
    sel = G.selection(g)
    ids = torch.tensor(sel, dtype=torch.int32, device="cuda")
    flat = [int(v) for v in M64.reshape(-1)]
    Hr, srcr = H64[:, ::-1].copy(), SRC[::-1]
    options = {ecg.ECG_OPT_GRID_MAP: g.grid_map, ecg.ECG_OPT_MAP_GROUP: g.map_group,
               ecg.ECG_OPT_COLS_PER_WG: g.cols_per_wg}
    saved = {o: ecg.get_option(o) for o in options}
    try:
        for o, v in options.items():
            ecg.set_option(o, v)
        # ---- the scrub over the first S stripes
        # [C | I]: C's 6 columns through the tables, the 4 stored parities read once; a general H: all 10, per row tile
        for name, H, src, rtiles, per_stripe in (("ci", H64, SRC, 1, K + M), ("ci", Hr, srcr, 1, N),
                                                 ("h17", H17, SRC, 3, 3 * N)):
            got = _run(torch, scrub, lambda: scrub.matrix_batch(H, src, view[:S]), img, d, _expected(g, rtiles),
                       S * B * per_stripe)
            assert np.array_equal(got, counts[name][:S]), (name, got, counts[name][:S])
        # ---- the locate over the selection
        want = votes[sel]
        assert len({tuple(votes[s]) for s in sel}) == S - 1          # every selected stripe has votes of its own
        got = _run(torch, locate, lambda: locate.encode_batch(K, M, flat, view[:, 1:], stripe_ids=ids), img, d,
                   _expected(g, 1), S * B * N)
        assert np.array_equal(got, want), (got, want)
        got = _run(torch, locate, lambda: locate.matrix_batch(Hr, srcr, view, stripe_ids=ids), img, d,
                   _expected(g, 1), S * B * N)
        assert np.array_equal(got[:, :N], want[:, N - 1::-1]) and np.array_equal(got[:, N:], want[:, N:]), (got, want)
        for row, s in zip(got, sel):                                  # and each names its stripe's damaged block
            assert locate.verdict(row) == (N - 1 - s % N, [N - 1 - s % N])
    finally:
        for o, v in saved.items():
            ecg.set_option(o, v)
