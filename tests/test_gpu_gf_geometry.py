"""The region-product kernels of libecg.so at every launch geometry: each (form, row) of tests/gf_geometry_cases.py
sets ECG_OPT_GRID_MAP / ECG_OPT_MAP_GROUP / ECG_OPT_COLS_PER_WG, makes the form's public call over guard-band arenas
and compares

  - `ecg.last_launch()` with the form's literal table, so that a case cannot quietly run another workgroup -> chunk
    map than the one it names, skip the row split, or lose the pointer-table launch's "outputs apart" hint;
  - the launch histogram's movement with the instantiations tests/gf_kernel_cases.py predicts;
  - the whole output arena with tests/gf_plain.py (never the library or the oracle), bit for bit: the named blocks,
    per stripe with that stripe's program, the bands, the unnamed slots and the stripes no launch stripe names -- a map
    that is no bijection leaves one 2 KiB chunk at its fill and writes another twice;
  - the input arena with what was uploaded.

The sweep's launches are vector launches.  The two other records launch_gf writes -- the byte kernel alone and the
latency kernel -- are pinned below it, all nine fields against literals and every output byte against gf_plain.

tests/test_gf_geometry_cases.py checks the tables and the plans without a GPU.
"""
import numpy as np
import pytest

import check_geometry_cases as G
import gf_arena as A
import gf_geometry_cases as F
import gf_kernel_cases as C
import gf_plain

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return torch


def _plan(form, S):
    return G.memo(("gf-geometry", form.name, S), lambda: F.plan(gf_plain.apply, form, S))


@gpu
@pytest.mark.parametrize("form,i", F.cases(), ids=[F.case_id(f, F.ROWS[i]) for f, i in F.cases()])
def test_geometry(ecg, torch_cuda, form, i):
    torch = torch_cuda
    g = F.ROWS[i]
    pl = _plan(form, g.S)
    keys = F.expected_keys(form, ecg.get_option(ecg.ECG_OPT_NT))
    d_in = A.to_dev(torch, pl.in_img)
    d_out = d_in if pl.out_img is None else A.to_dev(torch, pl.out_img)
    options = {ecg.ECG_OPT_GRID_MAP: g.grid_map, ecg.ECG_OPT_MAP_GROUP: g.map_group,
               ecg.ECG_OPT_COLS_PER_WG: g.cols_per_wg}
    if form.row_split:
        options[ecg.ECG_OPT_ROW_SPLIT] = F.ROW_SPLIT
    saved = [ecg.get_option(o) for o in range(ecg.ECG_OPT_COUNT)]
    try:
        for o, v in options.items():
            ecg.set_option(o, v)
        torch.cuda.synchronize()
        h0, l0 = ecg.launch_histogram(), ecg.traffic_counters()["launches"]
        F.run(ecg, torch, pl, d_in, d_out)
        torch.cuda.synchronize()
        h1, l1, last = ecg.launch_histogram(), ecg.traffic_counters()["launches"], ecg.last_launch()
    finally:
        for o, v in enumerate(saved):
            ecg.set_option(o, v)
    # the bytes and the report are looked at both before either fails the case: a wrong map shows in one, the other or both
    problems = []
    wr = F.written(pl)
    try:
        A.assert_same(d_out.cpu().numpy(), pl.want, F.B, lambda s, slot: (s, slot) in wr, F.case_id(form, g),
                      lambda s, slot, o: f"(chunk {o // G.CHUNK} of the block, column {o // 16})")
    except AssertionError as e:
        problems.append(f"bytes: {e}")
    if last != F.expected_report(form, i):
        problems.append(f"report: {last}, want {F.expected_report(form, i)}")
    assert not problems, (form.name, g, problems)
    delta = {key: h1.get(key, 0) - h0.get(key, 0) for key in set(h0) | set(h1)}
    delta = {key: n for key, n in delta.items() if n}
    assert delta == keys, (form.name, g, "launched", delta, "declared", keys)
    assert l1 - l0 == sum(keys.values()) == 2                    # one vector launch, one byte launch of the 5-byte tail
    if pl.out_img is not None:
        assert np.array_equal(d_in.cpu().numpy(), pl.in_img), (form.name, g, "the input arena changed")


# ---- the two records no vector launch writes: the byte kernel alone and the latency kernel.  Literals, read off
# launch_gf: a byte-only launch deals 16 * 128 = 2048 bytes to a workgroup (a block below that: its size rounded up to
# the 128 threads), the latency kernel 256 four-byte columns; both maps are linear (grid_map 0, map_group 1).

def _report(cols_per_wg, wg_per_stripe, S, mode, kernel):
    return {"grid_map": 0, "map_group": 1, "cols_per_wg": cols_per_wg, "wg_per_stripe": wg_per_stripe, "S": S,
            "rtiles": 1, "row_split": 0, "mode": mode, "kernel": kernel}


@gpu
@pytest.mark.parametrize("B,want_report", [(F.B, _report(2048, 3, 3, C.MODE_STRIDED, 1)),
                                           (100, _report(128, 1, 3, C.MODE_STRIDED, 1))], ids=["large", "below-one-wg"])
def test_byte_kernel_alone_report(ecg, torch_cuda, B, want_report):
    """A strided 5 -> 3 call over S = 3 stripes whose input arena starts one byte past a 16-byte boundary: no block is
    aligned, so the byte kernel runs alone over all B bytes."""
    torch = torch_cuda
    S, k, m = 3, 5, 3
    M = C.matrix(C._case("strided", 0, m, k, B, shift=1))
    src, dst = [k - j for j in range(k)], [p + 1 for p in range(m)]   # slot 0 (and m + 1 of the outputs) unnamed
    in_img, out_img = A.blank(S, k + 1, B), A.blank(S, m + 2, B)
    A.blocks(in_img, B)[:] = np.random.default_rng(B).integers(0, 256, (S, k + 1, B), dtype=np.uint8)
    want = out_img.copy()
    for s in range(S):
        A.blocks(want, B)[s, dst] = gf_plain.apply(M, A.blocks(in_img, B)[s, src])
    d_in, d_out = A.to_dev(torch, in_img, 1), A.to_dev(torch, out_img)
    torch.cuda.synchronize()
    ecg.matrix_apply_batch(M, src, dst, A.blocks(d_in, B), A.blocks(d_out, B))
    torch.cuda.synchronize()
    last = ecg.last_launch()
    A.assert_same(d_out.cpu().numpy(), want, B, lambda s, slot: slot in dst, ("byte kernel alone", B))
    assert np.array_equal(d_in.cpu().numpy(), in_img), (B, "the input arena changed")
    assert last == want_report, (B, last)


@gpu
@pytest.mark.parametrize("B,want_report", [(1024, _report(256, 1, 1, C.MODE_INLINE_LAT, 2)),
                                           (5120, _report(256, 5, 1, C.MODE_INLINE_LAT, 2))], ids=["small", "larger"])
def test_latency_kernel_report(ecg, torch_cuda, B, want_report):
    """A host-tier RS(6,4) ecg_ec_encode: one zero-copy call of the latency kernel."""
    k, m = 6, 4
    code = ecg.ec_factory(ecg.ECTYPE.RS, ecg.CodingParameters(k=k, m=m))
    M = np.asarray(code.make_encoding_matrix(), dtype=np.int64).reshape(m, k)
    data = np.random.default_rng(B).integers(0, 256, (k, B), dtype=np.uint8)
    kept = data.copy()
    out_img = A.blank(1, m + 2, B)
    want = out_img.copy()
    A.blocks(want, B)[0, 1:m + 1] = gf_plain.apply(M, data)
    code.encode([data[j] for j in range(k)], [A.blocks(out_img, B)[0, p + 1] for p in range(m)], B)
    last = ecg.last_launch()
    A.assert_same(out_img, want, B, lambda s, slot: 1 <= slot <= m, ("latency kernel", B))
    assert np.array_equal(data, kept), (B, "the inputs changed")
    assert last == want_report, (B, last)
