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

tests/test_gf_geometry_cases.py checks the tables and the plans without a GPU.
"""
import numpy as np
import pytest

import check_geometry_cases as G
import gf_arena as A
import gf_geometry_cases as F
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
