"""The tables and plans of tests/gf_geometry_cases.py, checked against the mirrored launch rule and the field's
definition alone (no GPU, no library): every form's literal table is what launch_gf's rule gives, between them the
rows reach every branch of wg_coords and every fallback, and the plans are what the forms promise -- so that the GPU
test's report and whole-arena compare mean what they say."""
import numpy as np
import pytest

import check_geometry_cases as G
import gf_arena as A
import gf_geometry_cases as F
import gf_kernel_cases as C
import gf_plain


def _plan(form, S):
    return G.memo(("gf-geometry", form.name, S), lambda: F.plan(gf_plain.apply, form, S))


def test_forms_are_the_seven_of_the_table():
    assert [(f.name, f.api, f.binary, f.k, f.m, f.in_stripe) for f in F.FORMS] == [
        ("strided-in", "apply", 0, 5, 3, True), ("strided-apart", "apply", 1, 7, 2, False),
        ("multi", "multi", 0, 3, 2, False), ("rowsplit", "multi", 0, 4, 2, False), ("tiles", "apply", 0, 3, 9, False),
        ("ptrs-apart", "scope", 0, 6, 1, False), ("ptrs-in", "scope", 0, 6, 1, True)]
    assert F.ROWS is G.GEOMETRY_CASES and len(F.cases()) == 7 * 12
    assert F.B == 4693 and G.CHUNKS == ((0, 2048), (2048, 4096), (4096, 4688))
    assert all(len(f.launch) == len(F.ROWS) for f in F.FORMS)


def test_auto_rule_resolves_before_the_fallbacks():
    e = F.expected_gf_geometry
    assert e(8, F.B, 3, 1, 0, True)["grid_map"] == 1 and e(8, F.B, 3, 1, 0, False)["grid_map"] == 2
    assert e(12, F.B, 3, 1, 0, False)["grid_map"] == 0          # 2 -> 1 (12 % 8), 1 -> 0 (gx = 36)
    assert e(12, F.B, 3, 1, 256, False)["grid_map"] == 1        # 2 -> 1, gx = 24 keeps it
    for gm in (0, 1, 2):                                        # a named map is the check libraries' rule as it stands
        for in_stripe in (True, False):
            assert e(16, F.B, gm, 2, 0, in_stripe) == G.expected_geometry(16, F.B, gm, 2, 0)


@pytest.mark.parametrize("form", F.FORMS, ids=[f.name for f in F.FORMS])
def test_table_agrees_with_the_mirrored_host_rule(form):
    R = form.row_split or 1
    for i, g in enumerate(F.ROWS):
        e = F.expected_gf_geometry(g.S * R, F.B, g.grid_map, g.map_group, g.cols_per_wg, form.in_stripe)
        assert (e["grid_map"], e["map_group"], e["wg_per_stripe"], e["S"]) == form.launch[i], (form.name, g)
        want = dict(e, rtiles=form.rtiles, row_split=form.row_split, mode=form.mode, kernel=0)
        assert F.expected_report(form, i) == want
        assert g.S <= F.MAX_SCOPE_CALLS
    assert (form.rtiles, form.row_split) == {"tiles": (2, 0), "rowsplit": (1, 2)}.get(form.name, (1, 0))
    assert form.mode == (C.MODE_PTRS if form.api == "scope" else C.MODE_STRIDED)
    if form.in_stripe:                                          # the check libraries' own table
        assert [l[:3] for l in form.launch] == [g.launch for g in F.ROWS]


def test_rows_reach_every_branch():
    reach = {f.name: f.launch for f in F.FORMS}
    opts = [(g.S, g.grid_map, g.map_group, g.cols_per_wg) for g in F.ROWS]
    for name, launch in reach.items():
        assert {l[0] for l in launch} == {0, 1, 2} or name == "rowsplit", name        # maps 0, 1 and 2
        assert {l[1] for l in launch if l[0] == 2} == {1, 2, 4}, name                 # groups 1, 2 and 4
        assert {l[2] for l in launch} == {1, 2, 3}, name                              # column loops of 3, 2, 1 rounds
    assert {l[0] for l in reach["rowsplit"]} == {0, 2}          # its S = 12 rows launch 24 stripes: map 2, never 1
    # each fallback, in every form that launches S stripes: gx % 8, S % 8G, G halved once, G halved all the way
    for name in ("strided-in", "strided-apart", "multi", "tiles", "ptrs-apart", "ptrs-in"):
        at = dict(zip(opts, reach[name]))
        assert at[(3, 3, 1, 0)][0] == 0                         # auto, gx = 9
        assert at[(12, 2, 1, 0)][0] == 0                        # map 2, 12 % 8: -> 1, gx = 36: -> 0
        assert at[(16, 2, 4, 0)][:2] == (2, 2)                  # G = 4 halved once
        assert at[(24, 2, 64, 0)][:2] == (2, 1)                 # G = 64 halved all the way
        assert at[(32, 2, 4, 0)][:2] == (2, 4) and at[(8, 0, 1, 0)][0] == 0
    # the auto rule both ways, for STRIDED and for PTRS
    auto = [i for i, o in enumerate(opts) if o[1] == 3 and o[0] % 8 == 0]
    assert len(auto) == 2
    for name, gm in (("strided-in", 1), ("strided-apart", 2), ("ptrs-in", 1), ("ptrs-apart", 2)):
        assert [reach[name][i][0] for i in auto] == [gm, gm], name
    # a row-split launch whose S is no multiple of 8 while S * R is; G = 4 tiles 2 * 16 stripes; 6 stripes stay linear
    at = dict(zip(opts, reach["rowsplit"]))
    assert at[(12, 2, 1, 0)] == (2, 1, 3, 24) and at[(12, 3, 1, 256)] == (2, 1, 2, 24)
    assert at[(16, 2, 4, 0)] == (2, 4, 3, 32) and at[(24, 2, 64, 0)] == (2, 2, 3, 48) and at[(3, 3, 1, 0)] == (0, 1, 3, 6)


def _apart(pl, s, src, dst):
    """engine.cpp outputs_apart on arena offsets, for a call whose outputs lie in its input arena."""
    P = A.pitch(F.B)
    at = lambda slot: (s * pl.in_img.shape[1] + slot) * P + A.GUARD
    lo, hi = min(at(j) for j in src), max(at(j) for j in src) + F.B
    return all(not (at(d) + F.B > lo and at(d) < hi + len(dst) * F.B) for d in dst)


@pytest.mark.parametrize("form", F.FORMS, ids=[f.name for f in F.FORMS])
def test_plans_are_what_the_forms_promise(form):
    for S in sorted({g.S for g in F.ROWS}):
        pl = _plan(form, S)
        named_in = {j for _, src, _ in pl.programs for j in src}
        named_out = {d for _, _, dst in pl.programs for d in dst}
        n_out = pl.want.shape[1]
        assert 0 not in named_in | named_out and n_out - 1 not in named_out          # unnamed slots at the edges
        for M, src, dst in pl.programs:
            assert M.shape == (form.m, form.k) == (len(dst), len(src))
            assert len(set(src)) == form.k and len(set(dst)) == form.m
            assert bool(M.max() <= 1) == bool(form.binary) and all(M[p].any() for p in range(form.m))
        assert any(src != sorted(src) for _, src, _ in pl.programs)                  # permuted ids
        assert (pl.out_img is None) == form.in_stripe
        if form.in_stripe:
            assert not named_in & named_out
        assert len(pl.stripes) == S == len(set(pl.stripes)) == len(pl.prog_of)
        assert set(pl.prog_of) == set(range(len(pl.programs)))                       # every program runs
        # the bands and what no call names keep their fill; the named outputs hold no fill
        base = pl.in_img if pl.out_img is None else pl.out_img
        wr = F.written(pl)
        for s in range(base.shape[0]):
            for slot in range(n_out):
                same = np.array_equal(pl.want[s, slot], base[s, slot])
                assert same != ((s, slot) in wr), (form.name, S, s, slot)
        assert np.array_equal(pl.want[:, :, :A.GUARD], base[:, :, :A.GUARD])
        assert np.array_equal(pl.want[:, :, A.GUARD + F.B:], base[:, :, A.GUARD + F.B:])
        if form.name in ("multi", "ptrs-apart", "ptrs-in"):                          # S of S + 8 stripes, scrambled
            assert base.shape[0] == S + F.EXTRA_STRIPES and pl.stripes != sorted(pl.stripes)
            assert len({b - a for a, b in zip(pl.stripes, pl.stripes[1:])}) > 1      # no strided batch
        else:
            assert pl.stripes == list(range(S))
        if form.name == "multi":
            assert len(pl.programs) == 3 and len({tuple(src) for _, src, _ in pl.programs}) == 3
            assert len({tuple(dst) for _, _, dst in pl.programs}) == 3
        if form.name == "rowsplit":
            for M, _, _ in pl.programs:                          # engine.cpp row_split: separable, two columns per row
                assert ((M != 0).sum(axis=0) == 1).all() and ((M != 0).sum(axis=1) == 2).all()
            assert form.k >= F.ROW_SPLIT and form.k % form.m == 0
            assert (pl.programs[0][0] != 0).tolist() != (pl.programs[1][0] != 0).tolist()
        if form.name == "tiles":
            assert C.tile(0, form.m) == (8, 2) and form.m - 8 == 1                   # a one-row last tile
        if form.name == "ptrs-in":
            assert not any(_apart(pl, s, *pl.programs[0][1:]) for s in pl.stripes)
        if form.api == "scope":
            assert C.tile(form.binary, form.m) == (1, 1)                             # the MT = 1 launch


def test_expected_image_runs_each_stripes_own_program():
    """The image of `multi` differs from what any single program would give, stripe by stripe."""
    form = next(f for f in F.FORMS if f.name == "multi")
    pl = _plan(form, 8)
    for i, s in enumerate(pl.stripes):
        for p, (M, src, dst) in enumerate(pl.programs):
            res = gf_plain.apply(M, pl.in_img[s, src, A.GUARD:A.GUARD + F.B])
            hit = all(np.array_equal(pl.want[s, d, A.GUARD:A.GUARD + F.B], res[q]) for q, d in enumerate(dst))
            assert hit == (p == pl.prog_of[i]), (s, p)


def test_keys_of_the_forms():
    for form in F.FORMS:
        mt = 1 if form.row_split else C.tile(form.binary, form.m)[0]
        assert F.expected_keys(form, 3) == {("vec", form.mode, form.binary, 3, mt): 1, ("byte", form.mode, form.binary, mt): 1}
