"""Launch geometries of the region-product kernels (gf_vec_kernel, gf_byte_kernel) of libecg.so: helper of
tests/test_gf_geometry_cases.py and tests/test_gpu_gf_geometry.py; numpy only, imports nothing of the project (the
library and torch are handed in).  It does for the product what tests/check_geometry_cases.py does for the check
libraries, and uses that module's geometry rows and its mirror of the launch rule's fallbacks.

Geometry.  `expected_gf_geometry` resolves launch_gf's auto rule (gf_kernels.hip outputs_in_stripe: ECG_OPT_GRID_MAP 3
is map 1 when the outputs are blocks of the input stripes, else map 2; a pointer-table launch counts as "apart" only
when every call's outputs lie apart from its inputs, engine.cpp outputs_apart) and hands the rest to
check_geometry_cases.expected_geometry.  Every FORM is one public call shape that reaches launch_gf by another road:
the strided launch with outputs inside and outside the input stripes, several programs with prog_of_stripe and
stripe_of, a row split (launch stripes = stripes x rows), two row tiles (grid.y = 2), and a batch scope's
pointer-table flush both ways.  Each form carries a literal table of what `ecg.last_launch()` must report on each
of the twelve rows of check_geometry_cases.GEOMETRY_CASES.

Bytes.  Any bijection of workgroups onto chunks gives right bytes, so a map is only seen by a compare of the whole
output: `plan` builds the arenas of a (form, S) (tests/gf_arena.py: guard bands, unnamed slots, permuted ids) and the
expected image from the field's definition, per stripe with that stripe's program.  B is B_MAIN = 4693: chunks of
128, 128 and 37 columns and a 5-byte tail.
"""
from collections import namedtuple

import numpy as np

import check_geometry_cases as G
import gf_arena as A
import gf_kernel_cases as C

B = G.B_MAIN
EXTRA_STRIPES = G.EXTRA_STRIPES   # `multi` and the `ptrs` forms address S of S + 8 stripes
MAX_SCOPE_CALLS = 40              # the largest S of a `ptrs` form: far below the scope's automatic flush (1024 calls)
ROW_SPLIT = 4                     # the ECG_OPT_ROW_SPLIT the `rowsplit` form sets (the least k_in that splits)


def expected_gf_geometry(S_launch, B, grid_map, map_group, cols_per_wg, in_stripe):
    """{grid_map, map_group, cols_per_wg, wg_per_stripe, S} of launch_gf's vector launch over S_launch launch stripes
    of B bytes with the three options as given.  in_stripe: the outputs are blocks of the input stripes (STRIDED: same
    stripe stride and the output base inside the first input stripe; PTRS: some call's outputs are not apart)."""
    if grid_map == 3:                     # if (gm == 3) gm = outputs_in_stripe(a, mode) ? 1 : 2;
        grid_map = 1 if in_stripe else 2
    return G.expected_geometry(S_launch, B, grid_map, map_group, cols_per_wg)


# api: "apply" ecg.matrix_apply_batch, "multi" ecg.matrix_apply_batch_multi, "scope" S ecg.dev_matrix_encode calls in
# one ecg.batch().  in_stripe: the outputs lie in the input arena.  rtiles / row_split / mode: what the launch must
# report.  launch: per row of GEOMETRY_CASES the (grid_map, map_group, wg_per_stripe, S_launch) it must report.
Form = namedtuple("Form", "name api binary k m in_stripe rtiles row_split mode launch")

# outputs inside the input stripes: auto is map 1, so the rows are those of the check libraries' table
_IN = ((0, 1, 3, 3), (1, 1, 3, 8), (0, 1, 3, 8), (2, 1, 3, 8), (2, 2, 3, 16), (2, 2, 3, 16), (2, 4, 3, 32), (2, 1, 3, 24),
       (0, 1, 3, 12), (1, 1, 2, 12), (1, 1, 1, 8), (2, 1, 1, 8))
# outputs apart: auto is map 2 (rows 1 and 10); S = 3 and S = 12 are no multiples of 8, so auto falls to map 1 there,
# and on to map 0 where gx = 9 is no multiple of 8 (row 0) while gx = 24 keeps map 1 (row 9)
_APART = ((0, 1, 3, 3), (2, 1, 3, 8), (0, 1, 3, 8), (2, 1, 3, 8), (2, 2, 3, 16), (2, 2, 3, 16), (2, 4, 3, 32),
          (2, 1, 3, 24), (0, 1, 3, 12), (1, 1, 2, 12), (2, 1, 1, 8), (2, 1, 1, 8))
# two rows per program: 2 S launch stripes.  S = 16 tiles G = 4 after all (32 stripes), S = 24 halves G = 64 down to 2
# (48 = 3 * 16), and S = 12 -- no multiple of 8 -- launches 24 stripes and takes map 2; S = 3 launches 6: gx = 18, map 0
_SPLIT = ((0, 1, 3, 6), (2, 1, 3, 16), (0, 1, 3, 16), (2, 1, 3, 16), (2, 2, 3, 32), (2, 4, 3, 32), (2, 4, 3, 64),
          (2, 2, 3, 48), (2, 1, 3, 24), (2, 1, 2, 24), (2, 1, 1, 16), (2, 1, 1, 16))

FORMS = (
    Form("strided-in", "apply", 0, 5, 3, True, 1, 0, C.MODE_STRIDED, _IN),
    Form("strided-apart", "apply", 1, 7, 2, False, 1, 0, C.MODE_STRIDED, _APART),
    Form("multi", "multi", 0, 3, 2, False, 1, 0, C.MODE_STRIDED, _APART),
    Form("rowsplit", "multi", 0, 4, 2, False, 1, 2, C.MODE_STRIDED, _SPLIT),
    Form("tiles", "apply", 0, 3, 9, False, 2, 0, C.MODE_STRIDED, _APART),
    Form("ptrs-apart", "scope", 0, 6, 1, False, 1, 0, C.MODE_PTRS, _APART),
    Form("ptrs-in", "scope", 0, 6, 1, True, 1, 0, C.MODE_PTRS, _IN),
)
ROWS = G.GEOMETRY_CASES


def case_id(form, g):
    return f"{form.name}-{G.geometry_id(g)}"


def cases():
    return [(f, i) for f in FORMS for i in range(len(ROWS))]


def expected_report(form, i):
    """ecg.last_launch() after the form's call on row i of ROWS, from the literal table."""
    gm, grp, wps, s_launch = form.launch[i]
    cpw = G.expected_geometry(ROWS[i].S, B, 0, 1, ROWS[i].cols_per_wg)["cols_per_wg"]
    return {"grid_map": gm, "map_group": grp, "cols_per_wg": cpw, "wg_per_stripe": wps, "S": s_launch,
            "rtiles": form.rtiles, "row_split": form.row_split, "mode": form.mode, "kernel": 0}


def key_case(form, nt):
    """The gf_kernel_cases.Case whose expected_keys are the form's: the launch runs `m` rows of `k` inputs -- one row
    of k / m inputs under the row split."""
    R = form.row_split or 1
    return C._case("ptrs" if form.api == "scope" else "strided", form.binary, form.m // R, form.k // R, B, nt=nt)


def expected_keys(form, nt):
    """{key: launches} of the form's call at ECG_OPT_NT = nt (gf_kernel_cases.expected_keys): one vector launch and one
    byte launch of the 5-byte tail."""
    c = key_case(form, nt)
    return C.expected_keys(c, np.full((c.m, c.k), 1 if form.binary else 2))


def scramble(S, total, seed):
    """S distinct stripe ids out of `total`, in no order a stride describes (so a scope's calls over them form no
    strided batch, engine.cpp run_calls_strided)."""
    ids = [int(v) for v in np.random.default_rng(seed).permutation(total)[:S]]
    steps = {b - a for a, b in zip(ids, ids[1:])}
    if len(steps) == 1:                   # an arithmetic run by chance: break it
        ids[-1] = next(v for v in range(total) if v not in ids)
    return ids


def _matrix(form, p=0):
    c = C._case("strided", form.binary, form.m, form.k, B)
    return C.matrix(c._replace(seed=c.seed + 7919 * p))


def _separable(form, p):
    """GENERAL 2 x 4 whose every column is used by exactly one row, two columns per row: the supports differ between
    the programs; coefficients from 2 up."""
    support = (((0, 2), (1, 3)), ((1, 2), (0, 3)))[p]
    rng = np.random.default_rng(C._case("strided", 0, form.m, form.k, B).seed + 7919 * p)
    M = np.zeros((form.m, form.k), np.int64)
    for r, cols in enumerate(support):
        M[r, list(cols)] = rng.integers(2, 256, len(cols))
    return M


Plan = namedtuple("Plan", "form S in_img out_img want programs prog_of stripes")
# in_img / out_img: the uploaded arenas; out_img is None when the outputs lie in the input arena.  want: the output
# arena (the one arena then) after the call.  programs: [(M, src slots, dst slots)].  prog_of[i] / stripes[i]: the
# program and the stripe of launch stripe (or scope call) i.


def plan(apply, form, S):
    """The arenas, programs and expected image of (form, S).  `apply` is tests/gf_plain.py apply, handed in."""
    k, m = form.k, form.m
    seed = C._case(form.name, form.binary, m, k, B).seed ^ (0x5EED + S)
    rng = np.random.default_rng(seed)
    sub = form.name in ("multi", "ptrs-apart", "ptrs-in")
    NS = S + EXTRA_STRIPES if sub else S
    stripes = scramble(S, NS, seed) if sub else list(range(S))
    prog_of = [0] * S
    if form.in_stripe:
        # one arena: slot 0 and the last slot unnamed, the others dealt to inputs and outputs, both permuted
        slots = [int(v) for v in rng.permutation(np.arange(1, k + m + 1))]
        if form.api == "scope" and slots[k] == 1:
            # an output block below every input is "apart" to the engine (outputs_apart looks at the input span and the
            # m blocks past it): keep it inside the span
            slots[0], slots[k] = slots[k], slots[0]
        programs = [(_matrix(form), slots[:k], slots[k:])]
        in_img = A.blank(NS, k + m + 2, B)
        data = rng.integers(0, 256, (NS, k, B), dtype=np.uint8)
        for j, slot in enumerate(slots[:k]):
            in_img[:, slot, A.GUARD:A.GUARD + B] = data[:, j]
        out_img = None
    else:
        # input arena: slot 0 unnamed; output arena: slot 0 and the last slot unnamed.  A block is GUARD + pitch bytes or
        # more from either end of its arena, so wherever the two allocations lie, an output block is more than B bytes
        # from a call's input span (outputs_apart)
        n_in = (6 if form.name == "multi" else k) + 1
        n_out = (5 if form.name == "multi" else m) + 2
        in_img = A.blank(NS, n_in, B)
        in_img[:, :, A.GUARD:A.GUARD + B] = rng.integers(0, 256, (NS, n_in, B), dtype=np.uint8)
        out_img = A.blank(NS, n_out, B)
        if form.name == "multi":
            ids = (([4, 2, 6], [3, 1]), ([1, 5, 3], [2, 4]), ([6, 3, 2], [5, 3]))
            programs = [(_matrix(form, p), *ids[p]) for p in range(3)]
            prog_of = [int(v) for v in np.random.default_rng(seed + 1).permutation(S) % 3]
        elif form.name == "rowsplit":
            programs = [(_separable(form, 0), [3, 1, 4, 2], [2, 1]), (_separable(form, 1), [2, 4, 1, 3], [1, 2])]
            prog_of = [int(v) for v in np.random.default_rng(seed + 1).permutation(S) % 2]
        else:
            src = [int(v) for v in rng.permutation(np.arange(1, k + 1))]
            dst = [int(v) for v in rng.permutation(np.arange(1, m + 1))]
            programs = [(_matrix(form), src, dst)]
    want = (in_img if out_img is None else out_img).copy()
    for i, s in enumerate(stripes):
        M, src, dst = programs[prog_of[i]]
        res = apply(M, in_img[s, src, A.GUARD:A.GUARD + B])
        for p, slot in enumerate(dst):
            want[s, slot, A.GUARD:A.GUARD + B] = res[p]
    return Plan(form, S, in_img, out_img, want, programs, prog_of, stripes)


def written(pl):
    """{(stripe, slot)} of the blocks the plan's call writes."""
    return {(s, slot) for i, s in enumerate(pl.stripes) for slot in pl.programs[pl.prog_of[i]][2]}


def run(ecg, torch, pl, d_in, d_out):
    """The plan's public call on the uploaded arenas (d_out is d_in when the outputs lie in the input arena)."""
    form, S = pl.form, pl.S
    vin, vout = A.blocks(d_in, B), A.blocks(d_out, B)
    if form.api == "apply":
        M, src, dst = pl.programs[0]
        ecg.matrix_apply_batch(M, src, dst, vin, vout)
    elif form.api == "multi":
        dev = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
        sub = pl.stripes != list(range(S))
        ecg.matrix_apply_batch_multi([(M, src, dst) for M, src, dst in pl.programs], vin, vout,
                                     prog_of_stripe=dev(pl.prog_of), stripe_of=dev(pl.stripes) if sub else None,
                                     n_launch=S)
    else:
        M, src, dst = pl.programs[0]
        flat = [int(v) for v in M.reshape(-1)]
        with ecg.batch():
            for s in pl.stripes:
                ecg.dev_matrix_encode(form.k, form.m, flat, [vin[s, j] for j in src], [vout[s, p] for p in dst], B)
