"""The check and checksum kernels across the 64-bit address range: libecg_scrub, libecg_locate, libecg_heal,
libecg_heal2 and libecg_sum (and, once, the region product) where base + stripe * sstride + block_id * bstride + offset,
a column count or a report row no longer fits 32, 31 or 16 bits.  tests/address_range_cases.py holds the layouts and
plans, tests/test_address_range_cases.py checks them without a GPU.

  A  `sparse`: two stripes of six 4693-byte blocks in a 24.1 GiB `torch.empty` arena, block stride 2^31 + 4096, so
     that the blocks lie past 2^31, 2^32 and 2^33.  Only the twelve windows [block - 64, block + 4693 + 64) are ever
     written, read by a kernel or compared; THE REST OF THE ARENA IS UNINITIALISED and is not looked at.  Every case
     runs on the aligned view and on the view moved up by one byte, where only the byte kernels run.
  B  `big`: one stripe of six blocks of 2^31 - 1 bytes (12 GiB, zero but for constant fills).  Expected counters come
     from the plain references on a 21-byte replica with the same fills (the layer is per byte position), scaled.
  C  `dense`: 65 600 selected stripes of 53 bytes out of 65 608, about forty of them damaged, each by its own amount;
     the whole report and the whole arena are compared.

Every check case runs in two forms: `encode_batch` (H = [C | I]: the stored blocks addressed as ident_base + q) and
`matrix_batch` with the six columns permuted (all through the tables).  References are tests/gf_plain.py,
locate_plain.py, heal_plain.py, heal2_plain.py and crc32c_plain.py, never the library.  One arena is held at a time.
"""
import contextlib

import numpy as np
import pytest

import address_range_cases as AR
import check_geometry_cases as G
import crc32c_plain as CP
import gf_plain
import heal2_plain as P2
import heal_plain as HP
import locate_plain as LP

K, R, N = AR.K, AR.R, AR.N
CM = P2.cauchy(R, K)
H = AR.check_matrix(CM)
H_PERM, SRC_PERM = AR.permuted(H)
FLAT = [int(v) for v in CM.reshape(-1)]
# (name, the block each reported column stands for, the call)
FORMS = (("encode", tuple(range(N)), lambda lib, view, **kw: lib.encode_batch(K, R, FLAT, view, **kw)),
         ("matrix", AR.PERM, lambda lib, view, **kw: lib.matrix_batch(H_PERM, SRC_PERM, view, **kw)))
by_form = pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
EXTRA = {"locate": 2, "heal": 2, "heal2": 3}            # counters behind the n per-block ones
AUTO_SEGMENT = 256 << 10                                 # sum_kernels.hpp kSumAutoSegment
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return torch


@pytest.fixture(scope="module")
def libs(ecg):
    import ecg_heal
    import ecg_heal2
    import ecg_locate
    import ecg_scrub
    import ecg_sum
    out = {"scrub": ecg_scrub, "locate": ecg_locate, "heal": ecg_heal, "heal2": ecg_heal2, "sum": ecg_sum}
    for lib in out.values():
        lib.lib()
    ecg_sum.set_segment_bytes(0)
    ecg_sum.set_table_scheme(-1)
    return out


@pytest.fixture(scope="module")
def arenas(torch_cuda):
    """get(name, make): the module's arena of that name, made on first use after the one held before it is freed, so
    that the peak is the largest arena (part A's) and nothing is left for the rest of the suite."""
    held = {}

    def get(name, make):
        if name not in held:
            held.clear()
            torch_cuda.cuda.empty_cache()
            held[name] = make()
        return held[name]

    yield get
    for name in list(held):
        del held[name]
    torch_cuda.cuda.empty_cache()


def _reference(lib, stripe):
    """One stripe's result by the definition: the scrub's counts, the locate's votes, a heal's report."""
    if lib == "scrub":
        return np.array([np.count_nonzero(row) for row in gf_plain.apply(H, stripe)], dtype=np.int64)
    if lib == "locate":
        return LP.votes(H, stripe)
    return (HP.heal(H, stripe) if lib == "heal" else P2.heal2(H, stripe))[1]


def _in_form_order(lib, want, cols):
    """`want` as a call whose columns stand for the blocks `cols` reports it (the scrub's counts are per check row)."""
    return want if lib == "scrub" else AR.in_column_order(want, cols, EXTRA[lib])


def _counted(torch, lib, call, launches, nbytes):
    """One call of a check library: its result (numpy int64), after checking the `counters()` deltas."""
    c0 = lib.counters()
    got = call()
    torch.cuda.synchronize()
    c1 = lib.counters()
    assert c1["launches"] - c0["launches"] == launches, (c0, c1)
    assert c1["bytes"] - c0["bytes"] == nbytes, (c0, c1)
    assert got.dtype == torch.int32
    return got.cpu().numpy().astype(np.int64)


def _ints(torch, values):
    return torch.tensor([int(v) for v in values], dtype=torch.int32, device="cuda")


@contextlib.contextmanager
def _with_options(ecg, options):
    """The options set for the block, and put back whatever happens in it."""
    saved = {o: ecg.get_option(o) for o in options}
    try:
        for o, v in options.items():
            ecg.set_option(o, v)
        yield
    finally:
        for o, v in saved.items():
            ecg.set_option(o, v)


def _expected_launch(ecg, S, B):
    """What last_launch() must read with the options as they stand."""
    e = G.expected_geometry(S, B, ecg.get_option(ecg.ECG_OPT_GRID_MAP), ecg.get_option(ecg.ECG_OPT_MAP_GROUP),
                            ecg.get_option(ecg.ECG_OPT_COLS_PER_WG))
    return dict(e, rtiles=1)


# ---------------------------------------------------------------------------------------------------------------------
# Part A: the sparse arena

SHIFT_IDS = ["aligned", "shifted"]


def _sparse(torch, arenas):
    return arenas("sparse", lambda: torch.empty(AR.ARENA_A, dtype=torch.uint8, device="cuda"))


def _view_a(arena, shift):
    return arena.as_strided((AR.S_A, N, AR.B_A), (AR.SS_A, AR.BS_A, 1), AR.BASE_A + shift)


def _fill_a(torch, arena, img, shift):
    """Twelve small copies: every block inside its two guard bands."""
    for (_, _, lo, hi), row in zip(AR.windows_a(shift), img):
        arena[lo:hi].copy_(torch.from_numpy(row.copy()))


def _read_a(arena, shift):
    return np.stack([arena[lo:hi].cpu().numpy() for _, _, lo, hi in AR.windows_a(shift)])


def _same_windows(got, want, what):
    if not np.array_equal(got, want):
        diff = np.argwhere(got != want)
        s, b = divmod(int(diff[0][0]), N)
        raise AssertionError((what, len(diff), "first at stripe", s, "block", b, "window byte", int(diff[0][1])))


def _stripes_a(pair):
    return AR.memo(("sparse", pair), lambda: AR.stripes_a(gf_plain.apply, CM, pair))


def _reference_a(lib):
    """[S_A][...] results of the damaged stripes of part A by the definition (heal2: the pair plan)."""
    def make():
        _, damaged = _stripes_a(lib == "heal2")
        return np.stack([_reference(lib, st) for st in damaged])
    return AR.memo(("sparse-reference", lib), make)


def _launches(shift):
    return 1 if shift else 2          # aligned: the vector kernel and the byte kernel of the 5-byte tail


@gpu
@pytest.mark.parametrize("shift", AR.SHIFTS_A, ids=SHIFT_IDS)
@by_form
def test_sparse_scrub(ecg, torch_cuda, arenas, libs, form, shift):
    torch, scrub = torch_cuda, libs["scrub"]
    arena = _sparse(torch, arenas)
    img = AR.image_a(_stripes_a(False)[1])
    _fill_a(torch, arena, img, shift)
    view = _view_a(arena, shift)
    want = _reference_a("scrub")
    assert (want[0] > 0).all() and want[1].tolist().count(0) == R - 1      # a data block: every row; a parity: its own
    name, _, call = form
    got = _counted(torch, scrub, lambda: call(scrub, view), _launches(shift), AR.S_A * AR.B_A * N)
    assert np.array_equal(got, want), (name, got, want)
    _same_windows(_read_a(arena, shift), img, "the scrub wrote to its inputs")


@gpu
@pytest.mark.parametrize("shift", AR.SHIFTS_A, ids=SHIFT_IDS)
@by_form
def test_sparse_locate(ecg, torch_cuda, arenas, libs, form, shift):
    torch, locate = torch_cuda, libs["locate"]
    arena = _sparse(torch, arenas)
    img = AR.image_a(_stripes_a(False)[1])
    _fill_a(torch, arena, img, shift)
    view = _view_a(arena, shift)
    sel = [1, 0, 1]                                       # read-only: a stripe may be named twice
    ids = _ints(torch, sel)
    want = _reference_a("locate")[sel]
    name, cols, call = form
    got = _counted(torch, locate, lambda: call(locate, view, stripe_ids=ids), _launches(shift), len(sel) * AR.B_A * N)
    assert np.array_equal(got, _in_form_order("locate", want, cols)), (name, got, want)
    _same_windows(_read_a(arena, shift), img, "the locate wrote to its inputs")


@gpu
@pytest.mark.parametrize("shift", AR.SHIFTS_A, ids=SHIFT_IDS)
@by_form
@pytest.mark.parametrize("lib", ["heal", "heal2"])
def test_sparse_heals(ecg, torch_cuda, arenas, libs, lib, form, shift):
    """ANY / ANY2 over the selection [1, 0]: the report, and all twelve windows equal to the definition's healed bytes
    with the guard bands intact.  Every case puts the damage back first."""
    torch, heal = torch_cuda, libs[lib]
    arena = _sparse(torch, arenas)
    clean, damaged = _stripes_a(lib == "heal2")
    healed = (HP.heal_stripes if lib == "heal" else P2.heal2_stripes)(H, damaged)[0]
    assert np.array_equal(healed, clean)
    img, healed_img = AR.image_a(damaged), AR.image_a(healed)
    view = _view_a(arena, shift)
    sel = [1, 0]
    ids = _ints(torch, sel)
    want = _reference_a(lib)[sel]
    assert (want[:, N] > 0).all() and not want[:, N + 1].any()
    name, cols, call = form
    _fill_a(torch, arena, img, shift)
    got = _counted(torch, heal, lambda: call(heal, view, stripe_ids=ids), _launches(shift), len(sel) * AR.B_A * N)
    assert np.array_equal(got, _in_form_order(lib, want, cols)), (name, got, want)
    _same_windows(_read_a(arena, shift), healed_img, (lib, name, "the windows after the heal"))


@gpu
@pytest.mark.parametrize("shift", AR.SHIFTS_A, ids=SHIFT_IDS)
def test_sparse_sums(ecg, torch_cuda, arenas, libs, shift):
    """blocks_batch and verify_batch with the block ids permuted and the selection [1, 0]: every sum against the
    definition, and the verify against the clean stripes' sums names the one damaged block of each stripe."""
    torch, sums = torch_cuda, libs["sum"]
    arena = _sparse(torch, arenas)
    clean, damaged = _stripes_a(False)
    img = AR.image_a(damaged)
    _fill_a(torch, arena, img, shift)
    view = _view_a(arena, shift)
    src, sel = list(AR.PERM), [1, 0]
    ids = _ints(torch, sel)
    want = CP.many(damaged)[sel][:, src]
    recorded = np.ascontiguousarray(CP.many(clean)[sel][:, src])
    vec = 0 if shift else 1

    c0 = sums.counters()
    got = sums.blocks_batch(src, view, stripe_ids=ids)
    torch.cuda.synchronize()
    c1 = sums.counters()
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
    assert c1["launches"] - c0["launches"] == vec + 1 and c1["bytes"] - c0["bytes"] == len(sel) * N * AR.B_A
    assert sums.last_launch()["path"] == (0 if vec else 1) and sums.last_launch()["blocks"] == len(sel) * N

    expected = torch.from_numpy(recorded.view(np.int32)).cuda()
    got, targets, bad = sums.verify_batch(src, view, expected, stripe_ids=ids)
    torch.cuda.synchronize()
    assert sums.counters()["launches"] - c1["launches"] == vec + 2          # and the compare
    assert sums.last_launch()["path"] == (0 if vec else 1)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
    assert [int(v) for v in targets.cpu()] == [src.index(AR.FIRST_A[s]) for s in sel]
    assert [int(v) for v in bad.cpu()] == [1, 1]
    _same_windows(_read_a(arena, shift), img, "the sums wrote to their inputs")


@gpu
@pytest.mark.parametrize("shift", AR.SHIFTS_A, ids=SHIFT_IDS)
def test_sparse_product(ecg, torch_cuda, arenas, shift):
    """One region-product call on the same arena: ecg.encode_batch from blocks 0, 1 into blocks 2..5 of both stripes,
    input and output strides above 2^31."""
    torch = torch_cuda
    arena = _sparse(torch, arenas)
    clean, _ = _stripes_a(False)
    stale = clean.copy()
    stale[:, K:] = 0x77
    _fill_a(torch, arena, AR.image_a(stale), shift)
    view = _view_a(arena, shift)
    l0 = ecg.traffic_counters()["launches"]
    ecg.encode_batch(K, R, FLAT, view[:, :K], view[:, K:])
    torch.cuda.synchronize()
    assert ecg.traffic_counters()["launches"] - l0 == _launches(shift)
    last = ecg.last_launch()
    assert last["kernel"] == (1 if shift else 0), last           # 0: the 16-byte-column kernel; 1: the byte kernel only
    _same_windows(_read_a(arena, shift), AR.image_a(clean), "the windows after the encode")


# ---------------------------------------------------------------------------------------------------------------------
# Part B: blocks of 2^31 - 1 bytes

def _big(torch, arenas):
    """[1][n][2^31] zeros; the stripes are its [..., :B_B].  Every case zeroes it again before it fills."""
    return arenas("big", lambda: torch.zeros((1, N, AR.PITCH_B), dtype=torch.uint8, device="cuda"))


def _nonzero_bytes(torch, full):
    """count_nonzero of the whole 12 GiB, 256 MiB at a time: taken at once its temporaries (a bool and an int64 per
    byte) would be several times the arena."""
    pieces = full.view(-1, 1 << 28)
    return int(sum(torch.count_nonzero(pieces[i]) for i in range(pieces.shape[0])))


def _damage_ranges(full):
    full.zero_()
    for lo, hi in AR.RANGES_B:
        full[0, 1, lo:hi] = AR.FILLS_B[1]


@gpu
@by_form
@pytest.mark.parametrize("lib", ["scrub", "locate"])
def test_big_read_only(ecg, torch_cuda, arenas, libs, lib, form):
    """Three damaged ranges of different lengths in block 1 -- from byte 0 into the sixth chunk, across 2^30, and the
    last 4099 bytes with the 15 of the byte path -- so that a chunk map that is no bijection changes the count; at the
    default geometry (2^20 workgroups) and with 2^20 columns per workgroup (column loops of 8192 iterations)."""
    torch, L = torch_cuda, libs[lib]
    full = _big(torch, arenas)
    _damage_ranges(full)
    view = full[:, :, :AR.B_B]
    want = AR.scaled_b(_reference(lib, AR.replica_b([1])), AR.RANGES_B_BYTES)[None]
    assert want.any()
    name, cols, call = form
    for cpw in (0, AR.COLS_PER_WG_B):
        with _with_options(ecg, {ecg.ECG_OPT_COLS_PER_WG: cpw}):
            got = _counted(torch, L, lambda: call(L, view), 2, AR.B_B * N)
            assert L.last_launch() == _expected_launch(ecg, 1, AR.B_B), (cpw, name, L.last_launch())
            assert np.array_equal(got, _in_form_order(lib, want, cols)), (cpw, name, got, want)
    assert _nonzero_bytes(torch, full) == AR.RANGES_B_BYTES


@gpu
@by_form
@pytest.mark.parametrize("lib,blocks", [("heal", (1,)), ("heal2", (1, 4))], ids=["heal", "heal2"])
def test_big_heals(ecg, torch_cuda, arenas, libs, lib, blocks, form):
    """Whole blocks filled with a constant (heal ANY: block 1; heal2 ANY2: blocks 1 and 4): every nonzero counter is
    2^31 - 1, positive in the int32 report, and the arena is all zero afterwards -- a skipped chunk stays nonzero, a
    chunk corrected twice turns nonzero again."""
    torch, L = torch_cuda, libs[lib]
    full = _big(torch, arenas)
    view = full[:, :, :AR.B_B]
    want = AR.scaled_b(_reference(lib, AR.replica_b(blocks)), AR.B_B)[None]
    assert want.max() == AR.B_B and np.count_nonzero(want) == 2 + (lib == "heal2") * 2
    name, cols, call = form
    full.zero_()
    for b in blocks:
        view[0, b].fill_(AR.FILLS_B[b])
    got = _counted(torch, L, lambda: call(L, view), 2, AR.B_B * N)
    assert L.last_launch() == _expected_launch(ecg, 1, AR.B_B), (name, L.last_launch())
    assert (got >= 0).all() and np.array_equal(got, _in_form_order(lib, want, cols)), (name, got, want)
    assert _nonzero_bytes(torch, full) == 0, name


@gpu
def test_big_sums(ecg, torch_cuda, arenas, libs):
    """The three damaged ranges in block 1, the other five blocks zero, auto segment: against ecg_sum.crc32c of the one
    block copied back and of 2^31 - 1 zero bytes (tests/test_sum_host.py pins that host function on the definition,
    which would walk these sizes for hours)."""
    torch, sums = torch_cuda, libs["sum"]
    full = _big(torch, arenas)
    _damage_ranges(full)
    view = full[:, :, :AR.B_B]
    sums.set_segment_bytes(0)
    c0 = sums.counters()
    got = sums.blocks_batch(list(range(N)), view)
    torch.cuda.synchronize()
    c1 = sums.counters()
    assert c1["launches"] - c0["launches"] == 2 and c1["bytes"] - c0["bytes"] == N * AR.B_B
    last = sums.last_launch()
    geo = dict(path=0, segment_bytes=AUTO_SEGMENT, segments_per_block=-(-AR.VEC_B // AUTO_SEGMENT), blocks=N)
    assert geo["segments_per_block"] == 8192 and {f: last[f] for f in geo} == geo, last
    block = view[0, 1].cpu().numpy()
    assert np.count_nonzero(block) == AR.RANGES_B_BYTES
    damaged = sums.crc32c(block)
    block[:] = 0
    zero = sums.crc32c(block)
    assert damaged != zero
    want = [zero, damaged, zero, zero, zero, zero]
    assert [int(v) for v in got.cpu().numpy().view(np.uint32)[0]] == want
    assert _nonzero_bytes(torch, full) == AR.RANGES_B_BYTES


# ---------------------------------------------------------------------------------------------------------------------
# Part C: 65 600 stripes of 53 bytes

GEOMETRIES_C = ((), AR.MAP_C)                            # the defaults (the auto map resolves to 1); map 2 in runs of 4
GEOMETRY_IDS_C = ["auto", "map2-G4"]


def _dense(torch, arenas):
    return arenas("dense", lambda: torch.zeros((AR.S_C + AR.EXTRA_C, N, AR.PITCH_C), dtype=torch.uint8, device="cuda"))


def _image_c():
    return AR.memo("dense-image", AR.image_c)


def _reference_c(lib):
    """{stripe id: result} of the damaged stripes by the definition."""
    return AR.memo(("dense-reference", lib), lambda: {s: _reference(lib, st) for s, st in AR.stripes_c().items()})


def _options_c(ecg, geometry):
    return dict(zip((ecg.ECG_OPT_GRID_MAP, ecg.ECG_OPT_MAP_GROUP), geometry))


def _same_arena(got, want, what):
    if not np.array_equal(got, want):
        diff = np.argwhere(got != want)
        raise AssertionError((what, len(diff), diff[:8].tolist()))


@gpu
@pytest.mark.parametrize("geometry", GEOMETRIES_C, ids=GEOMETRY_IDS_C)
@by_form
def test_dense_scrub(ecg, torch_cuda, arenas, libs, form, geometry):
    """The first 65 600 stripes in order: the whole (S, r) count tensor, zero rows included."""
    torch, scrub = torch_cuda, libs["scrub"]
    full = _dense(torch, arenas)
    img = _image_c()
    full.copy_(torch.from_numpy(img))
    view = full[:AR.S_C, :, :AR.B_C]
    want = AR.rows_c(np.arange(AR.S_C), _reference_c("scrub"), R)
    name, _, call = form
    with _with_options(ecg, _options_c(ecg, geometry)):
        got = _counted(torch, scrub, lambda: call(scrub, view), 2, AR.S_C * AR.B_C * N)
        assert scrub.last_launch() == _expected_launch(ecg, AR.S_C, AR.B_C), (name, scrub.last_launch())
    _same_arena(got, want, ("scrub counts", name))
    _same_arena(full.cpu().numpy(), img, "the scrub wrote to its inputs")


@gpu
@pytest.mark.parametrize("geometry", GEOMETRIES_C, ids=GEOMETRY_IDS_C)
@by_form
@pytest.mark.parametrize("lib", ["locate", "heal", "heal2"])
def test_dense_candidates(ecg, torch_cuda, arenas, libs, lib, form, geometry):
    """A permutation of all 65 600 stripes as the selection: the whole report against the definition run on the
    damaged stripes (every other row zero), and the whole arena -- untouched by the locate; after a heal the selected
    stripes clean and the damaged stripe outside the selection byte for byte as it was."""
    torch, L = torch_cuda, libs[lib]
    full = _dense(torch, arenas)
    img = _image_c()
    view = full[:, :, :AR.B_C]
    sel = AR.memo("dense-selection", AR.selection_c)
    ids = torch.from_numpy(sel.astype(np.int32)).cuda()
    want = AR.rows_c(sel, _reference_c(lib), N + EXTRA[lib])
    assert np.count_nonzero(want.any(axis=1)) == 39
    after = img
    if lib != "locate":
        after = np.zeros_like(img)
        after[AR.UNSELECTED_C] = img[AR.UNSELECTED_C]
    name, cols, call = form
    full.copy_(torch.from_numpy(img))
    with _with_options(ecg, _options_c(ecg, geometry)):
        got = _counted(torch, L, lambda: call(L, view, stripe_ids=ids), 2, AR.S_C * AR.B_C * N)
        assert L.last_launch() == _expected_launch(ecg, AR.S_C, AR.B_C), (name, L.last_launch())
    _same_arena(got, _in_form_order(lib, want, cols), (lib, "report", name))
    _same_arena(full.cpu().numpy(), after, (lib, "arena", name))


@gpu
def test_dense_sums(ecg, torch_cuda, arenas, libs):
    """All six sums of every selected stripe: the zero blocks against the bitwise definition, the damaged ones against
    crc32c_plain.many."""
    torch, sums = torch_cuda, libs["sum"]
    full = _dense(torch, arenas)
    img = _image_c()
    full.copy_(torch.from_numpy(img))
    view = full[:, :, :AR.B_C]
    sel = AR.memo("dense-selection", AR.selection_c)
    ids = torch.from_numpy(sel.astype(np.int32)).cuda()
    zero = CP.bitwise(bytes(AR.B_C))
    want = np.full((AR.S_C, N), zero, dtype=np.uint32)
    where = {int(s): p for p, s in enumerate(sel)}
    for sid, st in AR.stripes_c().items():
        if sid in where:
            want[where[sid]] = CP.many(st)
    assert np.count_nonzero((want != zero).any(axis=1)) == 39
    sums.set_segment_bytes(0)
    c0 = sums.counters()
    got = sums.blocks_batch(list(range(N)), view, stripe_ids=ids)
    torch.cuda.synchronize()
    c1 = sums.counters()
    assert c1["launches"] - c0["launches"] == 2 and c1["bytes"] - c0["bytes"] == AR.S_C * N * AR.B_C
    last = sums.last_launch()
    assert (last["path"], last["segments_per_block"], last["blocks"]) == (0, 1, AR.S_C * N), last
    _same_arena(got.cpu().numpy().view(np.uint32), want, "sums")
    _same_arena(full.cpu().numpy(), img, "the sums wrote to their inputs")
