"""Every region-product kernel instantiation of libecg.so, launched through a public call and compared byte for
byte with the field's definition (tests/gf_plain.py -- not the oracle).

tests/gf_kernel_cases.py lists the cases: one public call each, with the instantiations its launches must land
on.  A case snapshots ecg.launch_histogram() and the launch counter, makes its call, and asserts that the
histogram moved on exactly the declared keys and that those account for every launch counted; then it compares
the whole output arena -- the named blocks, the 64-byte bands of 0xC3 around every block, the blocks the op does
not name (0x3C) -- with the expected image, and the input arena with what was uploaded (tests/gf_arena.py).  So a
store past a block's end, a dead lane or a dead row of a short last tile that stores, and a call routed to another
kernel than the one declared all fail here.  ecg.last_launch() must report the mode, the row tiles and the kernel
class the case declares.  The last test (no GPU) checks that the declared keys cover the enumeration
tests/test_kernel_enumeration.py pins against the code object.
"""
import numpy as np
import pytest

import gf_arena as A
import gf_kernel_cases as C
import gf_plain

GUARD = A.GUARD
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return torch


def run_case(ecg, torch, c, M=None, fill_in=None, describe=None):
    """One case: set its options, make its call, check the histogram, the outputs, the bands and the inputs."""
    M = C.matrix(c) if M is None else np.asarray(M, dtype=np.int64)
    rows, keys, report = C.live_rows(c, M), C.expected_keys(c, M), C.expected_report(c, M)
    k, m, B = c.k, c.m, c.B
    pos = {"strided": (0, 1, 2), "ptrs": (0, 1, 3)}.get(c.form, (0,))  # ptrs: no single stripe stride
    NS, n_in, n_out = pos[-1] + 1, k + 1, m + 2
    rng = np.random.default_rng(c.seed ^ 0x5EED)
    in_img = A.blank(NS, n_in, B)
    in_img[:, :, GUARD:GUARD + B] = rng.integers(0, 256, (NS, n_in, B), dtype=np.uint8) if fill_in is None else fill_in
    out_img = A.blank(NS, n_out, B)
    src, dst = [k - j for j in range(k)], [p + 1 for p in range(m)]  # slot 0 (and m + 1 of the outputs) unnamed
    want = out_img.copy()
    for s in pos:
        res = gf_plain.apply(M[rows], in_img[s, src, GUARD:GUARD + B])
        for i, p in enumerate(rows):
            want[s, dst[p], GUARD:GUARD + B] = res[i]
    saved = [ecg.get_option(o) for o in range(ecg.ECG_OPT_COUNT)]
    try:
        ecg.set_option(ecg.ECG_OPT_NT, c.nt)
        ecg.set_option(ecg.ECG_OPT_COLS_PER_WG, c.cpw)
        ecg.set_option(ecg.ECG_OPT_LAT_DWORD_BYTES, c.lat)
        flat_m = [int(v) for v in M.reshape(-1)]
        if c.form == "host":
            h_in, got = in_img.copy(), out_img.copy()
            h0, l0 = ecg.launch_histogram(), ecg.traffic_counters()["launches"]
            ecg.jerasure_matrix_encode(k, m, flat_m, [h_in[0, src[j], GUARD:GUARD + B] for j in range(k)],
                                       [got[0, dst[p], GUARD:GUARD + B] for p in range(m)], B)
            in_after = h_in
        else:
            d_in, d_out = A.to_dev(torch, in_img, c.shift), A.to_dev(torch, out_img, c.shift)
            torch.cuda.synchronize()
            h0, l0 = ecg.launch_histogram(), ecg.traffic_counters()["launches"]
            if c.form == "strided":
                ecg.matrix_apply_batch(M, src, dst, d_in[:, :, GUARD:GUARD + B], d_out[:, :, GUARD:GUARD + B])
            else:
                def call(s):
                    ecg.dev_matrix_encode(k, m, flat_m, [d_in[s, src[j], GUARD:GUARD + B] for j in range(k)],
                                          [d_out[s, dst[p], GUARD:GUARD + B] for p in range(m)], B)
                if c.form == "ptrs":
                    with ecg.batch():
                        for s in pos:
                            call(s)
                else:
                    call(0)
            torch.cuda.synchronize()
            got, in_after = d_out.cpu().numpy(), d_in.cpu().numpy()
        h1, l1, last = ecg.launch_histogram(), ecg.traffic_counters()["launches"], ecg.last_launch()
    finally:
        for o, v in enumerate(saved):
            ecg.set_option(o, v)
    delta = {key: h1.get(key, 0) - h0.get(key, 0) for key in set(h0) | set(h1)}
    delta = {key: n for key, n in delta.items() if n}
    assert delta == keys, (c, "launched", delta, "declared", keys)
    assert l1 - l0 == sum(keys.values()), (c, l1 - l0, keys)
    assert {f: last[f] for f in report} == report, (c, "reported", last, "declared", report)
    assert np.array_equal(in_after, in_img), (c, "an input arena changed")

    def name(s, slot, o):
        msg = describe(M, dst.index(slot), o, in_img[s, src, GUARD:GUARD + B]) if describe else ""
        return f"(output row {dst.index(slot)}) {msg}"
    A.assert_same(got, want, B, lambda s, slot: slot in dst, c, name)
    return keys


@gpu
@pytest.mark.parametrize("path,binary,m", C.vec_groups(),
                         ids=[f"{p}-{'bin' if b else 'gen'}-m{m}" for p, b, m in C.vec_groups()])
def test_vec_and_byte_kernels(ecg, torch_cuda, path, binary, m):
    """gf_vec_kernel and gf_byte_kernel of one (path, flavour, tile): every k branch at NT 3, the other NT
    policies, a byte-only block, an unaligned block."""
    for c in C.vec_group(path, binary, m):
        run_case(ecg, torch_cuda, c)


@gpu
@pytest.mark.parametrize("binary,m", C.lat_groups(), ids=[f"{'bin' if b else 'gen'}-m{m}" for b, m in C.lat_groups()])
def test_latency_kernels(ecg, torch_cuda, binary, m):
    """gf_lat_dword_kernel of one (flavour, MT): both edges of every input-count bucket, EAGER and not."""
    for c in C.lat_group(binary, m):
        run_case(ecg, torch_cuda, c)


@gpu
def test_cols_per_wg(ecg, torch_cuda):
    for c in C.cols_per_wg_cases():
        run_case(ecg, torch_cuda, c)


@gpu
def test_host_tier_calls(ecg, torch_cuda):
    for c in C.host_cases():
        run_case(ecg, torch_cuda, c)


# ---- exhaustive field pass: every coefficient times every byte value at every byte position of a 16-byte column

FIELD_PATHS = {"vec16": ("strided", 0), "byte": ("strided", 1), "lat": ("dev", 0)}


def _field_input():
    x = np.zeros(C.FIELD_B, np.uint8)
    for col in range(256):
        for b in range(16):
            x[16 * col + b] = (col + 17 * b) & 0xFF
    assert all(len(set(x[b::16])) == 256 for b in range(16))  # every value at every byte position
    return x


def _name_product(M, p, o, inputs):
    return f"= coefficient {int(M[p, 0])} times value {int(inputs[0, o])} at lane byte {o % 16} (column {o // 16})"


@gpu
@pytest.mark.parametrize("path", sorted(FIELD_PATHS))
def test_exhaustive_field_pass(ecg, torch_cuda, path):
    """All 256 x 256 products on one multiply path: the SGPR v_perm tables of the 16-byte kernel, the byte kernel,
    the LDS tables of the latency kernel.  1 -> 8 ops, so every output byte is one product c * x."""
    form, shift = FIELD_PATHS[path]
    x = _field_input()
    seen = set()
    for i in range(32):
        c = C.Case(form, 0, 8, 1, C.FIELD_B, 3, 0, C.LAT_DWORD_DEFAULT, shift, 4000 + i)
        M = [[8 * i + r] for r in range(8)]
        seen |= set(run_case(ecg, torch_cuda, c, M=M, fill_in=x, describe=_name_product))
    # every coefficient in one 16 -> 16 op: two GENERAL row tiles
    c = C.Case(form, 0, 16, 16, C.FIELD_B, 3, 0, C.LAT_DWORD_DEFAULT, shift, 4100)
    seen |= set(run_case(ecg, torch_cuda, c, M=[[16 * p + j for j in range(16)] for p in range(16)]))
    assert seen <= C.FIELD_PASS_KEYS, seen - C.FIELD_PASS_KEYS
    if path == "lat":
        assert ("lat", 0, 8, 4, 1) in seen
    else:
        assert seen == {("byte" if shift else "vec", C.MODE_STRIDED, 0) + ((8,) if shift else (3, 8))}


def test_declared_cases_cover_every_instantiation():
    """No GPU work: the union of the keys the cases above declare (and verify when they run) is a superset of
    the enumeration, apart from what UNREACHABLE lists with its reason."""
    declared = C.declared_keys()
    missing = C.enumeration() - declared - set(C.UNREACHABLE)
    assert not missing, sorted(missing)[:16]
    assert not set(C.UNREACHABLE) & declared, "a listed key is reached after all"
