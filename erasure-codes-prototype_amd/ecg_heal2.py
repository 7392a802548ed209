"""Python binding of libecg_heal2.so (include/ecg_heal2.h): two-block correction, the heal that goes on where two
blocks are damaged at one byte position.

For a check matrix H (r x n, 3 <= r <= 8, 2 <= n <= 32) and the selected stripes, every bad byte position (nonzero
syndrome s[x] = H * v[x]) that a set A of one or two blocks explains (s[x] = XOR e_a * H[:, a], every e_a != 0) is
corrected in place: byte x of every block a in A becomes v_a[x] ^ e_a.  The admissible sets of a stripe are every
single block and every pair (`targets=None`, ANY2: refused unless every 4 columns of H are independent), or every
single block and every pair that holds the block `targets` names for the stripe (TARGET2: refused unless every 3
columns are independent; a value outside [0, n) admits nothing).  Per stripe

    report[b]     = positions corrected in block b (a pair counts in both of its blocks),   b < n
    report[n]     = bad positions
    report[n + 1] = bad positions left untouched
    report[n + 2] = positions corrected as a pair

comes back as an int32 CUDA tensor of shape (S_sel, n + 3), asynchronously on torch's current stream (or `stream`).
The stripes (torch uint8 CUDA tensors) are WRITTEN, only where a byte is corrected; the stripe ids of one call must be
distinct.  include/ecg_heal2.h states the miscorrection limit.

There is no CPU fallback: if libecg_heal2.so is missing or has no GPU to run on, calls raise.
"""
from __future__ import annotations

import _ecg_checklib as _checklib
from _ecg_checklib import I, IP, LL, LLP, P, PP, LAST_LAUNCH_FIELDS  # LAST_LAUNCH_FIELDS: re-exported

LIB_PATH = _checklib.lib_path("ecg_heal2")

# Every symbol include/ecg_heal2.h declares (checked by tests/test_heal2_host.py).
EXPORTS = [
    "ecg_heal2_matrix_batch", "ecg_heal2_encode_batch", "ecg_heal2_ec_batch", "ecg_heal2_ec", "ecg_heal2_counters",
    "ecg_heal2_last_launch",
]

ANY = -1  # ecg_heal2_ec's target for ANY2

_SIG = {
    "ecg_heal2_matrix_batch": ([I, I, IP, IP, P, LL, LL, LL, P, P, I, P, P], I),
    "ecg_heal2_encode_batch": ([I, I, IP, P, LL, LL, LL, P, P, I, P, P], I),
    "ecg_heal2_ec_batch": ([P, P, LL, LL, LL, P, P, I, P, P], I),
    "ecg_heal2_ec": ([P, PP, PP, I, I, P], I),
    "ecg_heal2_counters": ([LLP] * 2, I),
    "ecg_heal2_last_launch": ([IP, I], I),
}

_L = None


def lib():
    """Load libecg_heal2.so (after libecg.so, which it links against)."""
    global _L
    if _L is None:
        _L = _checklib.load(LIB_PATH, _SIG)
    return _L


def matrix_batch(H, src_ids, stripes, stripe_ids=None, targets=None, out=None, stream=None):
    """H: r x n check matrix (nested or flat); src_ids: the n block indices its columns stand for; stripes: [S][*][B]
    uint8 CUDA tensor view (any strides), corrected in place.  Returns the (S_sel, n + 3) report; report[:, j], and a
    target j, are block src_ids[j]."""
    return _checklib.correct_matrix_batch(lib, "heal2", 3, H, src_ids, stripes, stripe_ids, targets, out, stream)


def encode_batch(k, m, matrix, stripes, stripe_ids=None, targets=None, out=None, stream=None):
    """H = [matrix | I] over stripes [S][k+m][B] (data 0..k-1, coding k..k+m-1), corrected in place.  Returns the
    (S_sel, k+m+3) report."""
    return _checklib.correct_encode_batch(lib, "heal2", 3, k, m, matrix, stripes, stripe_ids, targets, out, stream)


def ec_batch(code, stripes, stripe_ids=None, targets=None, out=None, stream=None):
    """The class's own check (ErasureCode.check_matrix) over stripes [S][k+m][B], corrected in place.  Returns the
    (S_sel, k+m+3) report."""
    return _checklib.correct_ec_batch(lib, "heal2", 3, code, stripes, stripe_ids, targets, out, stream)


def ec(code, data_ptrs, coding_ptrs, block_size, target=ANY, out=None, stream=None):
    """One stripe through its block pointers (lists of uint8 CUDA tensors), on the handle's stream; target: a block
    id (a host int), or ANY.  Returns the (1, k+m+3) report."""
    return _checklib.correct_ec(lib, "heal2", 3, code, data_ptrs, coding_ptrs, block_size, target, out, stream)


def counters():
    """Process-wide {launches, bytes}: heal2 kernels launched and the bytes they read as planned (S_sel * B * n)."""
    return _checklib.counters(lib(), "heal2")


def last_launch():
    """Geometry of the process's most recent vector-path heal2 launch, as placed in the launch descriptor after the
    fallbacks (include/ecg_heal2.h ecg_heal2_last_launch): {grid_map, map_group, cols_per_wg, wg_per_stripe, S,
    rtiles}, all zero before the first.  Byte-kernel launches do not change it."""
    return _checklib.last_launch(lib(), "heal2")
