"""Python binding of libecg_heal.so (include/ecg_heal.h): in-place correction, the step after a scrub and a locate.

For a check matrix H (r x n, r <= 8, n <= 128) and the selected stripes, every bad byte position (nonzero syndrome
s[x] = H * v[x]) that a candidate block b explains (s[x] = e * H[:, b], e != 0) is corrected in place: byte x of
block b becomes v_b[x] ^ e.  The candidates of a stripe are the one block `targets` names for it (TARGET mode; a value
outside [0, n) names none) or every block (`targets=None`, ANY mode, refused when two columns of H are proportional).
Per stripe

    report[b]     = positions corrected in block b,                                  b < n
    report[n]     = bad positions
    report[n + 1] = bad positions left untouched

comes back as an int32 CUDA tensor of shape (S_sel, n + 2), asynchronously on torch's current stream (or `stream`);
ecg_locate.verdict reads a row unchanged.  The stripes (torch uint8 CUDA tensors) are WRITTEN, only where a byte is
corrected; the stripe ids of one call must be distinct.  include/ecg_heal.h states the miscorrection limit.

There is no CPU fallback: if libecg_heal.so is missing or has no GPU to run on, calls raise.
"""
from __future__ import annotations

import _ecg_checklib as _checklib
from _ecg_checklib import I, IP, LL, LLP, P, PP, LAST_LAUNCH_FIELDS  # LAST_LAUNCH_FIELDS: re-exported
from ecg import torch

LIB_PATH = _checklib.lib_path("ecg_heal")

# Every symbol include/ecg_heal.h declares (checked by tests/test_heal_host.py).
EXPORTS = [
    "ecg_heal_matrix_batch", "ecg_heal_encode_batch", "ecg_heal_ec_batch", "ecg_heal_ec", "ecg_heal_counters",
    "ecg_heal_last_launch",
]

ANY = -1  # ecg_heal_ec's target for ANY mode

_SIG = {
    "ecg_heal_matrix_batch": ([I, I, IP, IP, P, LL, LL, LL, P, P, I, P, P], I),
    "ecg_heal_encode_batch": ([I, I, IP, P, LL, LL, LL, P, P, I, P, P], I),
    "ecg_heal_ec_batch": ([P, P, LL, LL, LL, P, P, I, P, P], I),
    "ecg_heal_ec": ([P, PP, PP, I, I, P], I),
    "ecg_heal_counters": ([LLP] * 2, I),
    "ecg_heal_last_launch": ([IP, I], I),
}

_L = None


def lib():
    """Load libecg_heal.so (after libecg.so, which it links against)."""
    global _L
    if _L is None:
        _L = _checklib.load(LIB_PATH, _SIG)
    return _L


def matrix_batch(H, src_ids, stripes, stripe_ids=None, targets=None, out=None, stream=None):
    """H: r x n check matrix (nested or flat); src_ids: the n block indices its columns stand for; stripes: [S][*][B]
    uint8 CUDA tensor view (any strides), corrected in place.  Returns the (S_sel, n + 2) report; report[:, j], and a
    target j, are block src_ids[j]."""
    return _checklib.correct_matrix_batch(lib, "heal", 2, H, src_ids, stripes, stripe_ids, targets, out, stream)


def encode_batch(k, m, matrix, stripes, stripe_ids=None, targets=None, out=None, stream=None):
    """H = [matrix | I] over stripes [S][k+m][B] (data 0..k-1, coding k..k+m-1), corrected in place.  Returns the
    (S_sel, k+m+2) report."""
    return _checklib.correct_encode_batch(lib, "heal", 2, k, m, matrix, stripes, stripe_ids, targets, out, stream)


def ec_batch(code, stripes, stripe_ids=None, targets=None, out=None, stream=None):
    """The class's own check (ErasureCode.check_matrix) over stripes [S][k+m][B], corrected in place.  Returns the
    (S_sel, k+m+2) report."""
    return _checklib.correct_ec_batch(lib, "heal", 2, code, stripes, stripe_ids, targets, out, stream)


def ec(code, data_ptrs, coding_ptrs, block_size, target=ANY, out=None, stream=None):
    """One stripe through its block pointers (lists of uint8 CUDA tensors), on the handle's stream; target: a block
    id (a host int), or ANY.  Returns the (1, k+m+2) report."""
    return _checklib.correct_ec(lib, "heal", 2, code, data_ptrs, coding_ptrs, block_size, target, out, stream)


def targets_from_votes(votes):
    """The locate's votes ((S_sel, n + 2) tensor) -> the int32 CUDA tensor of targets: the block ecg_locate_verdict
    names for the row, -1 where it names no single block (CLEAN, AMBIGUOUS, MULTIPLE).  Stays on the device."""
    n = votes.shape[1] - 2
    bad = votes[:, n:n + 1]
    full = (votes[:, :n] == bad) & (votes[:, :n] != 0)      # the blocks that explain every bad position
    one = (full.sum(dim=1) == 1) & (votes[:, n + 1] == 0) & (bad[:, 0] != 0)
    who = full.to(torch.int32).argmax(dim=1).to(torch.int32)
    return torch.where(one, who, torch.full_like(who, -1)).contiguous()


def counters():
    """Process-wide {launches, bytes}: heal kernels launched and the bytes they read as planned (S_sel * B * n)."""
    return _checklib.counters(lib(), "heal")


def last_launch():
    """Geometry of the process's most recent vector-path heal launch, as placed in the launch descriptor after the
    fallbacks (include/ecg_heal.h ecg_heal_last_launch): {grid_map, map_group, cols_per_wg, wg_per_stripe, S,
    rtiles}, all zero before the first.  Byte-kernel launches do not change it."""
    return _checklib.last_launch(lib(), "heal")
