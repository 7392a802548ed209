"""Python binding of libecg_locate.so (include/ecg_locate.h): corruption localisation, the step after a scrub.

For a check matrix H (r x n, r <= 8, n <= 128) and the selected stripes, per stripe

    votes[b]     = byte positions whose syndrome s[x] = H * v[x] is a nonzero multiple of column b of H
                   (the positions that damage to block b alone explains),            b < n
    votes[n]     = byte positions with a nonzero syndrome (bad positions)
    votes[n + 1] = bad positions that no single block explains

over HBM-resident stripes (torch uint8 CUDA tensors), read once and never written.  Votes come back as an int32
CUDA tensor of shape (S_sel, n + 2), asynchronously on torch's current stream (or `stream`); `dirty` turns a
scrub's counts into the stripe selection, `verdict` one stripe's votes into the damaged block.  The verdict assumes
at most one damaged block per byte position (include/ecg_locate.h states the miscorrection limit).

There is no CPU fallback: if libecg_locate.so is missing or has no GPU to run on, calls raise.
"""
from __future__ import annotations

import ctypes

import numpy as np

import _ecg_checklib as _checklib
import ecg
from _ecg_checklib import I, IP, LL, LLP, P, PP, UP, LAST_LAUNCH_FIELDS  # LAST_LAUNCH_FIELDS: re-exported
from ecg import EcgError, _check, _ints, _ptrs, _stream, _strides, torch

LIB_PATH = _checklib.lib_path("ecg_locate")

# Every symbol include/ecg_locate.h declares (checked by tests/test_locate_host.py).
EXPORTS = [
    "ecg_locate_matrix_batch", "ecg_locate_encode_batch", "ecg_locate_ec_batch", "ecg_locate_ec",
    "ecg_locate_verdict", "ecg_locate_counters", "ecg_locate_last_launch",
]

# ecg_locate_verdict statuses (a value >= 0 is a block id)
CLEAN, AMBIGUOUS, MULTIPLE = -100, -101, -102

_SIG = {
    "ecg_locate_matrix_batch": ([I, I, IP, IP, P, LL, LL, LL, P, I, P, P], I),
    "ecg_locate_encode_batch": ([I, I, IP, P, LL, LL, LL, P, I, P, P], I),
    "ecg_locate_ec_batch": ([P, P, LL, LL, LL, P, I, P, P], I),
    "ecg_locate_ec": ([P, PP, PP, I, P], I),
    "ecg_locate_verdict": ([I, UP, IP, I, IP], I),
    "ecg_locate_counters": ([LLP] * 2, I),
    "ecg_locate_last_launch": ([IP, I], I),
}

_L = None


def lib():
    """Load libecg_locate.so (after libecg.so, which it links against)."""
    global _L
    if _L is None:
        _L = _checklib.load(LIB_PATH, _SIG)
    return _L


def _selection(stripe_ids, S):
    """(device pointer or None, S_sel) of a stripe selection: None = all S stripes in order."""
    ids, _, S_sel = _checklib.selection("locate", stripe_ids, None, S)
    return ids, S_sel


def _votes(out, S_sel, n, device):
    """The (S_sel, n + 2) int32 result tensor: `out` if given (checked), else a fresh one.  The call zeroes it."""
    return _checklib.result_tensor("locate", out, (S_sel, n + 2), device, "(S_sel, n + 2)")


def matrix_batch(H, src_ids, stripes, stripe_ids=None, out=None, stream=None):
    """H: r x n check matrix (nested or flat); src_ids: the n block indices its columns read; stripes: [S][*][B]
    uint8 CUDA tensor view (any strides).  Returns the (S_sel, n + 2) votes; votes[:, j] is block src_ids[j]."""
    n = len(src_ids)
    H = np.asarray(H, dtype=np.int64).reshape(-1, n)
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    ids, S_sel = _selection(stripe_ids, S)
    v = _votes(out, S_sel, n, stripes.device)
    _check(lib().ecg_locate_matrix_batch(n, H.shape[0], _ints(H.ravel()), _ints(src_ids), stripes.data_ptr(), ss, bs,
                                         B, ids, S_sel, v.data_ptr(), _stream(stream)), "locate.matrix_batch")
    return v


def encode_batch(k, m, matrix, stripes, stripe_ids=None, out=None, stream=None):
    """H = [matrix | I] over stripes [S][k+m][B] (data 0..k-1, coding k..k+m-1).  Returns the (S_sel, k+m+2) votes."""
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    ids, S_sel = _selection(stripe_ids, S)
    v = _votes(out, S_sel, k + m, stripes.device)
    _check(lib().ecg_locate_encode_batch(k, m, _ints(matrix), stripes.data_ptr(), ss, bs, B, ids, S_sel, v.data_ptr(),
                                         _stream(stream)), "locate.encode_batch")
    return v


def ec_batch(code, stripes, stripe_ids=None, out=None, stream=None):
    """The class's own check (ErasureCode.check_matrix) over stripes [S][k+m][B].  Returns the (S_sel, k+m+2) votes."""
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    ids, S_sel = _selection(stripe_ids, S)
    v = _votes(out, S_sel, code.k + code.m, stripes.device)
    _check(ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, _stream(stream)), "set_memory")
    _check(lib().ecg_locate_ec_batch(code._h, stripes.data_ptr(), ss, bs, B, ids, S_sel, v.data_ptr(),
                                     _stream(stream)), "locate.ec_batch")
    return v


def ec(code, data_ptrs, coding_ptrs, block_size, out=None, stream=None):
    """One stripe through its block pointers (lists of uint8 CUDA tensors), on the handle's stream.  Returns the
    (1, k+m+2) votes."""
    code._bind(list(data_ptrs) + list(coding_ptrs), stream)
    v = _votes(out, 1, code.k + code.m, data_ptrs[0].device)
    _check(lib().ecg_locate_ec(code._h, _ptrs(data_ptrs), _ptrs(coding_ptrs), block_size, v.data_ptr()), "locate.ec")
    return v


def dirty(counts):
    """The stripe selection of a scrub: the int32 CUDA tensor of the stripe indices (ascending) whose scrub counts
    (ecg_scrub's (S, r) tensor) have any nonzero.  Synchronises: its length is a host value."""
    return torch.nonzero((counts != 0).any(dim=1)).reshape(-1).to(torch.int32).contiguous()


def verdict(votes_row):
    """(status_or_block, ids) of one stripe's votes (host values: a list, a numpy array or a tensor row of n + 2).
    status_or_block: CLEAN, the block id that explains every bad position, AMBIGUOUS (several do: proportional
    columns) or MULTIPLE; ids: every block with a vote, ascending."""
    if torch is not None and isinstance(votes_row, torch.Tensor):
        votes_row = votes_row.detach().cpu().numpy()
    v = [int(x) & 0xFFFFFFFF for x in np.asarray(votes_row).reshape(-1)]
    n = len(v) - 2
    ids = (ctypes.c_int * max(1, n))()
    got = ctypes.c_int(0)
    rc = lib().ecg_locate_verdict(n, (ctypes.c_uint * max(1, len(v)))(*v), ids, max(0, n), ctypes.byref(got))
    if rc == ecg.ECG_EINVAL:
        raise EcgError(rc, "locate.verdict")
    return rc, list(ids)[:got.value]


def counters():
    """Process-wide {launches, bytes}: locate kernels launched and the bytes they read as planned (S_sel * B * n)."""
    return _checklib.counters(lib(), "locate")


def last_launch():
    """Geometry of the process's most recent vector-path locate launch, as placed in the launch descriptor after the
    fallbacks (include/ecg_locate.h ecg_locate_last_launch): {grid_map, map_group, cols_per_wg, wg_per_stripe, S,
    rtiles}, all zero before the first.  Byte-kernel launches do not change it."""
    return _checklib.last_launch(lib(), "locate")
