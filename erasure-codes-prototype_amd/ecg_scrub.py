"""Python binding of libecg_scrub.so (include/ecg_scrub.h): stripe scrubbing, a read-only GF(2^8) parity check.

    counts[s][p] = number of byte positions x with  XOR_j H[p][j] * block_j[x] != 0

over HBM-resident stripes (torch uint8 CUDA tensors).  Every input byte is read once and nothing is written but
the counters, and those only where a check fails.  Counts come back as an int32 CUDA tensor of shape (S, r),
asynchronously on torch's current stream (or `stream`); `suspects` turns one stripe's counts into the blocks a
single corrupted block can be, which feed ErasureCode.generate_repair_plan.

There is no CPU fallback: if libecg_scrub.so is missing or has no GPU to run on, calls raise.
"""
from __future__ import annotations

import ctypes

import numpy as np

import _ecg_checklib as _checklib
import ecg
from _ecg_checklib import I, IP, LL, LLP, P, PP, UP, LAST_LAUNCH_FIELDS  # LAST_LAUNCH_FIELDS: re-exported
from ecg import _check, _ints, _ptrs, _stream, _strides, torch

LIB_PATH = _checklib.lib_path("ecg_scrub")

# Every symbol include/ecg_scrub.h declares (checked by tests/test_scrub_host.py).
EXPORTS = [
    "ecg_scrub_matrix_batch", "ecg_scrub_encode_batch", "ecg_scrub_ec_batch", "ecg_scrub_ec", "ecg_scrub_suspects",
    "ecg_scrub_counters", "ecg_scrub_last_launch",
]

_SIG = {
    "ecg_scrub_matrix_batch": ([I, I, IP, IP, P, LL, LL, LL, I, P, P], I),
    "ecg_scrub_encode_batch": ([I, I, IP, P, LL, LL, LL, I, P, P], I),
    "ecg_scrub_ec_batch": ([P, P, LL, LL, LL, I, P, P], I),
    "ecg_scrub_ec": ([P, PP, PP, I, P], I),
    "ecg_scrub_suspects": ([I, I, IP, UP, IP, I], I),
    "ecg_scrub_counters": ([LLP] * 2, I),
    "ecg_scrub_last_launch": ([IP, I], I),
}

_L = None


def lib():
    """Load libecg_scrub.so (after libecg.so, which it links against)."""
    global _L
    if _L is None:
        _L = _checklib.load(LIB_PATH, _SIG)
    return _L


def _counts(out, S, r, device):
    """The (S, r) int32 result tensor: `out` if given (checked), else a fresh one.  The call zeroes it."""
    return _checklib.result_tensor("scrub", out, (S, r), device, "(S, r)")


def matrix_batch(H, src_ids, stripes, out=None, stream=None):
    """H: r x k_in check matrix (nested or flat); src_ids: the k_in block indices its columns read; stripes:
    [S][*][B] uint8 CUDA tensor view (any strides).  Returns the (S, r) counts."""
    H = np.asarray(H, dtype=np.int64).reshape(-1, len(src_ids))
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    c = _counts(out, S, H.shape[0], stripes.device)
    _check(lib().ecg_scrub_matrix_batch(len(src_ids), H.shape[0], _ints(H.ravel()), _ints(src_ids),
                                        stripes.data_ptr(), ss, bs, B, S, c.data_ptr(), _stream(stream)),
           "scrub.matrix_batch")
    return c


def encode_batch(k, m, matrix, stripes, out=None, stream=None):
    """Check P = matrix * D over stripes [S][k+m][B] (data 0..k-1, coding k..k+m-1).  Returns the (S, m) counts."""
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    c = _counts(out, S, m, stripes.device)
    _check(lib().ecg_scrub_encode_batch(k, m, _ints(matrix), stripes.data_ptr(), ss, bs, B, S, c.data_ptr(),
                                        _stream(stream)), "scrub.encode_batch")
    return c


def ec_batch(code, stripes, out=None, stream=None):
    """The class's own check (ErasureCode.check_matrix) over stripes [S][k+m][B].  Returns the (S, m) counts."""
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    c = _counts(out, S, code.m, stripes.device)
    _check(ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, _stream(stream)), "set_memory")
    _check(lib().ecg_scrub_ec_batch(code._h, stripes.data_ptr(), ss, bs, B, S, c.data_ptr(), _stream(stream)),
           "scrub.ec_batch")
    return c


def ec(code, data_ptrs, coding_ptrs, block_size, out=None, stream=None):
    """One stripe through its block pointers (lists of uint8 CUDA tensors), on the handle's stream.  Returns the
    (1, m) counts."""
    code._bind(list(data_ptrs) + list(coding_ptrs), stream)
    c = _counts(out, 1, code.m, data_ptrs[0].device)
    _check(lib().ecg_scrub_ec(code._h, _ptrs(data_ptrs), _ptrs(coding_ptrs), block_size, c.data_ptr()), "scrub.ec")
    return c


def suspects(H, counts):
    """The blocks a single corrupted block can be, from one stripe's counts (host values: a list, a numpy array
    or a tensor row): those whose column support in H equals the set of rows with a nonzero count.  [] if the
    stripe is clean or no single block explains the rows."""
    if torch is not None and isinstance(counts, torch.Tensor):
        counts = counts.detach().cpu().numpy()
    cnt = [int(v) & 0xFFFFFFFF for v in np.asarray(counts).reshape(-1)]
    r = len(cnt)
    H = np.asarray(H, dtype=np.int64).reshape(r, -1)
    n = H.shape[1]
    ids = (ctypes.c_int * max(1, n))()
    got = _check(lib().ecg_scrub_suspects(r, n, _ints(H.ravel()), (ctypes.c_uint * max(1, r))(*cnt), ids, n),
                 "scrub.suspects")
    return list(ids)[:got]


def counters():
    """Process-wide {launches, bytes}: scrub kernels launched and the bytes they read as planned (S * B * k_in per
    row tile)."""
    return _checklib.counters(lib(), "scrub")


def last_launch():
    """Geometry of the process's most recent vector-path scrub launch, as placed in the launch descriptor after the
    fallbacks (include/ecg_scrub.h ecg_scrub_last_launch): {grid_map, map_group, cols_per_wg, wg_per_stripe, S,
    rtiles}, all zero before the first.  Byte-kernel launches do not change it."""
    return _checklib.last_launch(lib(), "scrub")
