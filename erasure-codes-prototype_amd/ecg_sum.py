"""Python binding of libecg_sum.so (include/ecg_sum.h): block checksums, CRC-32C of every stored block.

    sums[i][j] = crc32c(block src_ids[j] of stripe stripe_ids[i])

over HBM-resident stripes (torch uint8 CUDA tensors).  Every byte is read once and nothing is written but the
outputs.  Sums come back as an int32 CUDA tensor of shape (S_sel, n) holding the 32-bit values (`& 0xFFFFFFFF` on the
host), asynchronously on torch's current stream (or `stream`).  `verify_batch` compares them with recorded sums and
returns (sums, targets, bad): `targets` is the int32 vector that ecg_heal's TARGET and ecg_heal2's TARGET2 forms take.

There is no CPU fallback for the device calls: if libecg_sum.so is missing or has no GPU to run on, they raise.
`crc32c` and `combine` are host functions over host bytes.
"""
from __future__ import annotations

import ctypes

import numpy as np

import _ecg_checklib as _checklib
import ecg
from _ecg_checklib import I, IP, LL, LLP, P, PP
from ecg import EcgError, _check, _ints, _ptrs, _stream, _strides, torch

LIB_PATH = _checklib.lib_path("ecg_sum")
U = ctypes.c_uint

# Every symbol include/ecg_sum.h declares (checked by tests/test_sum_host.py).
EXPORTS = [
    "ecg_sum_blocks_batch", "ecg_sum_verify_batch", "ecg_sum_ec_batch", "ecg_sum_verify_ec_batch", "ecg_sum_ec",
    "ecg_sum_crc32c", "ecg_sum_combine", "ecg_sum_counters", "ecg_sum_last_launch", "ecg_sum_set_segment_bytes",
    "ecg_sum_set_table_scheme",
]

_SIG = {
    "ecg_sum_blocks_batch": ([I, IP, P, LL, LL, LL, P, I, P, P], I),
    "ecg_sum_verify_batch": ([I, IP, P, LL, LL, LL, P, I, P, P, P, P, P], I),
    "ecg_sum_ec_batch": ([P, P, LL, LL, LL, P, I, P, P], I),
    "ecg_sum_verify_ec_batch": ([P, P, LL, LL, LL, P, I, P, P, P, P, P], I),
    "ecg_sum_ec": ([P, PP, PP, I, P], I),
    "ecg_sum_crc32c": ([P, LL], U),
    "ecg_sum_combine": ([U, U, LL], U),
    "ecg_sum_counters": ([LLP] * 2, I),
    "ecg_sum_last_launch": ([IP, I], I),
    "ecg_sum_set_segment_bytes": ([LL], I),
    "ecg_sum_set_table_scheme": ([I], I),
}

# The fields of ecg_sum_last_launch, in order.
LAST_LAUNCH_FIELDS = ("path", "segment_bytes", "segments_per_block", "blocks", "table_scheme")
PATH_VECTOR, PATH_BYTE = 0, 1

_L = None


def lib():
    """Load libecg_sum.so (after libecg.so, which it links against)."""
    global _L
    if _L is None:
        _L = _checklib.load(LIB_PATH, _SIG)
    return _L


def _selection(stripe_ids, S):
    return (None, S) if stripe_ids is None else _checklib.int32_vector("sum", stripe_ids, "stripe_ids")


def _sums(out, S_sel, n, device):
    return _checklib.result_tensor("sum", out, (S_sel, n), device, "(S_sel, n)")


def _expected(expected, S_sel, n):
    if (tuple(expected.shape) != (S_sel, n) or expected.dtype != torch.int32 or not expected.is_cuda
            or not expected.is_contiguous()):
        raise EcgError(ecg.ECG_EINVAL, "sum: expected must be a contiguous int32 CUDA tensor of shape (S_sel, n)")
    return expected.data_ptr()


def _verdicts(S_sel, device):
    return (torch.empty((S_sel,), dtype=torch.int32, device=device),
            torch.empty((S_sel,), dtype=torch.int32, device=device))


def blocks_batch(src_ids, stripes, stripe_ids=None, out=None, stream=None):
    """src_ids: the n block indices to sum; stripes: [S][*][B] uint8 CUDA tensor view (any strides); stripe_ids: int32
    CUDA vector of the stripes to sum (None: all, in order; duplicates allowed).  Returns the (S_sel, n) sums."""
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    ids, S_sel = _selection(stripe_ids, S)
    v = _sums(out, S_sel, len(src_ids), stripes.device)
    _check(lib().ecg_sum_blocks_batch(len(src_ids), _ints(src_ids), stripes.data_ptr(), ss, bs, B, ids, S_sel,
                                      v.data_ptr(), _stream(stream)), "sum.blocks_batch")
    return v


def verify_batch(src_ids, stripes, expected, stripe_ids=None, out=None, stream=None):
    """blocks_batch, then the compare with `expected` ((S_sel, n) int32 CUDA, row i for stripe stripe_ids[i]).
    Returns (sums, targets, bad): targets[i] is -1 (no column differs), j (exactly column j) or n (more than one);
    bad[i] counts the columns that differ."""
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    ids, S_sel = _selection(stripe_ids, S)
    n = len(src_ids)
    v = _sums(out, S_sel, n, stripes.device)
    targets, bad = _verdicts(S_sel, stripes.device)
    _check(lib().ecg_sum_verify_batch(n, _ints(src_ids), stripes.data_ptr(), ss, bs, B, ids, S_sel,
                                      _expected(expected, S_sel, n), v.data_ptr(), targets.data_ptr(), bad.data_ptr(),
                                      _stream(stream)), "sum.verify_batch")
    return v, targets, bad


def ec_batch(code, stripes, stripe_ids=None, out=None, stream=None):
    """All k + m blocks of the code's stripes [S][k+m][B].  Returns the (S_sel, k + m) sums."""
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    ids, S_sel = _selection(stripe_ids, S)
    v = _sums(out, S_sel, code.k + code.m, stripes.device)
    _check(ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, _stream(stream)), "set_memory")
    _check(lib().ecg_sum_ec_batch(code._h, stripes.data_ptr(), ss, bs, B, ids, S_sel, v.data_ptr(), _stream(stream)),
           "sum.ec_batch")
    return v


def verify_ec_batch(code, stripes, expected, stripe_ids=None, out=None, stream=None):
    """ec_batch, then the compare: (sums, targets, bad) as verify_batch."""
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    ids, S_sel = _selection(stripe_ids, S)
    n = code.k + code.m
    v = _sums(out, S_sel, n, stripes.device)
    targets, bad = _verdicts(S_sel, stripes.device)
    _check(ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, _stream(stream)), "set_memory")
    _check(lib().ecg_sum_verify_ec_batch(code._h, stripes.data_ptr(), ss, bs, B, ids, S_sel,
                                         _expected(expected, S_sel, n), v.data_ptr(), targets.data_ptr(),
                                         bad.data_ptr(), _stream(stream)), "sum.verify_ec_batch")
    return v, targets, bad


def ec(code, data_ptrs, coding_ptrs, block_size, out=None, stream=None):
    """One stripe through its block pointers (lists of uint8 CUDA tensors), on the handle's stream.  Returns the
    (1, k + m) sums."""
    code._bind(list(data_ptrs) + list(coding_ptrs), stream)
    v = _sums(out, 1, code.k + code.m, data_ptrs[0].device)
    _check(lib().ecg_sum_ec(code._h, _ptrs(data_ptrs), _ptrs(coding_ptrs), block_size, v.data_ptr()), "sum.ec")
    return v


def crc32c(data):
    """crc32c of host bytes (bytes, bytearray, memoryview or a contiguous numpy array), on the CPU."""
    a = data if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
    a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    return int(lib().ecg_sum_crc32c(a.ctypes.data, a.size)) if a.size else 0


def combine(crc_a, crc_b, len_b):
    """crc32c(A || B) from crc32c(A), crc32c(B) and len(B), any length in [0, 2^63)."""
    if len_b < 0:
        raise EcgError(ecg.ECG_EINVAL, "sum.combine: len_b must not be negative")
    return int(lib().ecg_sum_combine(int(crc_a) & 0xFFFFFFFF, int(crc_b) & 0xFFFFFFFF, int(len_b)))


def counters():
    """Process-wide {launches, bytes}: kernels launched and the bytes they read as planned (S_sel * n * B per call)."""
    return _checklib.counters(lib(), "sum")


def last_launch():
    """Geometry of the most recent call's main launch (include/ecg_sum.h ecg_sum_last_launch): {path, segment_bytes,
    segments_per_block, blocks, table_scheme}, all zero before the first."""
    f = lib().ecg_sum_last_launch
    n = f(None, 0)
    if n != len(LAST_LAUNCH_FIELDS):
        raise EcgError(ecg.ECG_EINVAL, f"sum.last_launch: library has {n} fields")
    v = (ctypes.c_int * n)()
    f(v, n)
    return dict(zip(LAST_LAUNCH_FIELDS, (int(x) for x in v)))


def set_segment_bytes(nbytes):
    """Bytes of a block per workgroup on the vector path, process-wide: 0 = auto, else a multiple of 2048."""
    _check(lib().ecg_sum_set_segment_bytes(int(nbytes)), "sum.set_segment_bytes")


def set_table_scheme(scheme):
    """LDS layout of the row tables, process-wide: -1 = auto, 0 = one copy, 1 = several copies of every entry (include/ecg_sum.h)."""
    _check(lib().ecg_sum_set_table_scheme(int(scheme)), "sum.set_table_scheme")
