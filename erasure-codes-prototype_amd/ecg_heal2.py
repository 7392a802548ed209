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

import ctypes
import os

import numpy as np

import ecg
from ecg import EcgError, _check, _ints, _ptrs, _stream, _strides, torch

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(ecg.LIB_PATH)), "libecg_heal2.so")

# Every symbol include/ecg_heal2.h declares (checked by tests/test_heal2_host.py).
EXPORTS = [
    "ecg_heal2_matrix_batch", "ecg_heal2_encode_batch", "ecg_heal2_ec_batch", "ecg_heal2_ec", "ecg_heal2_counters",
    "ecg_heal2_last_launch",
]

ANY = -1  # ecg_heal2_ec's target for ANY2

_L = None


def lib():
    """Load libecg_heal2.so (after libecg.so, which it links against)."""
    global _L
    if _L is not None:
        return _L
    ecg.lib()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not built (run `make -C erasure-codes-prototype_amd`)")
    L = ctypes.CDLL(LIB_PATH)
    I, LL, P = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    IP = ctypes.POINTER(ctypes.c_int)
    PP = ctypes.POINTER(ctypes.c_void_p)
    sig = {
        "ecg_heal2_matrix_batch": ([I, I, IP, IP, P, LL, LL, LL, P, P, I, P, P], I),
        "ecg_heal2_encode_batch": ([I, I, IP, P, LL, LL, LL, P, P, I, P, P], I),
        "ecg_heal2_ec_batch": ([P, P, LL, LL, LL, P, P, I, P, P], I),
        "ecg_heal2_ec": ([P, PP, PP, I, I, P], I),
        "ecg_heal2_counters": ([ctypes.POINTER(LL)] * 2, I),
        "ecg_heal2_last_launch": ([IP, I], I),
    }
    for name, (args, res) in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    _L = L
    return L


def _int32_vector(t, what):
    if t.dtype != torch.int32 or not t.is_cuda or t.dim() != 1 or not t.is_contiguous():
        raise EcgError(ecg.ECG_EINVAL, f"heal2: {what} must be a contiguous 1-D int32 CUDA tensor")
    return t.data_ptr(), int(t.numel())


def _selection(stripe_ids, targets, S):
    """(ids pointer or None, targets pointer or None, S_sel): stripe_ids None = all S stripes in order; targets None =
    ANY2, else one entry per selected stripe."""
    ids, S_sel = (None, S) if stripe_ids is None else _int32_vector(stripe_ids, "stripe_ids")
    if targets is None:
        return ids, None, S_sel
    tp, nt = _int32_vector(targets, "targets")
    if nt != S_sel:
        raise EcgError(ecg.ECG_EINVAL, f"heal2: {nt} targets for {S_sel} selected stripes")
    return ids, tp, S_sel


def _report(out, S_sel, n, device):
    """The (S_sel, n + 3) int32 result tensor: `out` if given (checked), else a fresh one.  The call zeroes it."""
    if out is None:
        return torch.empty((S_sel, n + 3), dtype=torch.int32, device=device)
    if (tuple(out.shape) != (S_sel, n + 3) or out.dtype != torch.int32 or not out.is_cuda or
            not out.is_contiguous()):
        raise EcgError(ecg.ECG_EINVAL, "heal2: out must be a contiguous int32 CUDA tensor of shape (S_sel, n + 3)")
    return out


def matrix_batch(H, src_ids, stripes, stripe_ids=None, targets=None, out=None, stream=None):
    """H: r x n check matrix (nested or flat); src_ids: the n block indices its columns stand for; stripes: [S][*][B]
    uint8 CUDA tensor view (any strides), corrected in place.  Returns the (S_sel, n + 3) report; report[:, j], and a
    target j, are block src_ids[j]."""
    n = len(src_ids)
    H = np.asarray(H, dtype=np.int64).reshape(-1, n)
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    ids, tg, S_sel = _selection(stripe_ids, targets, S)
    v = _report(out, S_sel, n, stripes.device)
    _check(lib().ecg_heal2_matrix_batch(n, H.shape[0], _ints(H.ravel()), _ints(src_ids), stripes.data_ptr(), ss, bs, B,
                                       ids, tg, S_sel, v.data_ptr(), _stream(stream)), "heal2.matrix_batch")
    return v


def encode_batch(k, m, matrix, stripes, stripe_ids=None, targets=None, out=None, stream=None):
    """H = [matrix | I] over stripes [S][k+m][B] (data 0..k-1, coding k..k+m-1), corrected in place.  Returns the
    (S_sel, k+m+3) report."""
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    ids, tg, S_sel = _selection(stripe_ids, targets, S)
    v = _report(out, S_sel, k + m, stripes.device)
    _check(lib().ecg_heal2_encode_batch(k, m, _ints(matrix), stripes.data_ptr(), ss, bs, B, ids, tg, S_sel, v.data_ptr(),
                                       _stream(stream)), "heal2.encode_batch")
    return v


def ec_batch(code, stripes, stripe_ids=None, targets=None, out=None, stream=None):
    """The class's own check (ErasureCode.check_matrix) over stripes [S][k+m][B], corrected in place.  Returns the
    (S_sel, k+m+3) report."""
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    ids, tg, S_sel = _selection(stripe_ids, targets, S)
    v = _report(out, S_sel, code.k + code.m, stripes.device)
    _check(ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, _stream(stream)), "set_memory")
    _check(lib().ecg_heal2_ec_batch(code._h, stripes.data_ptr(), ss, bs, B, ids, tg, S_sel, v.data_ptr(),
                                   _stream(stream)), "heal2.ec_batch")
    return v


def ec(code, data_ptrs, coding_ptrs, block_size, target=ANY, out=None, stream=None):
    """One stripe through its block pointers (lists of uint8 CUDA tensors), on the handle's stream; target: a block
    id (a host int), or ANY.  Returns the (1, k+m+3) report."""
    code._bind(list(data_ptrs) + list(coding_ptrs), stream)
    v = _report(out, 1, code.k + code.m, data_ptrs[0].device)
    _check(lib().ecg_heal2_ec(code._h, _ptrs(data_ptrs), _ptrs(coding_ptrs), block_size, int(target), v.data_ptr()),
           "heal2.ec")
    return v


def counters():
    """Process-wide {launches, bytes}: heal2 kernels launched and the bytes they read as planned (S_sel * B * n)."""
    v = [ctypes.c_longlong(0) for _ in range(2)]
    _check(lib().ecg_heal2_counters(*[ctypes.byref(x) for x in v]), "heal2.counters")
    return {"launches": v[0].value, "bytes": v[1].value}


LAST_LAUNCH_FIELDS = ("grid_map", "map_group", "cols_per_wg", "wg_per_stripe", "S", "rtiles")


def last_launch():
    """Geometry of the process's most recent vector-path heal2 launch, as placed in the launch descriptor after the
    fallbacks (include/ecg_heal2.h ecg_heal2_last_launch): {grid_map, map_group, cols_per_wg, wg_per_stripe, S,
    rtiles}, all zero before the first.  Byte-kernel launches do not change it."""
    n = lib().ecg_heal2_last_launch(None, 0)
    if n != len(LAST_LAUNCH_FIELDS):
        raise EcgError(ecg.ECG_EINVAL, f"heal2.last_launch: library has {n} fields")
    v = (ctypes.c_int * n)()
    lib().ecg_heal2_last_launch(v, n)
    return dict(zip(LAST_LAUNCH_FIELDS, (int(x) for x in v)))
