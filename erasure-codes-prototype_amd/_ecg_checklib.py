"""What the bindings of the check libraries share (ecg_scrub.py, ecg_locate.py, ecg_heal.py, ecg_heal2.py): loading a
library that links against libecg.so, checking the tensors a call takes, and reading a library's counters and last
launch.  `name` is the library's short name ("scrub", "locate", "heal", "heal2"): it is the prefix of its error
messages and the middle of its symbols (ecg_<name>_counters).  Private to the package.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

import ecg
from ecg import EcgError, _check, _ints, _ptrs, _stream, _strides, torch

# ctypes shorthands for the signature tables
I, LL, P = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
IP, UP, PP, LLP = (ctypes.POINTER(t) for t in (ctypes.c_int, ctypes.c_uint, ctypes.c_void_p, ctypes.c_longlong))


def lib_path(name):
    """lib<name>.so beside libecg.so."""
    return os.path.join(os.path.dirname(os.path.abspath(ecg.LIB_PATH)), f"lib{name}.so")


def load(path, sig):
    """The CDLL at `path`, loaded after libecg.so, with sig = {symbol: (argtypes, restype)} applied."""
    ecg.lib()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not built (run `make -C erasure-codes-prototype_amd`)")
    L = ctypes.CDLL(path)
    for symbol, (args, res) in sig.items():
        f = getattr(L, symbol)
        f.argtypes = args
        f.restype = res
    return L


def int32_vector(name, t, what):
    """(device pointer, length) of a contiguous 1-D int32 CUDA tensor."""
    if t.dtype != torch.int32 or not t.is_cuda or t.dim() != 1 or not t.is_contiguous():
        raise EcgError(ecg.ECG_EINVAL, f"{name}: {what} must be a contiguous 1-D int32 CUDA tensor")
    return t.data_ptr(), int(t.numel())


def selection(name, stripe_ids, targets, S):
    """(ids pointer or None, targets pointer or None, S_sel): stripe_ids None = all S stripes in order; targets None =
    no named block, else one entry per selected stripe."""
    ids, S_sel = (None, S) if stripe_ids is None else int32_vector(name, stripe_ids, "stripe_ids")
    if targets is None:
        return ids, None, S_sel
    tp, nt = int32_vector(name, targets, "targets")
    if nt != S_sel:
        raise EcgError(ecg.ECG_EINVAL, f"{name}: {nt} targets for {S_sel} selected stripes")
    return ids, tp, S_sel


def result_tensor(name, out, shape, device, describe):
    """The int32 result tensor of `shape`: `out` if given (checked; `describe` names the shape in the refusal), else a
    fresh one.  The call zeroes it."""
    if out is None:
        return torch.empty(shape, dtype=torch.int32, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.int32 or not out.is_cuda or not out.is_contiguous():
        raise EcgError(ecg.ECG_EINVAL, f"{name}: out must be a contiguous int32 CUDA tensor of shape {describe}")
    return out


def counters(L, name):
    """Process-wide {launches, bytes} of a library: kernels launched and the bytes they read as planned."""
    v = [ctypes.c_longlong(0) for _ in range(2)]
    _check(getattr(L, f"ecg_{name}_counters")(*[ctypes.byref(x) for x in v]), f"{name}.counters")
    return {"launches": v[0].value, "bytes": v[1].value}


LAST_LAUNCH_FIELDS = ("grid_map", "map_group", "cols_per_wg", "wg_per_stripe", "S", "rtiles")


def last_launch(L, name):
    """Geometry of a library's most recent vector-path launch: {field: value} over LAST_LAUNCH_FIELDS."""
    f = getattr(L, f"ecg_{name}_last_launch")
    n = f(None, 0)
    if n != len(LAST_LAUNCH_FIELDS):
        raise EcgError(ecg.ECG_EINVAL, f"{name}.last_launch: library has {n} fields")
    v = (ctypes.c_int * n)()
    f(v, n)
    return dict(zip(LAST_LAUNCH_FIELDS, (int(x) for x in v)))


# The four call forms of a correcting library (ecg_heal.py, ecg_heal2.py): `lib` is the module's loader, called once the
# arguments have passed; the report has n + extra counters per stripe.

def _report(name, extra, out, S_sel, n, device):
    return result_tensor(name, out, (S_sel, n + extra), device, f"(S_sel, n + {extra})")


def correct_matrix_batch(lib, name, extra, H, src_ids, stripes, stripe_ids, targets, out, stream):
    n = len(src_ids)
    H = np.asarray(H, dtype=np.int64).reshape(-1, n)
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    ids, tg, S_sel = selection(name, stripe_ids, targets, S)
    v = _report(name, extra, out, S_sel, n, stripes.device)
    f = getattr(lib(), f"ecg_{name}_matrix_batch")
    _check(f(n, H.shape[0], _ints(H.ravel()), _ints(src_ids), stripes.data_ptr(), ss, bs, B, ids, tg, S_sel,
             v.data_ptr(), _stream(stream)), f"{name}.matrix_batch")
    return v


def correct_encode_batch(lib, name, extra, k, m, matrix, stripes, stripe_ids, targets, out, stream):
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    ids, tg, S_sel = selection(name, stripe_ids, targets, S)
    v = _report(name, extra, out, S_sel, k + m, stripes.device)
    f = getattr(lib(), f"ecg_{name}_encode_batch")
    _check(f(k, m, _ints(matrix), stripes.data_ptr(), ss, bs, B, ids, tg, S_sel, v.data_ptr(), _stream(stream)),
           f"{name}.encode_batch")
    return v


def correct_ec_batch(lib, name, extra, code, stripes, stripe_ids, targets, out, stream):
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    ids, tg, S_sel = selection(name, stripe_ids, targets, S)
    v = _report(name, extra, out, S_sel, code.k + code.m, stripes.device)
    _check(ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, _stream(stream)), "set_memory")
    f = getattr(lib(), f"ecg_{name}_ec_batch")
    _check(f(code._h, stripes.data_ptr(), ss, bs, B, ids, tg, S_sel, v.data_ptr(), _stream(stream)),
           f"{name}.ec_batch")
    return v


def correct_ec(lib, name, extra, code, data_ptrs, coding_ptrs, block_size, target, out, stream):
    code._bind(list(data_ptrs) + list(coding_ptrs), stream)
    v = _report(name, extra, out, 1, code.k + code.m, data_ptrs[0].device)
    f = getattr(lib(), f"ecg_{name}_ec")
    _check(f(code._h, _ptrs(data_ptrs), _ptrs(coding_ptrs), block_size, int(target), v.data_ptr()), f"{name}.ec")
    return v
