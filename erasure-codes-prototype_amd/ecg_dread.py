"""Python binding of libecg_dread.so (include/ecg_dread.h): degraded range reads, byte ranges of stored blocks answered
into a caller buffer with the ranges of lost blocks rebuilt from the survivors.

For a check matrix H (r x n; column j is block src_ids[j]) one call answers R records {stripe, col, off, len, out_off}
over strided stripes on the device: bytes [off, off + len) of column `col` of the stripe go to out[out_off ..).
lost[S][n] flags every stripe's lost columns.  A column that is not lost is copied; a lost one is rebuilt as
XOR c_j * v_j over the survivors j with c_j != 0, c = Plan(H, E, col) (`plan` is the rule on the host).  Nothing of the
stripes is written and no byte of `out` outside the answered ranges is stored to.  The out ranges of one call must be
pairwise disjoint (`check_records` says whether they are).  Survivors are taken as good: the answer is not verified.

A call returns (out, report), asynchronously on torch's current stream (or `stream`): report is an int32 CUDA tensor of
shape (R, 2), {state, reads} per record: state 0 answered, 1 stripe, 2 col, 3 off/len, 4 len > max_len, 5 out range,
6 not recoverable; a refused record moves nothing.

There is no CPU fallback: if libecg_dread.so is missing or has no GPU to run on, calls raise.
"""
from __future__ import annotations

import ctypes

import numpy as np

import _ecg_checklib as _checklib
import ecg
from _ecg_checklib import I, IP, LL, LLP, P
from ecg import EcgError, _check, _ints, _stream, _strides, torch

LIB_PATH = _checklib.lib_path("ecg_dread")

# Every symbol include/ecg_dread.h declares (checked by tests/test_dread_host.py).
EXPORTS = [
    "ecg_dread_matrix_batch", "ecg_dread_encode_batch", "ecg_dread_ec_batch", "ecg_dread_work_bytes",
    "ecg_dread_plan", "ecg_dread_check_records", "ecg_dread_counters", "ecg_dread_last_launch",
]

ANSWERED, BAD_STRIPE, BAD_COL, BAD_RANGE, TOO_LONG, BAD_OUT, UNRECOVERABLE = range(7)   # report[:, 0]
LAST_LAUNCH_FIELDS = ("cols_per_wg", "wg_per_record", "R", "max_reads")

_UBP = ctypes.POINTER(ctypes.c_ubyte)
_BATCH = [LL, LL, LL, I, P, P, I, LL, P, LL, P, P, P]    # sstride .. stream
_SIG = {
    "ecg_dread_matrix_batch": ([I, I, IP, IP, P] + _BATCH, I),
    "ecg_dread_encode_batch": ([I, I, IP, P] + _BATCH, I),
    "ecg_dread_ec_batch": ([P, P] + _BATCH, I),
    "ecg_dread_work_bytes": ([I, I], LL),
    "ecg_dread_plan": ([I, I, IP, _UBP, I, _UBP, IP], I),
    "ecg_dread_check_records": ([LLP, I, I, LL, I, LL, LL], I),
    "ecg_dread_counters": ([LLP] * 2, I),
    "ecg_dread_last_launch": ([IP, I], I),
}

_L = None


def lib():
    """Load libecg_dread.so (after libecg.so, which it links against)."""
    global _L
    if _L is None:
        _L = _checklib.load(LIB_PATH, _SIG)
    return _L


def _host_records(records):
    """(R, 5) int64 numpy array of records given as a numpy array, a nested sequence or a tensor (a CUDA tensor is
    copied back: that synchronises)."""
    if torch is not None and isinstance(records, torch.Tensor):
        records = records.cpu().numpy()
    return np.ascontiguousarray(np.asarray(records, dtype=np.int64).reshape(-1, 5))


def _device_records(records, device):
    """The records as a contiguous (R, 5) int64 CUDA tensor (uploaded if they are host data)."""
    if torch is not None and isinstance(records, torch.Tensor) and records.is_cuda:
        if records.dtype != torch.int64 or records.dim() != 2 or records.shape[1] != 5 or not records.is_contiguous():
            raise EcgError(ecg.ECG_EINVAL, "dread: records must be a contiguous (R, 5) int64 tensor")
        return records
    return torch.from_numpy(_host_records(records)).to(device)


def _device_lost(lost, S, n, device):
    """The lost flags as a contiguous (S, n) uint8 CUDA tensor (uploaded if they are host data)."""
    if torch is not None and isinstance(lost, torch.Tensor) and lost.is_cuda:
        if lost.dtype != torch.uint8 or tuple(lost.shape) != (S, n) or not lost.is_contiguous():
            raise EcgError(ecg.ECG_EINVAL, f"dread: lost must be a contiguous ({S}, {n}) uint8 tensor")
        return lost
    h = np.ascontiguousarray(np.asarray(lost).astype(bool).astype(np.uint8))
    if h.shape != (S, n):
        raise EcgError(ecg.ECG_EINVAL, f"dread: lost has shape {h.shape}, not ({S}, {n})")
    return torch.from_numpy(h).to(device)


def work_bytes(R, n):
    """Bytes of device scratch a call over R records of an n-column check needs."""
    return _check(lib().ecg_dread_work_bytes(int(R), int(n)), "dread.work_bytes")


def _batch_args(n, stripes, lost, records, out, max_len, work, report, stream):
    """The arguments sstride .. stream of a batch form, the answer and report tensors and what must stay alive until
    the call returns."""
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    rec = _device_records(records, stripes.device)
    R = int(rec.shape[0])
    flags = _device_lost(lost, S, n, stripes.device)
    if isinstance(out, int):
        out = torch.empty((out,), dtype=torch.uint8, device=stripes.device)
    if out.dtype != torch.uint8 or not out.is_cuda or out.dim() != 1 or not out.is_contiguous():
        raise EcgError(ecg.ECG_EINVAL, "dread: out must be a contiguous 1-D uint8 CUDA tensor (or a byte count)")
    if max_len is None:
        max_len = B if rec is records else int(np.clip(_host_records(records)[:, 3], 0, B).max(initial=0))
    need = work_bytes(R, n)
    if work is None:
        work = torch.empty((max(need, 32),), dtype=torch.uint8, device=stripes.device)
    elif work.dtype != torch.uint8 or not work.is_cuda or not work.is_contiguous() or work.numel() < need:
        raise EcgError(ecg.ECG_EINVAL, f"dread: work must be a contiguous uint8 CUDA tensor of at least {need} bytes")
    v = _checklib.result_tensor("dread", report, (R, 2), stripes.device, "(R, 2)")
    # an answer buffer of zero bytes has no address: the scratch's stands in, and out_bytes = 0 keeps it unwritten
    out_ptr = out.data_ptr() if out.numel() else work.data_ptr()
    args = (ss, bs, B, S, flags.data_ptr(), rec.data_ptr(), R, int(max_len), out_ptr, int(out.numel()),
            work.data_ptr(), v.data_ptr(), _stream(stream))
    return args, out, v, (rec, flags, work)


def matrix_batch(H, src_ids, stripes, lost, records, out, max_len=None, work=None, report=None, stream=None):
    """H: r x n check matrix (nested or flat); src_ids: the blocks its columns stand for; stripes: [S][*][B] uint8 CUDA
    tensor view (any strides), never written; lost: (S, n) flags, host data or a uint8 CUDA tensor; records: (R, 5)
    int64 {stripe, col, off, len, out_off}, host data or a CUDA tensor; out: the 1-D uint8 CUDA answer buffer, or its
    size in bytes (a fresh one, uninitialised outside the answered ranges); max_len: the longest record (None: taken
    from host records, B for device records); work: uint8 CUDA scratch of work_bytes(R, n) bytes (None: allocated).
    Returns (out, report), report the (R, 2) int32 {state, reads}."""
    n = len(src_ids)
    H = np.asarray(H, dtype=np.int64).reshape(-1, n)
    args, out, v, keep = _batch_args(n, stripes, lost, records, out, max_len, work, report, stream)
    if v.shape[0] == 0:
        return out, v
    _check(lib().ecg_dread_matrix_batch(n, H.shape[0], _ints(H.ravel()), _ints(src_ids), stripes.data_ptr(), *args),
           "dread.matrix_batch")
    return out, v


def encode_batch(k, m, matrix, stripes, lost, records, out, max_len=None, work=None, report=None, stream=None):
    """H = [matrix | I] (matrix: m x k) over stripes [S][k+m][B]: data 0..k-1, coding k..k+m-1.  Returns
    (out, report)."""
    args, out, v, keep = _batch_args(k + m, stripes, lost, records, out, max_len, work, report, stream)
    if v.shape[0] == 0:
        return out, v
    _check(lib().ecg_dread_encode_batch(k, m, _ints(matrix), stripes.data_ptr(), *args), "dread.encode_batch")
    return out, v


def ec_batch(code, stripes, lost, records, out, max_len=None, work=None, report=None, stream=None):
    """The class's own check matrix over stripes [S][k+m][B].  Returns (out, report)."""
    args, out, v, keep = _batch_args(code.k + code.m, stripes, lost, records, out, max_len, work, report, stream)
    _check(ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, _stream(stream)), "set_memory")
    if v.shape[0] == 0:
        return out, v
    _check(lib().ecg_dread_ec_batch(code._h, stripes.data_ptr(), *args), "dread.ec_batch")
    return out, v


def plan(H, lost, col):
    """Host only: the plan rule.  H: r x n (nested or flat with n = len(lost)); lost: n flags.  Returns (state, reads,
    c) with c the n coefficients as a uint8 numpy array."""
    flags = np.ascontiguousarray(np.asarray(lost).astype(bool).astype(np.uint8))
    n = int(flags.size)
    H = np.asarray(H, dtype=np.int64).reshape(-1, n)
    c = np.zeros(n, np.uint8)
    reads = ctypes.c_int(0)
    state = _check(lib().ecg_dread_plan(n, H.shape[0], _ints(H.ravel()), flags.ctypes.data_as(_UBP), int(col),
                                        c.ctypes.data_as(_UBP), ctypes.byref(reads)), "dread.plan")
    return state, reads.value, c


def check_records(records, n, B, S, max_len, out_bytes):
    """Host only: -1 if no record is refused with a state 1-5 and the out ranges are pairwise disjoint; else the index
    of the first offending record, with ecg.lib().ecg_last_error() naming the rule."""
    h = _host_records(records)
    rc = lib().ecg_dread_check_records(h.ctypes.data_as(LLP), h.shape[0], int(n), int(B), int(S), int(max_len),
                                       int(out_bytes))
    if rc < -1:
        _check(rc, "dread.check_records")
    return rc


def counters():
    """Process-wide {launches, records}: main kernels launched and the records they covered."""
    v = [ctypes.c_longlong(0) for _ in range(2)]
    _check(lib().ecg_dread_counters(*[ctypes.byref(x) for x in v]), "dread.counters")
    return {"launches": v[0].value, "records": v[1].value}


def last_launch():
    """Geometry of the process's most recent dread launch that covered 16-byte columns (include/ecg_dread.h
    ecg_dread_last_launch): {cols_per_wg, wg_per_record, R, max_reads}, all zero before the first."""
    f = lib().ecg_dread_last_launch
    n = f(None, 0)
    if n != len(LAST_LAUNCH_FIELDS):
        raise EcgError(ecg.ECG_EINVAL, f"dread.last_launch: library has {n} fields")
    v = (ctypes.c_int * n)()
    f(v, n)
    return dict(zip(LAST_LAUNCH_FIELDS, (int(x) for x in v)))
