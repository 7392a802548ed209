"""Python binding of libecg_update.so (include/ecg_update.h): the delta update, small overwrites applied to data and
parity in place.

For a coefficient matrix G (m_out x k_in; column j is data block src_ids[j], row i parity block dst_ids[i]) one call
applies R records {stripe, col, off, len, in_off} to strided stripes on the device.  WRITE mode takes the new bytes of
[off, off + len) of data block `col` from data_in[in_off ..): delta = old ^ new, the data block gets the new bytes, and
every parity i with G[i][col] != 0 gets parity_i ^= G[i][col] * delta on the same range.  DELTA mode takes delta itself
and touches the parities only.  No byte outside the records' ranges is stored to.  The records of one call that name
the same stripe must have pairwise disjoint ranges (`check_records` says whether they do).

The report comes back as an int32 CUDA tensor of shape (R, 2), {state, changed} per record, asynchronously on torch's
current stream (or `stream`): state 0 applied, 1 stripe, 2 col, 3 off/len, 4 len > max_len, 5 staging range; a refused
record moves nothing.  Checksums are not updated: `touched_stripes` gives the stripe ids to re-sum and re-check
(ecg_sum, ecg_psum, ecg_scrub).

There is no CPU fallback: if libecg_update.so is missing or has no GPU to run on, calls raise.
"""
from __future__ import annotations

import ctypes

import numpy as np

import _ecg_checklib as _checklib
import ecg
from _ecg_checklib import I, IP, LL, LLP, P, PP
from ecg import EcgError, _check, _ints, _ptrs, _stream, _strides, torch

LIB_PATH = _checklib.lib_path("ecg_update")

# Every symbol include/ecg_update.h declares (checked by tests/test_update_host.py).
EXPORTS = [
    "ecg_update_matrix_batch", "ecg_update_encode_batch", "ecg_update_ec_batch", "ecg_update_ec",
    "ecg_update_check_records", "ecg_update_traffic_bytes", "ecg_update_counters", "ecg_update_last_launch",
]

WRITE, DELTA = 0, 1
APPLIED, BAD_STRIPE, BAD_COL, BAD_RANGE, TOO_LONG, BAD_STAGING = range(6)   # report[:, 0]
LAST_LAUNCH_FIELDS = ("cols_per_wg", "wg_per_record", "R", "max_nnz")

_UBP = ctypes.POINTER(ctypes.c_ubyte)
_BATCH = [LL, LL, LL, I, I, P, I, LL, P, LL, P, P, P]    # sstride .. stream
_SIG = {
    "ecg_update_matrix_batch": ([I, I, IP, IP, IP, P] + _BATCH, I),
    "ecg_update_encode_batch": ([I, I, IP, P] + _BATCH, I),
    "ecg_update_ec_batch": ([P, P] + _BATCH, I),
    "ecg_update_ec": ([P, PP, PP, I, I, I, LL, LL, P, P, P], I),
    "ecg_update_check_records": ([LLP, I, I, LL, I, LL, LL, I], I),
    "ecg_update_traffic_bytes": ([_UBP, LLP, I, I, I], LL),
    "ecg_update_counters": ([LLP] * 2, I),
    "ecg_update_last_launch": ([IP, I], I),
}

_L = None


def lib():
    """Load libecg_update.so (after libecg.so, which it links against)."""
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
            raise EcgError(ecg.ECG_EINVAL, "update: records must be a contiguous (R, 5) int64 tensor")
        return records
    return torch.from_numpy(_host_records(records)).to(device)


def _staging(t, what):
    if t.dtype != torch.uint8 or not t.is_cuda or t.dim() != 1 or not t.is_contiguous():
        raise EcgError(ecg.ECG_EINVAL, f"update: {what} must be a contiguous 1-D uint8 CUDA tensor")
    return t


def _batch_args(stripes, records, data_in, mode, max_len, delta_out, out, stream):
    """The arguments sstride .. stream of a batch form, the report tensor and what must stay alive until the call
    returns."""
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    rec = _device_records(records, stripes.device)
    R = int(rec.shape[0])
    data_in = _staging(data_in, "data_in")
    if delta_out is not None and _staging(delta_out, "delta_out").numel() < data_in.numel():
        raise EcgError(ecg.ECG_EINVAL, "update: delta_out is smaller than data_in")
    if max_len is None:
        max_len = B if rec is records else int(np.clip(_host_records(records)[:, 3], 0, B).max(initial=0))
    v = _checklib.result_tensor("update", out, (R, 2), stripes.device, "(R, 2)")
    args = (ss, bs, B, S, int(mode), rec.data_ptr(), R, int(max_len), data_in.data_ptr(), int(data_in.numel()),
            None if delta_out is None else delta_out.data_ptr(), v.data_ptr(), _stream(stream))
    return args, v, rec


def matrix_batch(G, src_ids, dst_ids, stripes, records, data_in, mode=WRITE, max_len=None, delta_out=None, out=None,
                 stream=None):
    """G: m_out x k_in coefficients (nested or flat); src_ids / dst_ids: the blocks its columns / rows stand for;
    stripes: [S][*][B] uint8 CUDA tensor view (any strides), updated in place; records: (R, 5) int64 {stripe, col, off,
    len, in_off}, host data or a CUDA tensor; data_in: 1-D uint8 CUDA staging buffer; max_len: the longest record
    (None: taken from host records, B for device records); delta_out: 1-D uint8 CUDA tensor as large as data_in that
    receives delta at the records' staging ranges (WRITE only).  Returns the (R, 2) report."""
    k_in = len(src_ids)
    G = np.asarray(G, dtype=np.int64).reshape(-1, k_in)
    args, v, keep = _batch_args(stripes, records, data_in, mode, max_len, delta_out, out, stream)
    if v.shape[0] == 0:
        return v
    _check(lib().ecg_update_matrix_batch(k_in, G.shape[0], _ints(G.ravel()), _ints(src_ids), _ints(dst_ids),
                                         stripes.data_ptr(), *args), "update.matrix_batch")
    return v


def encode_batch(k, m, matrix, stripes, records, data_in, mode=WRITE, max_len=None, delta_out=None, out=None,
                 stream=None):
    """G = matrix (m x k) over stripes [S][k+m][B]: data 0..k-1, coding k..k+m-1.  Returns the (R, 2) report."""
    args, v, keep = _batch_args(stripes, records, data_in, mode, max_len, delta_out, out, stream)
    if v.shape[0] == 0:
        return v
    _check(lib().ecg_update_encode_batch(k, m, _ints(matrix), stripes.data_ptr(), *args), "update.encode_batch")
    return v


def ec_batch(code, stripes, records, data_in, mode=WRITE, max_len=None, delta_out=None, out=None, stream=None):
    """The class's own encoding matrix over stripes [S][k+m][B].  Returns the (R, 2) report."""
    args, v, keep = _batch_args(stripes, records, data_in, mode, max_len, delta_out, out, stream)
    _check(ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, _stream(stream)), "set_memory")
    if v.shape[0] == 0:
        return v
    _check(lib().ecg_update_ec_batch(code._h, stripes.data_ptr(), *args), "update.ec_batch")
    return v


def ec(code, data_ptrs, coding_ptrs, block_size, col, off, data_in, mode=WRITE, delta_out=None, out=None, stream=None):
    """One record on one stripe through its block pointers (lists of uint8 CUDA tensors), on the handle's stream: bytes
    [off, off + len(data_in)) of data block `col`.  Returns the (1, 2) report."""
    data_in = _staging(data_in, "data_in")
    if delta_out is not None and _staging(delta_out, "delta_out").numel() < data_in.numel():
        raise EcgError(ecg.ECG_EINVAL, "update: delta_out is smaller than data_in")
    code._bind(list(data_ptrs) + list(coding_ptrs), stream)
    v = _checklib.result_tensor("update", out, (1, 2), data_in.device, "(1, 2)")
    _check(lib().ecg_update_ec(code._h, _ptrs(data_ptrs), _ptrs(coding_ptrs), block_size, int(mode), int(col), int(off),
                               int(data_in.numel()), data_in.data_ptr(),
                               None if delta_out is None else delta_out.data_ptr(), v.data_ptr()), "update.ec")
    return v


def check_records(records, k_in, B, S, max_len, in_bytes, with_delta_out=False):
    """Host only: -1 if every record is state 0 and the ranges (and, with_delta_out, the staging ranges) are pairwise
    disjoint; else the index of the first offending record, with ecg.lib().ecg_last_error() naming the rule."""
    h = _host_records(records)
    rc = lib().ecg_update_check_records(h.ctypes.data_as(LLP), h.shape[0], int(k_in), int(B), int(S), int(max_len),
                                        int(in_bytes), 1 if with_delta_out else 0)
    if rc < -1:
        _check(rc, "update.check_records")
    return rc


def traffic_bytes(nnz_per_col, records, mode=WRITE, with_delta_out=False):
    """Host only: the bytes the records move by the definition, len * ((3 if WRITE else 1) + with_delta_out +
    2 * nnz_per_col[col]) summed over the records."""
    h = _host_records(records)
    nnz = np.ascontiguousarray(nnz_per_col, dtype=np.uint8)
    if h.shape[0] and (h[:, 1].min() < 0 or h[:, 1].max() >= nnz.size):
        raise EcgError(ecg.ECG_EINVAL, "update.traffic_bytes: a record's col has no entry in nnz_per_col")
    return _check(lib().ecg_update_traffic_bytes(nnz.ctypes.data_as(_UBP), h.ctypes.data_as(LLP), h.shape[0],
                                                 int(mode), 1 if with_delta_out else 0), "update.traffic_bytes")


def nnz_per_col(G, k_in):
    """Nonzero coefficients per column of G (m_out x k_in, nested or flat): traffic_bytes' first argument."""
    return np.count_nonzero(np.asarray(G, dtype=np.int64).reshape(-1, k_in), axis=0).astype(np.uint8)


def touched_stripes(records, report=None, device="cuda"):
    """The sorted distinct stripe ids of the applied records as an int32 CUDA tensor: the stripe_ids that ecg_sum,
    ecg_psum and ecg_scrub take to re-sum and re-check what was written.  report: the call's (R, 2) report (copied
    back: that synchronises); None takes every record with len > 0 as applied."""
    h = _host_records(records)
    if report is None:
        applied = h[:, 3] > 0
    else:
        applied = (report.cpu().numpy().reshape(-1, 2)[:, 0] == APPLIED) & (h[:, 3] > 0)
    return torch.from_numpy(np.unique(h[applied, 0]).astype(np.int32)).to(device)


def counters():
    """Process-wide {launches, records}: update kernels launched and the records they covered."""
    v = [ctypes.c_longlong(0) for _ in range(2)]
    _check(lib().ecg_update_counters(*[ctypes.byref(x) for x in v]), "update.counters")
    return {"launches": v[0].value, "records": v[1].value}


def last_launch():
    """Geometry of the process's most recent update launch that covered 16-byte columns (include/ecg_update.h
    ecg_update_last_launch): {cols_per_wg, wg_per_record, R, max_nnz}, all zero before the first."""
    f = lib().ecg_update_last_launch
    n = f(None, 0)
    if n != len(LAST_LAUNCH_FIELDS):
        raise EcgError(ecg.ECG_EINVAL, f"update.last_launch: library has {n} fields")
    v = (ctypes.c_int * n)()
    f(v, n)
    return dict(zip(LAST_LAUNCH_FIELDS, (int(x) for x in v)))
