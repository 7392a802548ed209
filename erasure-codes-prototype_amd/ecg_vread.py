"""Python binding of libecg_vread.so (include/ecg_vread.h): verified range reads, the degraded range read of ecg_dread
whose answers are checked against the store's recorded CRC-32C.

Everything is as in ecg_dread -- H, src_ids, strided stripes, lost flags (None here: nothing is lost), records
{stripe, col, off, len, out_off}, the plan rule -- plus `piece_bytes` (0: block sums, Q = 1; else a power of two P in
[512, 2^30], Q = ceil(B / P)) and `expected`, the recorded (S, n, Q) table.  A record covers the pieces its range
touches; the call computes the column over every covering piece WHOLE (reads * cover bytes are read, not reads * len),
takes its CRC-32C, stores only the range to `out` and compares the sums with the table.

A call returns (out, report, sums), asynchronously on torch's current stream (or `stream`): report is an int32 CUDA
tensor of shape (R, 4), {state, reads, bad, first_bad} per record: states 0-6 are ecg_dread's, state 7 = answered but
`bad` covering pieces differ from the table, the first of them piece `first_bad` of the block (-1, that is 0xFFFFFFFF,
when none differs).  THE BYTES OF A STATE-7 RECORD ARE STORED: read the report before using the bytes.  sums is the
(R, NP) int32 tensor of the computed sums, NP = max_pieces(max_len, piece_bytes, B).

There is no CPU fallback: if libecg_vread.so is missing or has no GPU to run on, calls raise.
"""
from __future__ import annotations

import ctypes

import numpy as np

import _ecg_checklib as _checklib
import ecg
import ecg_dread
from _ecg_checklib import I, IP, LL, LLP, P
from ecg import EcgError, _check, _ints, _stream, _strides, torch

LIB_PATH = _checklib.lib_path("ecg_vread")

# Every symbol include/ecg_vread.h declares (checked by tests/test_vread_host.py).
EXPORTS = [
    "ecg_vread_matrix_batch", "ecg_vread_encode_batch", "ecg_vread_ec_batch", "ecg_vread_work_bytes",
    "ecg_vread_cover", "ecg_vread_max_pieces", "ecg_vread_check_records", "ecg_vread_set_span_bytes",
    "ecg_vread_counters", "ecg_vread_last_launch",
]

ANSWERED, BAD_STRIPE, BAD_COL, BAD_RANGE, TOO_LONG, BAD_OUT, UNRECOVERABLE, MISMATCH = range(8)   # report[:, 0]
NO_PIECE = 0xFFFFFFFF
LAST_LAUNCH_FIELDS = ("path", "piece_bytes", "max_pieces", "span_bytes", "wg_per_record", "R")

_BATCH = [LL, LL, LL, I, P, LL, P, P, I, LL, P, LL, P, P, P, P]    # sstride .. stream
_SIG = {
    "ecg_vread_matrix_batch": ([I, I, IP, IP, P] + _BATCH, I),
    "ecg_vread_encode_batch": ([I, I, IP, P] + _BATCH, I),
    "ecg_vread_ec_batch": ([P, P] + _BATCH, I),
    "ecg_vread_work_bytes": ([I, I], LL),
    "ecg_vread_cover": ([LL, LL, LL, LL, LLP, LLP, LLP], I),
    "ecg_vread_max_pieces": ([LL, LL, LL], LL),
    "ecg_vread_check_records": ([LLP, I, I, LL, I, LL, LL], I),
    "ecg_vread_set_span_bytes": ([LL], I),
    "ecg_vread_counters": ([LLP] * 2, I),
    "ecg_vread_last_launch": ([IP, I], I),
}

_L = None


def lib():
    """Load libecg_vread.so (after libecg.so, which it links against)."""
    global _L
    if _L is None:
        _L = _checklib.load(LIB_PATH, _SIG)
    return _L


def work_bytes(R, n):
    """Bytes of device scratch a call over R records of an n-column check needs."""
    return _check(lib().ecg_vread_work_bytes(int(R), int(n)), "vread.work_bytes")


def cover(off, length, piece_bytes, B):
    """Host only: (q0, npieces, cover_bytes) of bytes [off, off + length) of a B-byte block."""
    v = [ctypes.c_longlong(0) for _ in range(3)]
    _check(lib().ecg_vread_cover(int(off), int(length), int(piece_bytes), int(B), *[ctypes.byref(x) for x in v]),
           "vread.cover")
    return tuple(x.value for x in v)


def max_pieces(max_len, piece_bytes, B):
    """Host only: NP, the most pieces a record of max_len bytes can cover."""
    return _check(lib().ecg_vread_max_pieces(int(max_len), int(piece_bytes), int(B)), "vread.max_pieces")


def set_span_bytes(span_bytes):
    """A test knob: the bytes of a cover one workgroup takes (0 = auto, else a multiple of 2048)."""
    _check(lib().ecg_vread_set_span_bytes(int(span_bytes)), "vread.set_span_bytes")


def _batch_args(n, stripes, lost, piece_bytes, expected, records, out, max_len, work, report, sums, stream):
    """The arguments sstride .. stream of a batch form, the answer, report and sums tensors and what must stay alive
    until the call returns."""
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    dev = stripes.device
    rec = ecg_dread._device_records(records, dev)
    R = int(rec.shape[0])
    flags = None if lost is None else ecg_dread._device_lost(lost, S, n, dev)
    Q = 1 if piece_bytes == 0 else max(1, -(-B // int(piece_bytes)))
    if isinstance(expected, torch.Tensor) and expected.is_cuda:
        if expected.dtype != torch.int32 or expected.numel() != S * n * Q or not expected.is_contiguous():
            raise EcgError(ecg.ECG_EINVAL, f"vread: expected must be a contiguous int32 tensor of {S} x {n} x {Q} sums")
        exp = expected
    else:
        h = np.ascontiguousarray(np.asarray(expected).astype(np.uint32).reshape(S, n, Q))
        exp = torch.from_numpy(h.view(np.int32)).to(dev)
    if isinstance(out, int):
        out = torch.empty((out,), dtype=torch.uint8, device=dev)
    if out.dtype != torch.uint8 or not out.is_cuda or out.dim() != 1 or not out.is_contiguous():
        raise EcgError(ecg.ECG_EINVAL, "vread: out must be a contiguous 1-D uint8 CUDA tensor (or a byte count)")
    if max_len is None:
        max_len = B if rec is records else int(np.clip(ecg_dread._host_records(records)[:, 3], 0, B).max(initial=0))
    need = work_bytes(R, n)
    if work is None:
        work = torch.empty((max(need, 32),), dtype=torch.uint8, device=dev)
    elif work.dtype != torch.uint8 or not work.is_cuda or not work.is_contiguous() or work.numel() < need:
        raise EcgError(ecg.ECG_EINVAL, f"vread: work must be a contiguous uint8 CUDA tensor of at least {need} bytes")
    NP = max_pieces(max_len, piece_bytes, B)
    v = _checklib.result_tensor("vread", report, (R, 4), dev, "(R, 4)")
    sm = _checklib.result_tensor("vread", sums, (R, NP), dev, "(R, NP)")
    spare = torch.empty((1,), dtype=torch.int32, device=dev)
    # a tensor of no elements has no address: a spare word stands in, and its size keeps it unwritten
    out_ptr = out.data_ptr() if out.numel() else work.data_ptr()
    args = (ss, bs, B, S, None if flags is None else flags.data_ptr(), int(piece_bytes), exp.data_ptr(), rec.data_ptr(),
            R, int(max_len), out_ptr, int(out.numel()), work.data_ptr(), sm.data_ptr() if sm.numel() else spare.data_ptr(),
            v.data_ptr() if v.numel() else spare.data_ptr(), _stream(stream))
    return args, out, v, sm, (rec, flags, exp, work, spare)


def matrix_batch(H, src_ids, stripes, lost, piece_bytes, expected, records, out, max_len=None, work=None,
                 report=None, sums=None, stream=None):
    """H, src_ids, stripes, lost, records, out, max_len, work as ecg_dread.matrix_batch (lost may be None: nothing is
    lost); piece_bytes and expected as the module says (expected: host data or an int32 CUDA tensor of S * n * Q sums).
    Returns (out, report, sums)."""
    n = len(src_ids)
    H = np.asarray(H, dtype=np.int64).reshape(-1, n)
    args, out, v, sm, keep = _batch_args(n, stripes, lost, piece_bytes, expected, records, out, max_len, work, report,
                                         sums, stream)
    if v.shape[0] == 0:
        return out, v, sm
    _check(lib().ecg_vread_matrix_batch(n, H.shape[0], _ints(H.ravel()), _ints(src_ids), stripes.data_ptr(), *args),
           "vread.matrix_batch")
    return out, v, sm


def encode_batch(k, m, matrix, stripes, lost, piece_bytes, expected, records, out, max_len=None, work=None,
                 report=None, sums=None, stream=None):
    """H = [matrix | I] (matrix: m x k) over stripes [S][k+m][B].  Returns (out, report, sums)."""
    args, out, v, sm, keep = _batch_args(k + m, stripes, lost, piece_bytes, expected, records, out, max_len, work,
                                         report, sums, stream)
    if v.shape[0] == 0:
        return out, v, sm
    _check(lib().ecg_vread_encode_batch(k, m, _ints(matrix), stripes.data_ptr(), *args), "vread.encode_batch")
    return out, v, sm


def ec_batch(code, stripes, lost, piece_bytes, expected, records, out, max_len=None, work=None, report=None,
             sums=None, stream=None):
    """The class's own check matrix over stripes [S][k+m][B].  Returns (out, report, sums)."""
    args, out, v, sm, keep = _batch_args(code.k + code.m, stripes, lost, piece_bytes, expected, records, out, max_len,
                                         work, report, sums, stream)
    _check(ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, _stream(stream)), "set_memory")
    if v.shape[0] == 0:
        return out, v, sm
    _check(lib().ecg_vread_ec_batch(code._h, stripes.data_ptr(), *args), "vread.ec_batch")
    return out, v, sm


def check_records(records, n, B, S, max_len, out_bytes):
    """Host only: ecg_dread.check_records's rule through this library."""
    h = ecg_dread._host_records(records)
    rc = lib().ecg_vread_check_records(h.ctypes.data_as(LLP), h.shape[0], int(n), int(B), int(S), int(max_len),
                                       int(out_bytes))
    if rc < -1:
        _check(rc, "vread.check_records")
    return rc


def mismatched_rows(records, report, piece_bytes):
    """Host only: the sorted (stripe, q) pairs a repair starts from -- for every state-7 record the piece rows from its
    first bad piece to the end of its cover (the pieces before first_bad agree; which of a row's blocks is damaged is
    for ecg_psum.verify_batch over that stripe to say).  With block sums q is 0.  records, report: host data or
    tensors (copied back: that synchronises)."""
    rec = ecg_dread._host_records(records)
    rep = report.cpu().numpy() if isinstance(report, torch.Tensor) else np.asarray(report)
    rows = set()
    for (stripe, _, off, ln, _), (st, _, _, first) in zip(rec.tolist(), rep.reshape(-1, 4).tolist()):
        if st != MISMATCH:
            continue
        if piece_bytes == 0:
            rows.add((stripe, 0))
        else:
            rows.update((stripe, q) for q in range(first & 0xFFFFFFFF, (off + ln - 1) // piece_bytes + 1))
    return sorted(rows)


def counters():
    """Process-wide {launches, records}: main kernels launched and the records they covered."""
    v = [ctypes.c_longlong(0) for _ in range(2)]
    _check(lib().ecg_vread_counters(*[ctypes.byref(x) for x in v]), "vread.counters")
    return {"launches": v[0].value, "records": v[1].value}


def last_launch():
    """Geometry of the process's most recent main launch (include/ecg_vread.h ecg_vread_last_launch), all zero before
    the first."""
    f = lib().ecg_vread_last_launch
    n = f(None, 0)
    if n != len(LAST_LAUNCH_FIELDS):
        raise EcgError(ecg.ECG_EINVAL, f"vread.last_launch: library has {n} fields")
    v = (ctypes.c_int * n)()
    f(v, n)
    return dict(zip(LAST_LAUNCH_FIELDS, (int(x) for x in v)))
