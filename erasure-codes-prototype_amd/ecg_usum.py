"""Python binding of libecg_usum.so (include/ecg_usum.h): update sums, the recorded CRC-32C of blocks and pieces
carried through a delta update.

ecg_update changes len bytes of a data block and of the parities that depend on them; the sums a store keeps of those
blocks (ecg_sum per block, ecg_psum per piece) follow from the old sums and delta alone, because CRC-32C is linear.
`apply` takes the update's own G, records and delta (the `delta_out` of a WRITE call, or the `data_in` of a DELTA
call) and XORs every record's contribution into the store's sum table, an int32 CUDA tensor [S][n_sums][Q]: Q = 1
(piece_bytes = 0, the table ecg_sum.verify_batch takes) or Q = ceil(B / piece_bytes) (the table ecg_psum.verify_batch
takes).  The stripes are not an argument: nothing of them is read.

The report comes back as an int32 CUDA tensor of shape (R, 2), {state, nonzero} per record, asynchronously on torch's
current stream (or `stream`): the update's states, and the update's `changed`.

There is no CPU fallback for `apply`: if libecg_usum.so is missing or has no GPU to run on, it raises.  `expected` is
the library's host form of the same definition, on numpy arrays.
"""
from __future__ import annotations

import ctypes

import numpy as np

import _ecg_checklib as _checklib
import ecg
from _ecg_checklib import I, IP, LL, LLP, P
from ecg import EcgError, _check, _ints, _stream, torch

LIB_PATH = _checklib.lib_path("ecg_usum")

# Every symbol include/ecg_usum.h declares (checked by tests/test_usum_host.py).
EXPORTS = [
    "ecg_usum_matrix_batch", "ecg_usum_encode_batch", "ecg_usum_ec_batch", "ecg_usum_expected",
    "ecg_usum_traffic_bytes", "ecg_usum_counters", "ecg_usum_last_launch",
]

DATA, PARITY, BOTH = 1, 2, 3                                                  # `which`
APPLIED, BAD_STRIPE, BAD_COL, BAD_RANGE, TOO_LONG, BAD_STAGING = range(6)    # report[:, 0]
LAST_LAUNCH_FIELDS = ("cols_per_wg", "wg_per_record", "R", "max_nnz", "piece_bytes")

_UBP = ctypes.POINTER(ctypes.c_ubyte)
_HEAD = [LL, I, P, I, LL, P, LL]             # B, S, records, R, max_len, delta, in_bytes
_TAIL = [LL, I, P, P, P]                     # piece_bytes, which, sums, update_report, report
_SIG = {
    "ecg_usum_matrix_batch": ([I, I, IP, IP, IP] + _HEAD + [IP, I] + _TAIL + [P], I),
    "ecg_usum_encode_batch": ([I, I, IP] + _HEAD + _TAIL + [P], I),
    "ecg_usum_ec_batch": ([P] + _HEAD + _TAIL + [P], I),
    "ecg_usum_expected": ([I, I, IP, IP, IP] + _HEAD + [IP, I] + _TAIL, I),
    "ecg_usum_traffic_bytes": ([_UBP, LLP, I, LL, LL, I], LL),
    "ecg_usum_counters": ([LLP] * 2, I),
    "ecg_usum_last_launch": ([IP, I], I),
}

_L = None


def lib():
    """Load libecg_usum.so (after libecg.so, which it links against)."""
    global _L
    if _L is None:
        _L = _checklib.load(LIB_PATH, _SIG)
    return _L


def pieces(B, piece_bytes):
    """Q: sums per block."""
    return 1 if piece_bytes == 0 else (B + piece_bytes - 1) // piece_bytes


def _host_records(records):
    if torch is not None and isinstance(records, torch.Tensor):
        records = records.cpu().numpy()
    return np.ascontiguousarray(np.asarray(records, dtype=np.int64).reshape(-1, 5))


def _device_records(records, device):
    if torch is not None and isinstance(records, torch.Tensor) and records.is_cuda:
        if records.dtype != torch.int64 or records.dim() != 2 or records.shape[1] != 5 or not records.is_contiguous():
            raise EcgError(ecg.ECG_EINVAL, "usum: records must be a contiguous (R, 5) int64 tensor")
        return records
    return torch.from_numpy(_host_records(records)).to(device)


def apply(sums, records, delta, B, *, G=None, src_ids=None, dst_ids=None, sum_ids=None, k=None, m=None, matrix=None,
          code=None, piece_bytes=0, which=BOTH, max_len=None, update_report=None, out=None, stream=None):
    """XOR the records' contributions into sums, an int32 CUDA tensor [S][n_sums][Q] (changed in place).  The code is
    given in one of three forms:
      G, src_ids, dst_ids, sum_ids   m_out x k_in coefficients over named blocks; column c of sums is block sum_ids[c]
      k, m, matrix                   stripes of k + m blocks, data first; sums has k + m columns
      code                           an ErasureCode's own encoding matrix; sums has k + m columns
    records: (R, 5) int64 {stripe, col, off, len, in_off}, host data or a CUDA tensor; delta: 1-D uint8 CUDA tensor that
    holds delta at the records' staging ranges; B: the block size; max_len: the longest record (None: taken from host
    records, B for device records); update_report: the (R, 2) report of the update call, whose refused records then
    contribute nothing.  Returns the (R, 2) report."""
    if sums.dtype != torch.int32 or not sums.is_cuda or sums.dim() != 3 or not sums.is_contiguous():
        raise EcgError(ecg.ECG_EINVAL, "usum: sums must be a contiguous int32 CUDA tensor [S][n_sums][Q]")
    if delta.dtype != torch.uint8 or not delta.is_cuda or delta.dim() != 1 or not delta.is_contiguous():
        raise EcgError(ecg.ECG_EINVAL, "usum: delta must be a contiguous 1-D uint8 CUDA tensor")
    S, n_sums, Q = (int(v) for v in sums.shape)
    if Q != pieces(B, piece_bytes):
        raise EcgError(ecg.ECG_EINVAL, f"usum: sums has {Q} sums per block, B and piece_bytes give "
                                       f"{pieces(B, piece_bytes)}")
    rec = _device_records(records, sums.device)
    R = int(rec.shape[0])
    if max_len is None:
        max_len = B if rec is records else int(np.clip(_host_records(records)[:, 3], 0, B).max(initial=0))
    if update_report is not None and (tuple(update_report.shape) != (R, 2) or update_report.dtype != torch.int32
                                      or not update_report.is_cuda or not update_report.is_contiguous()):
        raise EcgError(ecg.ECG_EINVAL, "usum: update_report must be a contiguous int32 CUDA tensor of shape (R, 2)")
    v = _checklib.result_tensor("usum", out, (R, 2), sums.device, "(R, 2)")
    head = (int(B), S, rec.data_ptr(), R, int(max_len), delta.data_ptr(), int(delta.numel()))
    tail = (int(piece_bytes), int(which), sums.data_ptr(),
            None if update_report is None else update_report.data_ptr(), v.data_ptr(), _stream(stream))
    forms = (G is not None) + (matrix is not None) + (code is not None)
    if forms != 1:
        raise EcgError(ecg.ECG_EINVAL, "usum: give exactly one of G, matrix and code")
    if G is None and n_sums != (code.k + code.m if matrix is None else k + m):
        raise EcgError(ecg.ECG_EINVAL, f"usum: sums has {n_sums} columns, the stripes have k + m blocks")
    if code is not None:
        _check(ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, _stream(stream)), "set_memory")
    if R == 0:
        return v
    if G is not None:
        if len(sum_ids) != n_sums:
            raise EcgError(ecg.ECG_EINVAL, f"usum: sums has {n_sums} columns for {len(sum_ids)} sum_ids")
        k_in = len(src_ids)
        G = np.asarray(G, dtype=np.int64).reshape(-1, k_in)
        _check(lib().ecg_usum_matrix_batch(k_in, G.shape[0], _ints(G.ravel()), _ints(src_ids), _ints(dst_ids), *head,
                                           _ints(sum_ids), n_sums, *tail), "usum.matrix_batch")
    elif matrix is not None:
        _check(lib().ecg_usum_encode_batch(k, m, _ints(matrix), *head, *tail), "usum.encode_batch")
    else:
        _check(lib().ecg_usum_ec_batch(code._h, *head, *tail), "usum.ec_batch")
    return v


def expected(G, src_ids, dst_ids, sum_ids, sums, records, delta, B, piece_bytes=0, which=BOTH, max_len=None,
             update_report=None):
    """Host only (ecg_usum_expected): the same definition on numpy arrays.  sums: [S][n_sums][Q] integers, left as they
    are; delta: uint8 array; update_report: (R, 2) or None.  Returns (new sums as uint32 [S][n_sums][Q], report as
    uint32 (R, 2))."""
    k_in = len(src_ids)
    G = np.asarray(G, dtype=np.int64).reshape(-1, k_in)
    h = _host_records(records)
    R = int(h.shape[0])
    new = np.ascontiguousarray((np.asarray(sums).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32))
    S, n_sums, Q = new.shape
    if Q != pieces(B, piece_bytes) or n_sums != len(sum_ids):
        raise EcgError(ecg.ECG_EINVAL, "usum.expected: the shape of sums does not fit sum_ids, B and piece_bytes")
    dl = np.ascontiguousarray(delta, dtype=np.uint8)
    if max_len is None:
        max_len = int(np.clip(h[:, 3], 0, B).max(initial=0))
    up = None
    if update_report is not None:
        up = np.ascontiguousarray((np.asarray(update_report).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32))
        if up.shape != (R, 2):
            raise EcgError(ecg.ECG_EINVAL, "usum.expected: update_report must have shape (R, 2)")
    report = np.zeros((R, 2), np.uint32)
    one = np.zeros(1, np.uint8)                           # an empty array still has to be a pointer
    _check(lib().ecg_usum_expected(k_in, G.shape[0], _ints(G.ravel()), _ints(src_ids), _ints(dst_ids), int(B), S,
                                   (h if R else np.zeros((1, 5), np.int64)).ctypes.data, R, int(max_len),
                                   (dl if dl.size else one).ctypes.data, int(dl.size), _ints(sum_ids), n_sums,
                                   int(piece_bytes), int(which), new.ctypes.data,
                                   None if up is None else up.ctypes.data,
                                   (report if R else np.zeros((1, 2), np.uint32)).ctypes.data), "usum.expected")
    return new, report


def traffic_bytes(nnz_per_col, records, B, piece_bytes=0, which=BOTH):
    """Host only: the bytes the records move by the definition: len of delta read, and 8 bytes per sum word met."""
    h = _host_records(records)
    nnz = np.ascontiguousarray(nnz_per_col, dtype=np.uint8)
    if h.shape[0] and (h[:, 1].min() < 0 or h[:, 1].max() >= nnz.size):
        raise EcgError(ecg.ECG_EINVAL, "usum.traffic_bytes: a record's col has no entry in nnz_per_col")
    return _check(lib().ecg_usum_traffic_bytes(nnz.ctypes.data_as(_UBP), h.ctypes.data_as(LLP), h.shape[0], int(B),
                                               int(piece_bytes), int(which)), "usum.traffic_bytes")


def counters():
    """Process-wide {launches, records}: usum kernels launched and the records they covered."""
    v = [ctypes.c_longlong(0) for _ in range(2)]
    _check(lib().ecg_usum_counters(*[ctypes.byref(x) for x in v]), "usum.counters")
    return {"launches": v[0].value, "records": v[1].value}


def last_launch():
    """Geometry of the process's most recent usum launch (include/ecg_usum.h ecg_usum_last_launch), all zero before
    the first."""
    f = lib().ecg_usum_last_launch
    n = f(None, 0)
    if n != len(LAST_LAUNCH_FIELDS):
        raise EcgError(ecg.ECG_EINVAL, f"usum.last_launch: library has {n} fields")
    v = (ctypes.c_int * n)()
    f(v, n)
    return dict(zip(LAST_LAUNCH_FIELDS, (int(x) for x in v)))
