"""Python binding of libecg_restore.so (include/ecg_restore.h): named-block restoration, the step after a checksum
verify that says "more than one".

For a check matrix H (r x n, r <= 8, n <= 128) every selected stripe brings its own set E of flagged blocks, a row of
n uint8 flags on the device.  Where 1 <= |E| <= r and the columns H[:, E] are independent (state 0), every bad byte
position (nonzero syndrome s[x] = H * v[x]) at which H_E * e = s[x] has a solution is corrected in place: byte x of
block b becomes v_b[x] ^ e_b for the b in E with e_b != 0.  A position the flagged blocks cannot explain is left alone;
so is every stripe with no flag (state 1), more than r flags (state 2) or dependent flagged columns (state 3).  Per
stripe

    report[b]     = positions corrected in block b,                                  b < n
    report[n]     = bad positions
    report[n + 1] = bad positions left untouched
    report[n + 2] = the state

comes back as an int32 CUDA tensor of shape (S_sel, n + 3), asynchronously on torch's current stream (or `stream`).
The stripes (torch uint8 CUDA tensors) are WRITTEN, only where a byte is corrected; the stripe ids of one call must be
distinct.  include/ecg_restore.h states what the spare check rows guard against and where that guard ends (t = r).

`names_from_sums` makes the flags from a verify's sums on the device, `rows` turns them into the views and vectors the
batch forms take, a piece row being a stripe of P-byte blocks.

There is no CPU fallback: if libecg_restore.so is missing or has no GPU to run on, calls raise.
"""
from __future__ import annotations

import numpy as np

import _ecg_checklib as _checklib
import ecg
from _ecg_checklib import I, IP, LL, LLP, P, PP, LAST_LAUNCH_FIELDS  # LAST_LAUNCH_FIELDS: re-exported
from ecg import EcgError, _check, _ints, _ptrs, _stream, _strides, torch

LIB_PATH = _checklib.lib_path("ecg_restore")

# Every symbol include/ecg_restore.h declares (checked by tests/test_restore_host.py).
EXPORTS = [
    "ecg_restore_matrix_batch", "ecg_restore_encode_batch", "ecg_restore_ec_batch", "ecg_restore_ec",
    "ecg_restore_work_bytes", "ecg_restore_names_from_sums", "ecg_restore_counters", "ecg_restore_last_launch",
]

USABLE, NONE_FLAGGED, TOO_MANY, DEPENDENT = 0, 1, 2, 3  # report[n + 2]

_SIG = {
    "ecg_restore_matrix_batch": ([I, I, IP, IP, P, LL, LL, LL, P, P, I, P, P, P], I),
    "ecg_restore_encode_batch": ([I, I, IP, P, LL, LL, LL, P, P, I, P, P, P], I),
    "ecg_restore_ec_batch": ([P, P, LL, LL, LL, P, P, I, P, P, P], I),
    "ecg_restore_ec": ([P, PP, PP, I, P, P], I),
    "ecg_restore_work_bytes": ([I], LL),
    "ecg_restore_names_from_sums": ([I, I, P, P, I, P, P, P], I),
    "ecg_restore_counters": ([LLP] * 2, I),
    "ecg_restore_last_launch": ([IP, I], I),
}

_L = None


def lib():
    """Load libecg_restore.so (after libecg.so, which it links against)."""
    global _L
    if _L is None:
        _L = _checklib.load(LIB_PATH, _SIG)
    return _L


def work_bytes(S_sel):
    """Bytes of device scratch the batch forms need for S_sel selected stripes."""
    v = int(lib().ecg_restore_work_bytes(int(S_sel)))
    if v < 0:
        _check(v, "restore.work_bytes")
    return v


def _selection(stripe_ids, S):
    return (None, S) if stripe_ids is None else _checklib.int32_vector("restore", stripe_ids, "stripe_ids")


def _named(named, S_sel, n):
    if (tuple(named.shape) != (S_sel, n) or named.dtype != torch.uint8 or not named.is_cuda
            or not named.is_contiguous()):
        raise EcgError(ecg.ECG_EINVAL, "restore: named must be a contiguous uint8 CUDA tensor of shape (S_sel, n)")
    return named.data_ptr()


def _work(work, S_sel, device):
    """The scratch tensor: `work` if given (checked), else a fresh one."""
    need = work_bytes(S_sel)
    if work is None:
        return torch.empty((max(need, 32),), dtype=torch.uint8, device=device)
    if work.dtype != torch.uint8 or not work.is_cuda or not work.is_contiguous() or work.numel() < need:
        raise EcgError(ecg.ECG_EINVAL, f"restore: work must be a contiguous uint8 CUDA tensor of {need} bytes or more")
    return work


def _report(out, S_sel, n, device):
    return _checklib.result_tensor("restore", out, (S_sel, n + 3), device, "(S_sel, n + 3)")


def matrix_batch(H, src_ids, stripes, named, stripe_ids=None, work=None, out=None, stream=None):
    """H: r x n check matrix (nested or flat); src_ids: the n block indices its columns stand for; stripes: [S][*][B]
    uint8 CUDA tensor view (any strides), corrected in place; named: (S_sel, n) uint8 CUDA flags, row i for stripe
    stripe_ids[i]; work: uint8 CUDA scratch of work_bytes(S_sel) (None: allocated here; it must outlive the launch,
    which torch's caching allocator sees to on the current stream; pass your own with another `stream`).  Returns the
    (S_sel, n + 3) report; report[:, j], and flag j, are block src_ids[j]."""
    n = len(src_ids)
    H = np.asarray(H, dtype=np.int64).reshape(-1, n)
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    ids, S_sel = _selection(stripe_ids, S)
    w = _work(work, S_sel, stripes.device)
    v = _report(out, S_sel, n, stripes.device)
    if S_sel == 0 or B == 0:
        return v.zero_()                             # nothing to read: no call (an empty tensor has no address)
    _check(lib().ecg_restore_matrix_batch(n, H.shape[0], _ints(H.ravel()), _ints(src_ids), stripes.data_ptr(), ss, bs,
                                          B, ids, _named(named, S_sel, n), S_sel, w.data_ptr(), v.data_ptr(),
                                          _stream(stream)), "restore.matrix_batch")
    return v


def encode_batch(k, m, matrix, stripes, named, stripe_ids=None, work=None, out=None, stream=None):
    """H = [matrix | I] over stripes [S][k+m][B] (data 0..k-1, coding k..k+m-1), corrected in place.  Returns the
    (S_sel, k+m+3) report."""
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    ids, S_sel = _selection(stripe_ids, S)
    w = _work(work, S_sel, stripes.device)
    v = _report(out, S_sel, k + m, stripes.device)
    if S_sel == 0 or B == 0:
        return v.zero_()                             # nothing to read: no call (an empty tensor has no address)
    _check(lib().ecg_restore_encode_batch(k, m, _ints(matrix), stripes.data_ptr(), ss, bs, B, ids,
                                          _named(named, S_sel, k + m), S_sel, w.data_ptr(), v.data_ptr(),
                                          _stream(stream)), "restore.encode_batch")
    return v


def ec_batch(code, stripes, named, stripe_ids=None, work=None, out=None, stream=None):
    """The class's own check (ErasureCode.check_matrix) over stripes [S][k+m][B], corrected in place.  Returns the
    (S_sel, k+m+3) report."""
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    ids, S_sel = _selection(stripe_ids, S)
    w = _work(work, S_sel, stripes.device)
    v = _report(out, S_sel, code.k + code.m, stripes.device)
    if S_sel == 0 or B == 0:
        return v.zero_()                             # nothing to read: no call (an empty tensor has no address)
    _check(ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, _stream(stream)), "set_memory")
    _check(lib().ecg_restore_ec_batch(code._h, stripes.data_ptr(), ss, bs, B, ids,
                                      _named(named, S_sel, code.k + code.m), S_sel, w.data_ptr(), v.data_ptr(),
                                      _stream(stream)), "restore.ec_batch")
    return v


def ec(code, data_ptrs, coding_ptrs, block_size, named, out=None, stream=None):
    """One stripe through its block pointers (lists of uint8 CUDA tensors), on the handle's stream; named: k + m host
    flags (a sequence or numpy array).  Solved on the host.  Returns the (1, k+m+3) report."""
    n = code.k + code.m
    flags = np.ascontiguousarray(np.asarray(named).reshape(-1) != 0, dtype=np.uint8)
    if flags.size != n:
        raise EcgError(ecg.ECG_EINVAL, f"restore.ec: {flags.size} flags for {n} blocks")
    code._bind(list(data_ptrs) + list(coding_ptrs), stream)
    v = _report(out, 1, n, data_ptrs[0].device)
    _check(lib().ecg_restore_ec(code._h, _ptrs(data_ptrs), _ptrs(coding_ptrs), block_size, flags.ctypes.data,
                                v.data_ptr()), "restore.ec")
    return v


def names_from_sums(sums, expected, stream=None):
    """sums, expected: (S_sel, n, Q) int32 CUDA tensors of a piece verify, or (S_sel, n) of a block verify (Q = 1).
    Returns (named, count): (S_sel, Q, n) uint8 flags, 1 where the two differ, and (S_sel, Q) int32 flags per piece
    row.  Stays on the device."""
    if sums.dim() == 2:
        sums, expected = sums.unsqueeze(2), expected.unsqueeze(2)
    for t in (sums, expected):
        if t.dim() != 3 or t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous():
            raise EcgError(ecg.ECG_EINVAL, "restore.names_from_sums: sums and expected must be contiguous int32 CUDA "
                                           "tensors of shape (S_sel, n, Q) or (S_sel, n)")
    if tuple(sums.shape) != tuple(expected.shape):
        raise EcgError(ecg.ECG_EINVAL, "restore.names_from_sums: sums and expected differ in shape")
    S_sel, n, Q = sums.shape
    named = torch.empty((S_sel, Q, n), dtype=torch.uint8, device=sums.device)
    count = torch.empty((S_sel, Q), dtype=torch.int32, device=sums.device)
    if S_sel == 0 or Q == 0:
        return named, count
    _check(lib().ecg_restore_names_from_sums(n, Q, sums.data_ptr(), expected.data_ptr(), S_sel, named.data_ptr(),
                                             count.data_ptr(), _stream(stream)), "restore.names_from_sums")
    return named, count


def rows(stripes, sums, expected, piece_bytes, stripe_ids=None):
    """The bridge from a verify to the restore.  stripes: the [S][n][B] view the verify ran over; sums, expected: the
    verify's sums and the recorded ones, (S_sel, n, Q) for piece sums of piece_bytes = P, or (S_sel, n) with
    piece_bytes None for block sums (one piece: the block); stripe_ids: the verify's selection (distinct ids), None =
    all stripes in order.  Synchronises (it reads the flag counts on the host).

    Returns a list of (view, row_ids, row_named): `view` is a [rows][n][len] uint8 view of the stripes' memory whose
    "stripes" are piece rows, row_ids (int32 CUDA) the rows in which at least one column differs, row_named (uint8
    CUDA, one row of n flags each) their flagged sets, for *_batch(view, row_named, stripe_ids=row_ids).  Rows with no
    differing column are not listed.

    The three cases are those of ecg_psum.heal_rows: when the stripe stride is a multiple of piece_bytes, the full
    pieces of all stripes are one view with row stride piece_bytes, row id stripe * (stride / piece_bytes) + q.  A
    ragged last piece is an entry of its own, of length B - (Q - 1) piece_bytes.  With any other stride there is one
    entry per piece index that has a flagged row."""
    S, n, B = stripes.shape
    named, count = names_from_sums(sums, expected)
    S_sel, Q = count.shape
    if named.shape[2] != n:
        raise EcgError(ecg.ECG_EINVAL, f"restore.rows: sums over {named.shape[2]} columns for stripes of {n} blocks")
    if piece_bytes is None:
        if Q != 1:
            raise EcgError(ecg.ECG_EINVAL, "restore.rows: piece sums need their piece_bytes")
        P_ = max(int(B), 1)
        full = 0 if B == 0 else 1
    else:
        import ecg_psum
        P_ = int(piece_bytes)
        if Q != ecg_psum.pieces(B, P_):
            raise EcgError(ecg.ECG_EINVAL, f"restore.rows: {Q} sums per block for B = {B}, piece_bytes = {P_}")
        full = B // P_                                                   # pieces of P bytes; piece `full` is ragged
    c = count.cpu().numpy()                                              # synchronises
    sid = np.arange(S, dtype=np.int64) if stripe_ids is None else stripe_ids.cpu().numpy().astype(np.int64)
    if sid.shape[0] != S_sel:
        raise EcgError(ecg.ECG_EINVAL, f"restore.rows: {S_sel} rows of sums for {sid.shape[0]} selected stripes")
    if sid.size and (sid.min() < 0 or sid.max() >= S):
        raise EcgError(ecg.ECG_EINVAL, "restore.rows: a stripe id lies outside the stripes")
    flagged = c > 0
    ss, bs = _strides(stripes)
    dev = stripes.device

    def entry(make_view, row_ids, i, q):
        if row_ids.max() >= 1 << 31:
            raise EcgError(ecg.ECG_EINVAL, f"restore.rows: row id {int(row_ids.max())} does not fit an int32")
        pick = named[torch.as_tensor(i, device=dev), torch.as_tensor(q, device=dev)].contiguous()
        return make_view(), torch.tensor(row_ids, dtype=torch.int32, device=dev), pick

    out = []
    if full > 0 and ss > 0 and ss % P_ == 0:
        i, q = np.nonzero(flagged[:, :full])
        if i.size:
            per = ss // P_
            out.append(entry(lambda: torch.as_strided(stripes, ((S - 1) * per + full, n, P_), (P_, bs, 1),
                                                      stripes.storage_offset()), sid[i] * per + q, i, q))
    else:
        for q in range(full):
            i = np.nonzero(flagged[:, q])[0]
            if i.size:
                out.append(entry(lambda: stripes[:, :, q * P_:(q + 1) * P_], sid[i], i, np.full_like(i, q)))
    if full < Q:
        i = np.nonzero(flagged[:, full])[0]
        if i.size:
            out.append(entry(lambda: stripes[:, :, full * P_:], sid[i], i, np.full_like(i, full)))
    return out


def counters():
    """Process-wide {launches, bytes}: restore kernels launched and the bytes they read as planned (S_sel * B * n)."""
    return _checklib.counters(lib(), "restore")


def last_launch():
    """Geometry of the process's most recent vector-path restore launch, as placed in the launch descriptor after the
    fallbacks (include/ecg_restore.h ecg_restore_last_launch): {grid_map, map_group, cols_per_wg, wg_per_stripe, S,
    rtiles}, all zero before the first.  Byte-kernel launches do not change it."""
    return _checklib.last_launch(lib(), "restore")
