"""Python binding of libecg_psum.so (include/ecg_psum.h): piece checksums, CRC-32C of every fixed-size piece of every
stored block.

    sums[i][j][q] = crc32c(bytes [q P, min((q + 1) P, B)) of block src_ids[j] of stripe stripe_ids[i])

over HBM-resident stripes (torch uint8 CUDA tensors), P = piece_bytes a power of two in [512, 2^30], Q = ceil(B / P).
Every byte is read once and nothing is written but the outputs.  Sums come back as an int32 CUDA tensor of shape
(S_sel, n, Q) holding the 32-bit values (`& 0xFFFFFFFF` on the host), asynchronously on torch's current stream (or
`stream`).  `verify_batch` compares them with recorded sums and returns (sums, targets, bad), targets and bad of shape
(S_sel, Q): one verdict per piece row.  `heal_rows` turns those targets into the views and vectors that ecg_heal's
TARGET and ecg_heal2's TARGET2 forms take, a piece row being a stripe of P-byte blocks.

There is no CPU fallback for the device calls: if libecg_psum.so is missing or has no GPU to run on, they raise.
`fold` is a host function over host sums.
"""
from __future__ import annotations

import ctypes

import numpy as np

import _ecg_checklib as _checklib
import ecg
from _ecg_checklib import I, IP, LL, LLP, P, PP
from ecg import EcgError, _check, _ints, _ptrs, _stream, _strides, torch

LIB_PATH = _checklib.lib_path("ecg_psum")
U = ctypes.c_uint

# Every symbol include/ecg_psum.h declares (checked by tests/test_psum_host.py).
EXPORTS = [
    "ecg_psum_pieces_batch", "ecg_psum_verify_batch", "ecg_psum_ec_batch", "ecg_psum_verify_ec_batch", "ecg_psum_ec",
    "ecg_psum_fold", "ecg_psum_counters", "ecg_psum_last_launch", "ecg_psum_set_span_bytes",
]

_SIG = {
    "ecg_psum_pieces_batch": ([I, IP, P, LL, LL, LL, LL, P, I, P, P], I),
    "ecg_psum_verify_batch": ([I, IP, P, LL, LL, LL, LL, P, I, P, P, P, P, P], I),
    "ecg_psum_ec_batch": ([P, P, LL, LL, LL, LL, P, I, P, P], I),
    "ecg_psum_verify_ec_batch": ([P, P, LL, LL, LL, LL, P, I, P, P, P, P, P], I),
    "ecg_psum_ec": ([P, PP, PP, I, LL, P], I),
    "ecg_psum_fold": ([P, LL, LL, LL], U),
    "ecg_psum_counters": ([LLP] * 2, I),
    "ecg_psum_last_launch": ([IP, I], I),
    "ecg_psum_set_span_bytes": ([LL], I),
}

# The fields of ecg_psum_last_launch, in order.
LAST_LAUNCH_FIELDS = ("path", "piece_bytes", "pieces_per_block", "blocks", "span_bytes")
PATH_VECTOR, PATH_BYTE = 0, 1
MIN_PIECE, MAX_PIECE = 512, 1 << 30

_L = None


def lib():
    """Load libecg_psum.so (after libecg.so, which it links against)."""
    global _L
    if _L is None:
        _L = _checklib.load(LIB_PATH, _SIG)
    return _L


def pieces(B, piece_bytes):
    """Q = ceil(B / piece_bytes); refuses a piece_bytes the library would refuse."""
    P_ = int(piece_bytes)
    if P_ < MIN_PIECE or P_ > MAX_PIECE or P_ & (P_ - 1):
        raise EcgError(ecg.ECG_EINVAL, f"psum: piece_bytes = {P_} is not a power of two in [512, 2^30]")
    return -(-int(B) // P_)


def _selection(stripe_ids, S):
    return (None, S) if stripe_ids is None else _checklib.int32_vector("psum", stripe_ids, "stripe_ids")


def _sums(out, S_sel, n, Q, device):
    return _checklib.result_tensor("psum", out, (S_sel, n, Q), device, "(S_sel, n, Q)")


def _expected(expected, S_sel, n, Q):
    if (tuple(expected.shape) != (S_sel, n, Q) or expected.dtype != torch.int32 or not expected.is_cuda
            or not expected.is_contiguous()):
        raise EcgError(ecg.ECG_EINVAL, "psum: expected must be a contiguous int32 CUDA tensor of shape (S_sel, n, Q)")
    return expected.data_ptr()


def _verdicts(S_sel, Q, device):
    return (torch.empty((S_sel, Q), dtype=torch.int32, device=device),
            torch.empty((S_sel, Q), dtype=torch.int32, device=device))


def pieces_batch(src_ids, stripes, piece_bytes, stripe_ids=None, out=None, stream=None):
    """src_ids: the n block indices to sum; stripes: [S][*][B] uint8 CUDA tensor view (any strides); stripe_ids: int32
    CUDA vector of the stripes to sum (None: all, in order; duplicates allowed).  Returns the (S_sel, n, Q) sums."""
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    ids, S_sel = _selection(stripe_ids, S)
    v = _sums(out, S_sel, len(src_ids), pieces(B, piece_bytes), stripes.device)
    _check(lib().ecg_psum_pieces_batch(len(src_ids), _ints(src_ids), stripes.data_ptr(), ss, bs, B, int(piece_bytes),
                                       ids, S_sel, v.data_ptr(), _stream(stream)), "psum.pieces_batch")
    return v


def verify_batch(src_ids, stripes, piece_bytes, expected, stripe_ids=None, out=None, stream=None):
    """pieces_batch, then the compare with `expected` ((S_sel, n, Q) int32 CUDA, row i for stripe stripe_ids[i]).
    Returns (sums, targets, bad): targets[i][q] is -1 (no column of piece row (i, q) differs), j (exactly column j) or
    n (more than one); bad[i][q] counts the columns that differ."""
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    ids, S_sel = _selection(stripe_ids, S)
    n, Q = len(src_ids), pieces(B, piece_bytes)
    v = _sums(out, S_sel, n, Q, stripes.device)
    targets, bad = _verdicts(S_sel, Q, stripes.device)
    _check(lib().ecg_psum_verify_batch(n, _ints(src_ids), stripes.data_ptr(), ss, bs, B, int(piece_bytes), ids, S_sel,
                                       _expected(expected, S_sel, n, Q), v.data_ptr(), targets.data_ptr(),
                                       bad.data_ptr(), _stream(stream)), "psum.verify_batch")
    return v, targets, bad


def ec_batch(code, stripes, piece_bytes, stripe_ids=None, out=None, stream=None):
    """All k + m blocks of the code's stripes [S][k+m][B].  Returns the (S_sel, k + m, Q) sums."""
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    ids, S_sel = _selection(stripe_ids, S)
    v = _sums(out, S_sel, code.k + code.m, pieces(B, piece_bytes), stripes.device)
    _check(ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, _stream(stream)), "set_memory")
    _check(lib().ecg_psum_ec_batch(code._h, stripes.data_ptr(), ss, bs, B, int(piece_bytes), ids, S_sel, v.data_ptr(),
                                   _stream(stream)), "psum.ec_batch")
    return v


def verify_ec_batch(code, stripes, piece_bytes, expected, stripe_ids=None, out=None, stream=None):
    """ec_batch, then the compare: (sums, targets, bad) as verify_batch."""
    S, _, B = stripes.shape
    ss, bs = _strides(stripes)
    ids, S_sel = _selection(stripe_ids, S)
    n, Q = code.k + code.m, pieces(B, piece_bytes)
    v = _sums(out, S_sel, n, Q, stripes.device)
    targets, bad = _verdicts(S_sel, Q, stripes.device)
    _check(ecg.lib().ecg_ec_set_memory(code._h, ecg.ECG_MEM_DEVICE, _stream(stream)), "set_memory")
    _check(lib().ecg_psum_verify_ec_batch(code._h, stripes.data_ptr(), ss, bs, B, int(piece_bytes), ids, S_sel,
                                          _expected(expected, S_sel, n, Q), v.data_ptr(), targets.data_ptr(),
                                          bad.data_ptr(), _stream(stream)), "psum.verify_ec_batch")
    return v, targets, bad


def ec(code, data_ptrs, coding_ptrs, block_size, piece_bytes, out=None, stream=None):
    """One stripe through its block pointers (lists of uint8 CUDA tensors), on the handle's stream.  Returns the
    (1, k + m, Q) sums."""
    code._bind(list(data_ptrs) + list(coding_ptrs), stream)
    v = _sums(out, 1, code.k + code.m, pieces(block_size, piece_bytes), data_ptrs[0].device)
    _check(lib().ecg_psum_ec(code._h, _ptrs(data_ptrs), _ptrs(coding_ptrs), block_size, int(piece_bytes),
                             v.data_ptr()), "psum.ec")
    return v


def fold(piece_sums, piece_bytes, B):
    """crc32c of a block of B bytes from its Q piece sums (a host sequence or numpy array of 32-bit values), on the
    CPU: what ecg_sum.blocks_batch gives for the block."""
    a = np.ascontiguousarray(np.asarray(piece_sums).reshape(-1).astype(np.int64) & 0xFFFFFFFF, dtype=np.uint32)
    if a.size != pieces(B, piece_bytes) or B < 0:
        raise EcgError(ecg.ECG_EINVAL, f"psum.fold: {a.size} sums for B = {B}, piece_bytes = {piece_bytes}")
    return int(lib().ecg_psum_fold(a.ctypes.data, a.size, int(piece_bytes), int(B))) if a.size else 0


def heal_rows(stripes, targets, piece_bytes, stripe_ids=None, columns=None):
    """The bridge from a piece verify to the heal.  stripes: the [S][n][B] view the verify ran over; targets: the
    verify's (S_sel, Q) tensor; stripe_ids: the verify's selection (distinct ids), None = all stripes in order;
    columns: the number of columns the verify compared when it ran over src_ids = 0..columns-1 with columns < n (its
    "more than one" is then `columns`, which must not be read as a block), None = n.  Synchronises (it reads
    `targets` on the host).

    Returns a list of (view, row_ids, row_targets): `view` is a [rows][n][len] uint8 view of the stripes' memory whose
    "stripes" are piece rows, row_ids (int32 CUDA) the rows whose target names a block, row_targets (int32 CUDA) those
    targets, for ecg_heal.*_batch(view, stripe_ids=row_ids, targets=row_targets) and ecg_heal2's TARGET2 forms.
    Rows whose target is -1 or n are not listed: the heal would leave them unwritten anyway.

    When the stripe stride is a multiple of piece_bytes, the full pieces of all stripes are one view with row stride
    piece_bytes, row id stripe * (stride / piece_bytes) + q.  A ragged last piece is an entry of its own, of length
    B - (Q - 1) piece_bytes.  With any other stride there is one entry per piece index that has a target."""
    S, n, B = stripes.shape
    P_ = int(piece_bytes)
    Q = pieces(B, P_)
    if targets.dim() != 2 or targets.shape[1] != Q or targets.dtype != torch.int32:
        raise EcgError(ecg.ECG_EINVAL, "psum.heal_rows: targets must be the (S_sel, Q) int32 tensor of a verify")
    t = targets.cpu().numpy()                                            # synchronises
    sid = np.arange(S, dtype=np.int64) if stripe_ids is None else stripe_ids.cpu().numpy().astype(np.int64)
    if sid.shape[0] != t.shape[0]:
        raise EcgError(ecg.ECG_EINVAL, f"psum.heal_rows: {t.shape[0]} target rows for {sid.shape[0]} selected stripes")
    if sid.size and (sid.min() < 0 or sid.max() >= S):
        raise EcgError(ecg.ECG_EINVAL, "psum.heal_rows: a stripe id lies outside the stripes")
    named = (t >= 0) & (t < (n if columns is None else min(int(columns), n)))
    ss, bs = _strides(stripes)
    full = B // P_                                                       # pieces of P bytes; piece `full` is ragged

    def entry(make_view, rows, tg):
        if rows.max() >= 1 << 31:
            raise EcgError(ecg.ECG_EINVAL, f"psum.heal_rows: row id {int(rows.max())} does not fit an int32")
        dev = stripes.device
        return (make_view(), torch.tensor(rows, dtype=torch.int32, device=dev),
                torch.tensor(tg, dtype=torch.int32, device=dev))

    out = []
    if full > 0 and ss > 0 and ss % P_ == 0:
        i, q = np.nonzero(named[:, :full])
        if i.size:
            per = ss // P_
            out.append(entry(lambda: torch.as_strided(stripes, ((S - 1) * per + full, n, P_), (P_, bs, 1),
                                                      stripes.storage_offset()), sid[i] * per + q, t[i, q]))
    else:
        for q in range(full):
            i = np.nonzero(named[:, q])[0]
            if i.size:
                out.append(entry(lambda: stripes[:, :, q * P_:(q + 1) * P_], sid[i], t[i, q]))
    if full < Q:
        i = np.nonzero(named[:, full])[0]
        if i.size:
            out.append(entry(lambda: stripes[:, :, full * P_:], sid[i], t[i, full]))
    return out


def counters():
    """Process-wide {launches, bytes}: kernels launched and the bytes they read as planned (S_sel * n * B per call)."""
    return _checklib.counters(lib(), "psum")


def last_launch():
    """Geometry of the most recent call's main launch (include/ecg_psum.h ecg_psum_last_launch): {path, piece_bytes,
    pieces_per_block, blocks, span_bytes}, all zero before the first."""
    f = lib().ecg_psum_last_launch
    n = f(None, 0)
    if n != len(LAST_LAUNCH_FIELDS):
        raise EcgError(ecg.ECG_EINVAL, f"psum.last_launch: library has {n} fields")
    v = (ctypes.c_int * n)()
    f(v, n)
    return dict(zip(LAST_LAUNCH_FIELDS, (int(x) for x in v)))


def set_span_bytes(nbytes):
    """Bytes of a block per workgroup on the vector path, process-wide: 0 = auto, else a multiple of 2048."""
    _check(lib().ecg_psum_set_span_bytes(int(nbytes)), "psum.set_span_bytes")
