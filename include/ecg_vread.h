/*
 * ecg_vread.h — verified range reads on the MI355X (gfx950): answer byte ranges of stored blocks, rebuilding the ranges
 * of lost blocks from the survivors, and check every answer against the store's recorded CRC-32C (libecg_vread.so).
 *
 * ecg_dread.h answers byte ranges of a store that has lost blocks, but takes the survivors as good: a damaged survivor
 * gives a wrong answer with state 0.  A store that records a CRC-32C per block (ecg_sum.h) or per piece (ecg_psum.h),
 * and keeps it current through overwrites (ecg_usum.h), verifies the recorded sum of every piece a read touches, on
 * every read, healthy or degraded.  This call is that read: one call answers R ranges and says, per record, whether the
 * bytes agree with what the store recorded.  With no block lost it is the ordinary verified read.
 *
 * Definition.  Everything is as in ecg_dread.h -- H (r x n, r <= 8, n <= 128), src_ids and the strided layout, d_lost,
 * the records {stripe, col, off, len, out_off}, max_len, d_out, out_bytes, and the plan rule, bit for bit that of
 * ecg_dread_plan -- with one relaxation and two more inputs:
 *   d_lost        [S][n] as there; NULL means that no column is lost in any stripe.
 *   piece_bytes   0 means block sums: Q = 1, the table layout of ecg_sum_verify_batch.  Otherwise a power of two P in
 *                 [512, 2^30]: Q = ceil(B / P), the table layout of ecg_psum_verify_batch; the last piece is the
 *                 shorter one.  The convention of ecg_usum.h.
 *   d_expected    [S][n][Q] (unsigned, device): the store's recorded CRC-32C table.  Row s is stripe number s, column j
 *                 is column j of H.  The sums of lost blocks are still in it: a store loses a node, not its metadata.
 *
 * Covering pieces.  An answered record with len > 0 covers pieces q0 = off / P .. q1 = (off + len - 1) / P of its
 * block, the bytes [q0 * P, min((q1 + 1) * P, B)); with piece_bytes == 0 it covers the whole block.  For every covering
 * piece the call computes the value of column `col` over the WHOLE piece -- a present column is copied, a lost one is
 * XOR c_j * v_j over the plan's sources --, takes its CRC-32C (the definition of ecg_sum.h) and compares it with
 * d_expected[stripe][col][q].  Only bytes [off, off + len) are stored to d_out; the rest of the cover lives in
 * registers and is never stored.
 *
 * Bytes read.  A record reads  reads * (bytes of its covering pieces),  not reads * len: that is inherent to
 * verification against per-piece sums.  A 3-byte read that straddles a piece boundary reads two whole pieces of every
 * source; with block sums every record reads whole blocks.  ecg_vread_cover computes the cover of a range on the host.
 *
 * Report.  d_report[R][4] (unsigned), zeroed by the call, holds {state, reads, bad, first_bad}.  The state is the first
 * of these that applies:
 *         0  answered, every covering piece's sum agrees
 *         1  stripe not in [0, S)
 *         2  col not in [0, n)
 *         3  off < 0, len < 0 or off + len > B
 *         4  len > max_len
 *         5  out_off < 0 or out_off + len > out_bytes
 *         6  col is lost and not recoverable from the survivors
 *         7  answered, but the sum of at least one covering piece differs from the recorded one
 * States 1-6 are ecg_dread.h's: a refused record reads no block, writes no byte of d_out, and reports reads = 0,
 * bad = 0, first_bad = 0xFFFFFFFF.  `bad` is the number of covering pieces whose sum differs; first_bad is the index q
 * of the first such piece within the block, 0xFFFFFFFF when there is none.  A record with len == 0 is answered with no
 * piece covered: bad = 0, and reads as in ecg_dread.h.
 *
 * THE BYTES OF A STATE-7 RECORD ARE STORED TO d_out.  The pieces of one record are folded by several workgroups of one
 * launch, so the verdict is known only after the bytes have gone out.  A caller reads the report BEFORE it uses the
 * bytes, and treats the range of a state-7 record as garbage.
 *
 * Sums.  d_sums[R][NP] (unsigned, required, zeroed by the call) receives the computed sums of each record's covering
 * pieces in order: d_sums[i][p] is piece q0 + p of record i.  NP = ecg_vread_max_pieces(max_len, piece_bytes, B), the
 * most pieces a record of max_len bytes can cover; entries past a record's pieces, and the rows of refused records,
 * stay 0.
 *
 * Guarantees.  No byte of the stripes is ever stored to.  No byte of d_out outside an answered record's range is stored
 * to.  Blocks in E are never read.  d_expected is only read.  The out ranges of one call must be pairwise disjoint
 * (ecg_vread_check_records checks that on the host).
 *
 * Not promised: which survivor is bad.  State 7 on a degraded read says that the fold of the survivors is not what was
 * recorded for the lost block; ecg_psum_verify_batch (or ecg_sum_verify_batch) over that stripe names the damaged
 * block, and ecg_heal.h or ecg_restore.h repairs it.
 *
 * Limits.  ECG_EINVAL with ecg_last_error() set, before any device is touched, for everything ecg_dread.h refuses (a
 * NULL d_lost excepted) and for:
 *   - a piece_bytes that is neither 0 nor a power of two in [512, 2^30];
 *   - a NULL d_expected, d_sums or d_report (or one that is not 4-byte aligned);
 *   - R * NP >= 2^31;
 *   - a launch that would need more than 2^31 - 1 workgroups (R * ceil(largest cover / span), see below).
 * R == 0 is a no-op returning 0.  With max_len == 0 no byte can move and NP is 0: the call still fills the report.
 *
 * The launches.  Three on the stream: the plan launch of ecg_dread.h (one wave per record, into d_work); ONE main
 * launch of R * ceil(largest cover / span) workgroups, largest cover = min(NP * P, B), span = 256 KiB cut down to that
 * cover; a verdict launch of one lane per record, which compares the record's sums with the table and writes the
 * report.  A workgroup whose span lies past its record's cover exits at once, so max_len should be the batch's real
 * maximum.  The last B % 16 bytes of a block, and layouts whose base or strides are not 16-byte aligned, are read byte
 * by byte: slow and correct.
 *
 * Links against libecg.so (include/ecg.h): same status codes, batch scopes and streams.  All pointers are DEVICE
 * pointers unless noted; `stream` is a hipStream_t (NULL = default stream) and the calls are asynchronous on it.  A call
 * flushes the thread's batch scope first.  No call allocates: d_work is ecg_vread_work_bytes(R, n) bytes of
 * caller-owned device scratch, 32-byte aligned.
 */
#ifndef ECG_VREAD_H
#define ECG_VREAD_H

#include "ecg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ECG_VREAD_ANSWERED 0
#define ECG_VREAD_UNRECOVERABLE 6
#define ECG_VREAD_MISMATCH 7
#define ECG_VREAD_NO_PIECE 0xFFFFFFFFu

/* The primitive: H (r x n, row-major) over blocks src_ids[0..n) of the strided layout. */
int ecg_vread_matrix_batch(int n, int r, const int* H, const int* src_ids, const void* d_base, long long sstride,
                           long long bstride, long long B, int S,
                           const unsigned char* d_lost /* device, [S][n], or NULL */, long long piece_bytes,
                           const unsigned* d_expected /* device, [S][n][Q] */,
                           const long long* d_records /* device, [R][5] */, int R, long long max_len, void* d_out,
                           long long out_bytes, void* d_work, unsigned* d_sums /* [R][NP] */,
                           unsigned* d_report /* [R][4] */, void* stream);
/* H = [matrix | I] (matrix: m x k) over stripes of k+m blocks: data are blocks 0..k-1, coding blocks k..k+m-1. */
int ecg_vread_encode_batch(int k, int m, const int* matrix, const void* d_stripes, long long sstride,
                           long long bstride, long long B, int S, const unsigned char* d_lost, long long piece_bytes,
                           const unsigned* d_expected, const long long* d_records, int R, long long max_len,
                           void* d_out, long long out_bytes, void* d_work, unsigned* d_sums, unsigned* d_report,
                           void* stream);
/* The class's own check (ecg_ec_check_matrix) over strided stripes.  ECG_MEM_DEVICE handles only. */
int ecg_vread_ec_batch(ecg_ec* ec, const void* d_stripes, long long sstride, long long bstride, long long B, int S,
                       const unsigned char* d_lost, long long piece_bytes, const unsigned* d_expected,
                       const long long* d_records, int R, long long max_len, void* d_out, long long out_bytes,
                       void* d_work, unsigned* d_sums, unsigned* d_report, void* stream);
/* Bytes of device scratch a call over R records of an n-column check needs (a multiple of 32), or ECG_EINVAL. */
long long ecg_vread_work_bytes(int R, int n);
/* Host only, no device: the cover of bytes [off, off + len) of a block of B bytes.  *q0 = the first covering piece,
 * *npieces = how many, *cover_bytes = their bytes (the last piece of a block is the shorter one); all three 0 when
 * len == 0, and any of the pointers may be NULL.  ECG_EINVAL for a bad piece_bytes or a range outside the block. */
int ecg_vread_cover(long long off, long long len, long long piece_bytes, long long B, long long* q0,
                    long long* npieces, long long* cover_bytes);
/* Host only: NP, the most pieces a record of max_len bytes can cover (0 for max_len == 0), or ECG_EINVAL. */
long long ecg_vread_max_pieces(long long max_len, long long piece_bytes, long long B);
/* Host only, no device: the rule of ecg_dread_check_records.  -1 if every record is free of states 1-5 and the out
 * ranges are pairwise disjoint, else the index of the first offending record.  ECG_EINVAL (-2) for a NULL array or a
 * negative R. */
int ecg_vread_check_records(const long long* h_records, int R, int n, long long B, int S, long long max_len,
                            long long out_bytes);
/* A test knob, process-wide: the bytes of a cover one workgroup takes.  0 = auto (256 KiB), otherwise a positive
 * multiple of 2048.  The results do not depend on it. */
int ecg_vread_set_span_bytes(long long bytes);
/* Main kernels launched and records they covered, process-wide (plan and verdict launches are not counted). */
int ecg_vread_counters(long long* launches, long long* records);
/* Launch geometry of the most recent main launch, process-wide.  Six values, in order:
 *   v[0] path           0 = 16-byte columns, 1 = the byte kernel (an unaligned layout)
 *   v[1] piece_bytes    the kernels' piece: piece_bytes, or with block sums the power of two >= max(B, 512)
 *   v[2] max_pieces     NP
 *   v[3] span_bytes     bytes of a cover per workgroup
 *   v[4] wg_per_record  workgroups per record
 *   v[5] R              the records of the launch
 * All zero before the first; calls with max_len == 0 have no main launch and do not change it.  Host only.  Returns
 * the number of values, 6; v is written when cap >= 6 (v may be NULL with cap == 0). */
int ecg_vread_last_launch(int* v, int cap);

#ifdef __cplusplus
}
#endif
#endif /* ECG_VREAD_H */
