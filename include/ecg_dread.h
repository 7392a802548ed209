/*
 * ecg_dread.h — degraded range reads on the MI355X (gfx950): answer byte ranges of stored blocks, rebuilding the ranges
 * of lost blocks from the survivors (libecg_dread.so).
 *
 * The check libraries (ecg_scrub.h .. ecg_restore.h) repair what is stored and ecg_update.h changes it.  This is the
 * read side of a store that has lost blocks: a client wants bytes [off, off+len) of a block whose node is down.
 * ecg_decode_batch rebuilds whole blocks ((k + 1) * B bytes per stripe whatever the size of the answer, host-side
 * erasure patterns of one shape), ecg_restore_* reads n * B per stripe and writes the stored blocks.  Here one launch
 * answers R records, whatever their mix of stripes, lost sets, blocks, offsets and lengths; a record reads reads * len
 * bytes, `reads` being the survivors its reconstruction really needs, and nothing of the store is written.
 *
 * Definition.  H is a check matrix, r x n over GF(2^8) / 0x11d, r <= 8, n <= 128: H * v[x] = 0 at every byte position
 * x of an intact stripe.  Column j stands for block src_ids[j] of a strided layout: block b of stripe s is at
 * d_base + s*sstride + b*bstride, it has B bytes, and the layout has S stripes.  d_lost[S][n] (uint8, device memory,
 * indexed by stripe number) flags the lost columns of every stripe: E_s = { j : d_lost[s][j] != 0 }.  There is no limit
 * on |E_s|.  A record is five int64 values in device memory, d_records[R][5]: {stripe, col, off, len, out_off}.  Its
 * answer is d_out[out_off .. out_off+len), inside a buffer of out_bytes bytes, and holds bytes [off, off+len) of column
 * `col` of that stripe:
 *   col not lost   the bytes are copied.  reads = 1.
 *   col lost       out[x] = XOR_{j not in E} c_j * v_j[x], with the coefficient vector c = Plan(H, E, col) below.
 *                  Blocks in E are never read.  reads = the number of nonzero c_j.
 *
 * The plan rule.  Deterministic and exact:
 *   1. Order the rows of H by ascending (nonzeros in the columns outside E, row index).
 *   2. Walk the lost columns in ascending column index.  For each, the pivot is the first unused row in that order
 *      whose current (eliminated) entry in the column is nonzero.  Scale it to 1 and eliminate the column from every
 *      other row (Gauss-Jordan, tracking the r x r row transform).  A column with no pivot is skipped.
 *   3. If `col` got no pivot, the block is not recoverable.  If the pivot row of `col`, applied to H[:, E], is not
 *      exactly the unit vector at `col`, the block is not recoverable either.
 *   4. Otherwise w is that row of the transform, and c_j = (w * H)[j] for j not in E.
 * Both refusals of step 3 are exact: a w with w * H_E = unit_col exists if and only if rank H_E > rank H_{E \ col}.
 * With one loss, w is a multiple of the sparsest row that covers col, so the local parities of an LRC serve local
 * reads, also when more blocks are lost elsewhere in the stripe than the code has parities.  For [G | I] of an MDS code
 * every recoverable record reads exactly k blocks.  The current value of a lost column is transform * H[:, c], so the
 * device keeps the r x r transform only and |E| may exceed r.
 *
 * Record state and report.  The device validates every record and refuses it as a whole.  d_report[R][2] (unsigned)
 * holds {state, reads}.  The state is the first of these that applies:
 *         0  answered
 *         1  stripe not in [0, S)
 *         2  col not in [0, n)
 *         3  off < 0, len < 0 or off + len > B
 *         4  len > max_len
 *         5  out_off < 0 or out_off + len > out_bytes
 *         6  col is lost and not recoverable from the survivors
 * A refused record reads no block, writes no byte of d_out and has reads = 0.  An answered record reports the reads of
 * its plan, also when len == 0.  The call zeroes d_report on the stream before it launches.
 *
 * Guarantees.  No byte of the stripes is ever stored to.  No byte of d_out outside an answered record's range is
 * stored to, not even with its own value.  The out ranges of one call must be pairwise disjoint: the device does not
 * check this (ecg_dread_check_records does, on the host).  SURVIVORS ARE TAKEN AS GOOD and the answer is not verified:
 * a damaged survivor gives a wrong answer with state 0.  Checksums remain the last word -- a caller whose record covers
 * whole pieces can run ecg_psum.h over d_out and compare with the recorded sums.
 *
 * When to use something else.  Whole lost blocks of many stripes with one erasure shape: ecg_decode_batch, whose
 * composed matrix reads every source once for all outputs.  Rebuilding the stored blocks in place, or damaged (not
 * lost) blocks: ecg_restore.h.  One stripe through block pointers, or a class with r > 8 (the product codes):
 * ecg_ec_decode.  There is no per-stripe pointer form here: a plan of up to 127 coefficient tables does not fit the
 * kernel arguments.
 *
 * Limits.  ECG_EINVAL with ecg_last_error() set, before any device is touched:
 *   - NULL pointers;
 *   - r < 1, r > 8, n < 1 or n > 128;
 *   - ids that are negative or repeated within src_ids;
 *   - B < 0, B >= 2^31, S < 0, R < 0, max_len < 0, max_len > B or out_bytes < 0;
 *   - d_records not 8-byte aligned, d_work not 32-byte aligned;
 *   - a launch that would need more than 2^31 - 1 workgroups (R * ceil((max_len + 15) / chunk), see below);
 *   - in the `ec` form: a host-memory handle, or a class whose check has more than 8 rows.
 * R == 0 is a no-op returning 0.  With max_len == 0 no byte can move (every record with len > 0 is state 4): the call
 * still zeroes and fills the report.
 *
 * The launches.  A plan launch of one wave per record turns every record into its plan in d_work (state, reads, the
 * source blocks and one coefficient table per source); then ONE main launch of R * ceil((max_len + 15) / chunk)
 * workgroups, chunk = 16 * cols_per_wg bytes (ECG_OPT_COLS_PER_WG, default 128 columns = 2 KiB).  A workgroup whose
 * chunk lies past its record's end exits at once, so max_len should be the batch's real maximum.  Chunks are cut on
 * the source blocks' 16-byte grid; the alignment of out_off relative to off does not matter.  Partial first and last
 * columns, and layouts whose base or strides are not 16-byte aligned, move byte by byte.
 *
 * Links against libecg.so (include/ecg.h): same status codes, batch scopes and streams.  All pointers are DEVICE
 * pointers unless noted; `stream` is a hipStream_t (NULL = default stream) and the calls are asynchronous on it.  A call
 * flushes the thread's batch scope first (it sees the recorded calls' results).  No call allocates: d_work is
 * ecg_dread_work_bytes(R, n) bytes of caller-owned device scratch, 32-byte aligned.
 */
#ifndef ECG_DREAD_H
#define ECG_DREAD_H

#include "ecg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ECG_DREAD_ANSWERED 0
#define ECG_DREAD_UNRECOVERABLE 6

/* The primitive: H (r x n, row-major) over blocks src_ids[0..n) of the strided layout. */
int ecg_dread_matrix_batch(int n, int r, const int* H, const int* src_ids, const void* d_base, long long sstride,
                           long long bstride, long long B, int S, const unsigned char* d_lost /* device, [S][n] */,
                           const long long* d_records /* device, [R][5] */, int R, long long max_len, void* d_out,
                           long long out_bytes, void* d_work, unsigned* d_report /* [R][2] */, void* stream);
/* H = [matrix | I] (matrix: m x k) over stripes of k+m blocks: data are blocks 0..k-1, coding blocks k..k+m-1 (the
 * layout of ecg_decode_batch). */
int ecg_dread_encode_batch(int k, int m, const int* matrix, const void* d_stripes, long long sstride,
                           long long bstride, long long B, int S, const unsigned char* d_lost,
                           const long long* d_records, int R, long long max_len, void* d_out, long long out_bytes,
                           void* d_work, unsigned* d_report, void* stream);
/* The class's own check (ecg_ec_check_matrix) over strided stripes.  ECG_MEM_DEVICE handles only. */
int ecg_dread_ec_batch(ecg_ec* ec, const void* d_stripes, long long sstride, long long bstride, long long B, int S,
                       const unsigned char* d_lost, const long long* d_records, int R, long long max_len, void* d_out,
                       long long out_bytes, void* d_work, unsigned* d_report, void* stream);
/* Bytes of device scratch a call over R records of an n-column check needs (a multiple of 32), or ECG_EINVAL. */
long long ecg_dread_work_bytes(int R, int n);
/* Host only, no device: the plan rule as a callable.  h_lost[n] flags E.  Returns the state, 0 or 6 (or ECG_EINVAL);
 * writes c into c_out[n] -- the unit vector of col when col is not lost, all zero in state 6 -- and the number of
 * nonzero c_j to *reads (reads may be NULL). */
int ecg_dread_plan(int n, int r, const int* H, const unsigned char* h_lost, int col, unsigned char* c_out, int* reads);
/* Host only, no device: -1 if every record of h_records[R][5] is free of states 1-5 and the out ranges are pairwise
 * disjoint (empty ranges overlap nothing).  Otherwise the index of the first offending record -- the first that is
 * refused, or whose out range overlaps that of a record before it -- with ecg_last_error() saying which rule broke.
 * State 6 depends on the lost flags and is not looked at.  ECG_EINVAL (-2) for a NULL array or a negative R. */
int ecg_dread_check_records(const long long* h_records, int R, int n, long long B, int S, long long max_len,
                            long long out_bytes);
/* Main kernels launched and records they covered, process-wide (the plan launches are not counted).  The lengths live
 * on the device, so this counts records, not bytes. */
int ecg_dread_counters(long long* launches, long long* records);
/* Launch geometry of the most recent dread launch that covered 16-byte columns, process-wide.  Four values, in order:
 *   v[0] cols_per_wg    16-byte columns per workgroup
 *   v[1] wg_per_record  workgroups per record
 *   v[2] R              the records of the launch
 *   v[3] max_reads      the columns of H that are not all zero: the most sources a record can have
 * All zero before the first such launch; launches over an unaligned layout (byte lanes only) and launches with
 * max_len == 0 do not change it.  Host only.  Returns the number of values, 4; v is written when cap >= 4 (v may be
 * NULL with cap == 0). */
int ecg_dread_last_launch(int* v, int cap);

#ifdef __cplusplus
}
#endif
#endif /* ECG_DREAD_H */
