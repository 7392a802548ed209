/*
 * ecg_restore.h — named-block restoration on the MI355X (gfx950): rebuild up to r flagged blocks of a stripe in
 * place, from its syndromes (libecg_restore.so).
 *
 * The heal (ecg_heal.h) corrects ONE named block per stripe, heal2 (ecg_heal2.h) one or two.  A store with block or
 * piece checksums (ecg_sum.h, ecg_psum.h) knows more: every block whose checksum differs.  This treats those blocks as
 * erasures and rebuilds all of them, up to the code's r, in one launch whatever the mix of flagged sets -- and, unlike
 * a decode, it uses the check rows it has to spare to notice damage in a block nobody flagged.
 *
 * Definition.  H, v[x], s[x] and BAD are those of ecg_locate.h: H is a check matrix (r x n over GF(2^8) / 0x11d,
 * r <= 8, n <= 128), v[x] the n stored bytes of one stripe at byte position x in [0, B), s[x] = H * v[x]; x is bad if
 * s[x] != 0.  Every selected stripe i has flags d_named[i][0..n) (uint8, device memory): E = { j : flag != 0 },
 * t = |E|.  Column j stands for block src_ids[j].  The stripe's STATE is
 *         0  usable: 1 <= t <= r and the columns H[:, E] are independent,
 *         1  no block flagged,
 *         2  t > r,
 *         3  the flagged columns are dependent, a zero column included.
 * In states 1-3 the stripe is read and counted and never written.  In state 0, for every bad x:
 *   - if there is an e with H_E * e = s[x] (then it is unique: full column rank), byte x of block b becomes
 *     v_b[x] ^ e_b for every b in E with e_b != 0;
 *   - otherwise x is left alone.  This is possible only when t < r.
 * No other byte of memory changes: a byte that is not corrected is not written (a lane stores the 16-byte column that
 * holds a corrected byte, as the heal does; the column's other bytes are stored with the values they had).
 * The report for one selected stripe is n + 3 unsigned counters:
 *         report[b]     (b < n)  positions corrected in block b (block b = column b of H),
 *         report[n]              bad positions,
 *         report[n + 1]          bad positions left untouched,
 *         report[n + 2]          the state.
 * A bad position of a usable stripe is either left untouched or corrected in at least one block, so
 * report[n] - report[n + 1] <= report[0] + .. + report[n - 1] <= t * (report[n] - report[n + 1]); in states 1-3
 * report[n + 1] == report[n] and every report[b] is 0.  Counts are exact and reproducible.  Every stored byte of a
 * selected stripe is read once (n * B per stripe, see ecg_restore_counters); clean data costs what the locate costs.
 *
 * Three facts.
 *   - Guard.  With t < r over a check whose every t + 1 columns are independent (every RS check with t < r), damage
 *     in ONE unflagged block is never written anywhere and is always counted in report[n + 1]: at such a position the
 *     syndrome is H_E * e + f * H[:, u] with f != 0, which no e' can explain, or column u would depend on H[:, E].
 *     The position is left alone as a whole, the flagged blocks' bytes there included.  Damage in two or more
 *     unflagged blocks at one position can imitate the flagged set as soon as t + 2 > r.
 *   - No guard at t = r.  H_E is then square and invertible: every syndrome is explained, report[n + 1] is 0 whatever
 *     the damage, and damage in an unflagged block is folded into the flagged ones.  The checksums are the only
 *     witness.
 *   - Identity.  For t = 1 the bytes and the first n + 2 counters equal those of the heal's TARGET mode with the
 *     flagged block as target (a flagged zero column is state 3 here and an unexplaining target there: the same
 *     bytes and counters).
 *
 * Limits.
 *   - One lane holds all r syndromes: r <= 8 and n <= 128, otherwise ECG_EINVAL with ecg_last_error() set.  Product
 *     codes with r > 8 are refused, as in the locate.
 *   - The stripe ids of one call must be DISTINCT.  A duplicate makes two workgroups read-modify-write the same
 *     bytes, and the result is undefined.  The ids are not checked.
 *   - This call WRITES the stored blocks.  A store should re-verify afterwards: its checksums remain the last word.
 *   - When to decode instead.  Blocks that are lost as a whole and named on the host are a decode's case
 *     (ecg_decode_batch): it reads k blocks per stripe, not n.  This call is for flagged blocks that are damaged in
 *     places, for per-stripe sets that differ, and for sets that live on the device.
 *
 * Links against libecg.so (include/ecg.h): same status codes, coefficient-table cache, batch scopes and streams.
 * All pointers are DEVICE pointers unless noted; `stream` is a hipStream_t (NULL = default stream) and the calls are
 * asynchronous on it.  A call flushes the thread's batch scope first (it sees the recorded calls' results), zeroes
 * `d_report` on the stream, then launches: once it completes d_report holds this call's result, not an accumulation.
 * No call allocates: the strided forms take d_work, ecg_restore_work_bytes(S_sel) bytes of caller-owned device scratch
 * (32-byte aligned), where a small launch ahead of the main one writes one plan per selected stripe.  The scratch may
 * be reused once the call's work on the stream has completed.
 *
 * Arguments: NULL pointers (d_stripe_ids excepted), negative sizes, B >= 2^31, r < 1, n < 1, r > 8, n > 128, a
 * misaligned d_work and host-memory handles are ECG_EINVAL, with ecg_last_error() set, before any device is touched;
 * otherwise S_sel == 0 or B == 0 is a no-op returning 0.  Blocks, strides or a base that are not 16-byte aligned run
 * a byte kernel.
 *
 * Stripe selection: d_stripe_ids is a device array of S_sel stripe indices (int32), NULL = 0 .. S_sel-1.  Row i of
 * d_report, and row i of d_named, belong to stripe d_stripe_ids[i].
 */
#ifndef ECG_RESTORE_H
#define ECG_RESTORE_H

#include "ecg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The primitive: H (r x n, row-major) over blocks src_ids[0..n) of every selected stripe (block b of stripe s at
 * d_base + s*sstride + b*bstride).  report[j], and flag j, stand for column j of H, i.e. block src_ids[j]. */
int ecg_restore_matrix_batch(int n, int r, const int* H, const int* src_ids, void* d_base, long long sstride,
                             long long bstride, long long B,
                             const int* d_stripe_ids /* device, [S_sel]; NULL = 0..S_sel-1 */,
                             const unsigned char* d_named /* device, [S_sel][n] */, int S_sel,
                             void* d_work /* device, ecg_restore_work_bytes(S_sel) */,
                             unsigned* d_report /* [S_sel][n+3] */, void* stream);
/* H = [matrix | I] over stripes of k+m blocks (data 0..k-1, coding k..k+m-1: the layout of ecg_decode_batch and
 * ecg_heal_encode_batch); n = k + m, r = m. */
int ecg_restore_encode_batch(int k, int m, const int* matrix, void* d_stripes, long long sstride, long long bstride,
                             long long B, const int* d_stripe_ids, const unsigned char* d_named /* [S_sel][k+m] */,
                             int S_sel, void* d_work, unsigned* d_report /* [S_sel][k+m+3] */, void* stream);
/* The class's own check (ecg_ec_check_matrix) over strided stripes / over one stripe's block pointers.
 * ECG_MEM_DEVICE handles only.  The per-stripe form launches on the handle's stream and takes its flags from HOST
 * memory: it solves on the host and passes the plan in the kernel arguments, so it needs no scratch. */
int ecg_restore_ec_batch(ecg_ec* ec, void* d_stripes, long long sstride, long long bstride, long long B,
                         const int* d_stripe_ids, const unsigned char* d_named /* [S_sel][k+m] */, int S_sel,
                         void* d_work, unsigned* d_report /* [S_sel][k+m+3] */, void* stream);
int ecg_restore_ec(ecg_ec* ec, char** d_data_ptrs, char** d_coding_ptrs, int block_size,
                   const unsigned char* h_named /* HOST, [k+m] */, unsigned* d_report /* [k+m+3] */);
/* Bytes of device scratch the strided forms need for S_sel selected stripes: 0 for 0, growing with S_sel; a negative
 * S_sel is ECG_EINVAL. */
long long ecg_restore_work_bytes(int S_sel);
/* The bridge from a verify (ecg_sum_verify_batch, ecg_psum_verify_batch), without a host round trip: from the sums
 * and the recorded sums, both [S_sel][n][Q] (Q = 1: block sums), d_named[i][q][j] = (the two differ) as 0 / 1, one row
 * of n flags per piece row as the strided forms take it, and d_count[i][q] = the flags set in the row.  Asynchronous
 * on `stream`; Q == 0 or S_sel == 0 is a no-op. */
int ecg_restore_names_from_sums(int n, int Q, const unsigned* d_sums, const unsigned* d_expected /* [S_sel][n][Q] */,
                                int S_sel, unsigned char* d_named /* [S_sel][Q][n] */, int* d_count /* [S_sel][Q] */,
                                void* stream);
/* Restore kernels launched and bytes they read as planned, process-wide: S_sel * B * n per call.  The plan and names
 * launches, and the bytes written (they depend on the data), are not counted. */
int ecg_restore_counters(long long* launches, long long* bytes);
/* Launch geometry of the most recent vector-path (16-byte column) restore launch, process-wide: a diagnostic that
 * says which workgroup -> chunk map a call really ran, after the fallbacks of ECG_OPT_GRID_MAP, ECG_OPT_MAP_GROUP and
 * ECG_OPT_COLS_PER_WG.  Six values, in order (those of ecg_heal_last_launch):
 *   v[0] grid_map       0 linear, 1 XCD-contiguous, 2 stripe groups per XCD
 *   v[1] map_group      stripes per group, reduced to a power-of-two fraction of the option that divides S_sel / 8
 *   v[2] cols_per_wg    16-byte columns per workgroup
 *   v[3] wg_per_stripe  workgroups per selected stripe
 *   v[4] S              S_sel, the launch stripes
 *   v[5] rtiles         row tiles, always 1
 * All zero before the first such launch; byte-kernel launches (tails, unaligned blocks) do not change it.  Host
 * only.  Returns the number of values, 6; v is written when cap >= 6 (v may be NULL with cap == 0). */
int ecg_restore_last_launch(int* v, int cap);

#ifdef __cplusplus
}
#endif
#endif /* ECG_RESTORE_H */
