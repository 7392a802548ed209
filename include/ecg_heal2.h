/*
 * ecg_heal2.h — two-block correction on the MI355X (gfx950): fix a dirty stripe's damaged bytes from its syndromes
 * where up to TWO blocks are damaged at one byte position (libecg_heal2.so).
 *
 * The heal (ecg_heal.h) corrects a position that one block explains and leaves every other bad position alone.  Take
 * one block that is garbage (a lost sector, a misdirected write) and a 4 KiB run damaged in a second block: the heal
 * fixes the first block everywhere except at those 4096 positions.  This call goes on to the code's distance: an
 * unknown pair of blocks per position over a check whose every 4 columns are independent (RS with r >= 4), one named
 * block plus one unknown block over a check whose every 3 columns are independent (r >= 3).
 *
 * Definition.  H, v[x], s[x] and BAD are those of ecg_locate.h: H is a check matrix (r x n over GF(2^8) / 0x11d),
 * v[x] the n stored bytes of one stripe at byte position x in [0, B), s[x] = H * v[x]; x is bad if s[x] != 0; h_b is
 * column b of H.
 * An EXPLANATION of a bad x is a set A of one or two blocks with values e_a != 0 (a in A) such that
 *         s[x] = XOR_{a in A} e_a * h_a.
 * Every selected stripe has a family F of admissible sets:
 *   - ANY2 (d_targets NULL): F = every set of one or two blocks.
 *   - TARGET2 (d_targets not NULL, a device array int32[S_sel]; t = d_targets[i], 0 <= t < n): F = every single
 *     block, and every pair that contains t.
 *   - A target outside [0, n) (-1, n, a negative number) gives an empty F: the stripe is read and counted, never
 *     written.  This is the heal's rule.
 * For every bad x that has an explanation A in F, byte x of every block a in A becomes v_a[x] ^ e_a.  No other byte
 * of memory changes: a byte that is not corrected is not written.
 * The report for one selected stripe is n + 3 unsigned counters:
 *         report[b]     (b < n)  positions corrected in block b (block b = column b of H); a pair counts in both,
 *         report[n]              bad positions,
 *         report[n + 1]          bad positions left untouched,
 *         report[n + 2]          positions corrected as a pair,
 * so that report[0] + .. + report[n-1] - report[n+2] + report[n+1] == report[n].  Where no position needs a pair,
 * the first n + 2 counters and the bytes equal what ecg_heal_* in ANY mode produces.  Counts are exact and
 * reproducible.  Every stored byte of a selected stripe is read once (n * B per stripe, see ecg_heal2_counters), and
 * the bytes a lane corrects once more; clean data costs what the heal and the locate cost, and a wave whose bad bytes
 * are all explained by single blocks never enters the pair phase.
 *
 * Uniqueness.  Two different explanations A, A' of one x XOR to a nontrivial combination of the columns in A u A'
 * that is zero.  In ANY2 |A u A'| <= 4, in TARGET2 <= 3 (two pairs share t; a single and a pair make 3): where every
 * 4, respectively every 3, columns of H are independent there is no such combination, the explanation in F is unique,
 * and the order in which candidates are tried cannot matter.
 *
 * Limits.
 *   - 3 <= r <= 8 and 2 <= n <= 32, otherwise ECG_EINVAL with ecg_last_error() set.  One lane holds all r syndromes,
 *     a pair needs a third row to be tested against, and the pair tables grow with n (n - 1) / 2 <= 496.  32 blocks
 *     cover every RS / ERS / LRC check of this library that passes the independence tests below.
 *   - ANY2 is refused (ECG_EINVAL, ecg_last_error() names the columns, before any device is touched) unless every 4
 *     columns of H are linearly independent -- so r >= 4 and no zero column.  TARGET2 is refused unless every 3 are.
 *     RS(k, m) with m >= 4 passes both; an LRC's check with a local row does not pass ANY2 (a local group is a
 *     dependent set), and passes TARGET2 only if every 3 columns are independent.
 *   - Miscorrection.  With r = 4, three blocks damaged at ONE position can imitate a pair (any 4 columns are
 *     independent, but a syndrome of weight 3 may equal one of weight 2 from other columns), and in ANY2 that pair
 *     gets written.  From r = 5 over an MDS check such positions are left alone and counted in report[n + 1]; in
 *     TARGET2 with r = 3 a third damaged block can likewise imitate a pair with t.  Blocks damaged at DISJOINT
 *     positions are corrected position by position, however many they are.
 *   - The stripe ids of one call must be DISTINCT.  A duplicate makes two workgroups read-modify-write the same
 *     bytes, and the result is undefined.  The ids are not checked.
 *   - This call WRITES the stored blocks.  A store should re-scrub afterwards, and its own block checksums remain
 *     the last word.
 *
 * Links against libecg.so (include/ecg.h): same status codes, coefficient-table cache, batch scopes and streams.
 * All pointers are DEVICE pointers unless noted; `stream` is a hipStream_t (NULL = default stream) and the calls are
 * asynchronous on it.  A call flushes the thread's batch scope first (it sees the recorded calls' results), zeroes
 * `d_report` on the stream, then launches: once it completes d_report holds this call's result, not an accumulation.
 *
 * Arguments: NULL pointers (d_stripe_ids and d_targets excepted), negative sizes, B >= 2^31, r < 3, n < 2, r > 8,
 * n > 32, host-memory handles and a check that fails its mode's independence test are ECG_EINVAL before any device is
 * touched; otherwise S_sel == 0 or B == 0 is a no-op returning 0.  Blocks, strides or a base that are not 16-byte
 * aligned run a byte kernel.
 *
 * Stripe selection: d_stripe_ids is a device array of S_sel stripe indices (int32), NULL = 0 .. S_sel-1.  Row i of
 * d_report, and d_targets[i], belong to stripe d_stripe_ids[i].
 */
#ifndef ECG_HEAL2_H
#define ECG_HEAL2_H

#include "ecg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The primitive: H (r x n, row-major) over blocks src_ids[0..n) of every selected stripe (block b of stripe s at
 * d_base + s*sstride + b*bstride).  report[j], and a target j, stand for column j of H, i.e. block src_ids[j]. */
int ecg_heal2_matrix_batch(int n, int r, const int* H, const int* src_ids, void* d_base, long long sstride,
                           long long bstride, long long B,
                           const int* d_stripe_ids /* device, [S_sel]; NULL = 0..S_sel-1 */,
                           const int* d_targets /* device, [S_sel]; NULL = ANY2 */, int S_sel,
                           unsigned* d_report /* [S_sel][n+3] */, void* stream);
/* H = [matrix | I] over stripes of k+m blocks (data 0..k-1, coding k..k+m-1: the layout of ecg_decode_batch and
 * ecg_heal_encode_batch); n = k + m, r = m. */
int ecg_heal2_encode_batch(int k, int m, const int* matrix, void* d_stripes, long long sstride, long long bstride,
                           long long B, const int* d_stripe_ids, const int* d_targets, int S_sel,
                           unsigned* d_report /* [S_sel][k+m+3] */, void* stream);
/* The class's own check (ecg_ec_check_matrix) over strided stripes / over one stripe's block pointers.
 * ECG_MEM_DEVICE handles only; the per-stripe form launches on the handle's stream and takes its target as a host
 * value: a block id in [0, k+m) for TARGET2, or -1 for ANY2 (anything else is ECG_EINVAL). */
int ecg_heal2_ec_batch(ecg_ec* ec, void* d_stripes, long long sstride, long long bstride, long long B,
                       const int* d_stripe_ids, const int* d_targets, int S_sel,
                       unsigned* d_report /* [S_sel][k+m+3] */, void* stream);
int ecg_heal2_ec(ecg_ec* ec, char** d_data_ptrs, char** d_coding_ptrs, int block_size,
                 int target /* host; -1 = ANY2 */, unsigned* d_report /* [k+m+3] */);
/* Kernels launched and bytes they read as planned, process-wide: S_sel * B * n per call.  What the corrections read
 * again and write depends on the data and is not counted. */
int ecg_heal2_counters(long long* launches, long long* bytes);
/* Launch geometry of the most recent vector-path (16-byte column) launch of this library, process-wide: a diagnostic
 * that says which workgroup -> chunk map a call really ran, after the fallbacks of ECG_OPT_GRID_MAP,
 * ECG_OPT_MAP_GROUP and ECG_OPT_COLS_PER_WG.  Six values, in order (those of ecg_heal_last_launch):
 *   v[0] grid_map       0 linear, 1 XCD-contiguous, 2 stripe groups per XCD
 *   v[1] map_group      stripes per group, reduced to a power-of-two fraction of the option that divides S_sel / 8
 *   v[2] cols_per_wg    16-byte columns per workgroup
 *   v[3] wg_per_stripe  workgroups per selected stripe
 *   v[4] S              S_sel, the launch stripes
 *   v[5] rtiles         row tiles, always 1
 * All zero before the first such launch; byte-kernel launches (tails, unaligned blocks) do not change it.  Host
 * only.  Returns the number of values, 6; v is written when cap >= 6 (v may be NULL with cap == 0). */
int ecg_heal2_last_launch(int* v, int cap);

#ifdef __cplusplus
}
#endif
#endif /* ECG_HEAL2_H */
