/*
 * ecg_heal.h — in-place correction on the MI355X (gfx950): fix a dirty stripe's damaged bytes from its syndromes
 * (libecg_heal.so).
 *
 * A scrub (ecg_scrub.h) says THAT a stored stripe no longer satisfies its code, the locate (ecg_locate.h) WHICH
 * block is damaged.  This repairs the damage: a pass over the dirty stripes that reads what the locate reads and
 * XORs the error value back into the damaged bytes, in one launch whatever the mix of damaged blocks.
 *
 * Definition.  H, v[x], s[x], BAD and EXPLAINS are those of ecg_locate.h: H is a check matrix (r x n over
 * GF(2^8) / 0x11d), v[x] the n stored bytes of one stripe at byte position x in [0, B), s[x] = H * v[x]; x is bad
 * if s[x] != 0; block b explains a bad x if s[x] = e * H[:, b] for some e != 0, the error value.
 * Every selected stripe has a candidate set K:
 *   - TARGET mode (d_targets not NULL, a device array int32[S_sel]): K = {t}, t = d_targets[i], if 0 <= t < n;
 *     any other value (-1, n, a negative number) gives an empty K: the stripe is read and counted, never written.
 *   - ANY mode (d_targets NULL): K = every block.
 * For every bad position x and every b in K that explains x with error value e, byte x of block b becomes
 * v_b[x] ^ e.  No other byte of memory changes: a byte that is not corrected is not written.
 * The report for one selected stripe is n + 2 unsigned counters, laid out as the locate's votes:
 *         report[b]     (b < n)  positions corrected in block b (block b = column b of H),
 *         report[n]              bad positions,
 *         report[n + 1]          bad positions left untouched,
 * so that report[0] + .. + report[n-1] + report[n+1] == report[n].  In ANY mode the report equals what
 * ecg_locate_* returns over the same bytes before the call; in TARGET mode report[t] is the locate's votes[t], every
 * other report[b] is 0 and report[n+1] = votes[n] - votes[t].  ecg_locate_verdict reads a report unchanged: the
 * block it names is the block that was corrected everywhere.  The locate is this call's dry run.
 * Counts are exact and reproducible.  Every stored byte of a selected stripe is read once (n * B per stripe, see
 * ecg_heal_counters); clean data costs what the locate costs.
 *
 * Limits.
 *   - One lane holds all r syndromes: r <= 8 and n <= 128, otherwise ECG_EINVAL with ecg_last_error() set.  Product
 *     codes with r > 8 are refused, as in the locate.
 *   - ANY mode needs at most one explaining block per position: it is refused with ECG_EINVAL (ecg_last_error() set,
 *     before any device is touched) when two nonzero columns of H are proportional.  That is every r = 1 check with
 *     n >= 2.  TARGET mode takes any H, r = 1 included: there the caller names the block, for instance from its
 *     block checksums.  A zero column of H explains nothing and is never corrected.
 *   - Miscorrection.  The limit is the one ecg_locate.h states.  With r = 2 two blocks damaged at ONE position can
 *     imitate a third, and in ANY mode that third, undamaged block gets written.  With r >= 3 over an MDS check (RS)
 *     such positions are left alone and counted in report[n + 1].  Blocks damaged at DISJOINT positions are
 *     corrected position by position, however many they are: six blocks of an RS(10,4) stripe, each damaged at its
 *     own offsets, all come back.
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
 * Arguments: NULL pointers (d_stripe_ids and d_targets excepted), negative sizes, B >= 2^31, r < 1, n < 1, r > 8,
 * n > 128, host-memory handles and ANY mode over proportional columns are ECG_EINVAL before any device is touched;
 * otherwise S_sel == 0 or B == 0 is a no-op returning 0.  Blocks, strides or a base that are not 16-byte aligned run
 * a byte kernel.
 *
 * Stripe selection: d_stripe_ids is a device array of S_sel stripe indices (int32), NULL = 0 .. S_sel-1.  Row i of
 * d_report, and d_targets[i], belong to stripe d_stripe_ids[i].
 */
#ifndef ECG_HEAL_H
#define ECG_HEAL_H

#include "ecg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The primitive: H (r x n, row-major) over blocks src_ids[0..n) of every selected stripe (block b of stripe s at
 * d_base + s*sstride + b*bstride).  report[j], and a target j, stand for column j of H, i.e. block src_ids[j]. */
int ecg_heal_matrix_batch(int n, int r, const int* H, const int* src_ids, void* d_base, long long sstride,
                          long long bstride, long long B,
                          const int* d_stripe_ids /* device, [S_sel]; NULL = 0..S_sel-1 */,
                          const int* d_targets /* device, [S_sel]; NULL = ANY mode */, int S_sel,
                          unsigned* d_report /* [S_sel][n+2] */, void* stream);
/* H = [matrix | I] over stripes of k+m blocks (data 0..k-1, coding k..k+m-1: the layout of ecg_decode_batch and
 * ecg_locate_encode_batch); n = k + m, r = m. */
int ecg_heal_encode_batch(int k, int m, const int* matrix, void* d_stripes, long long sstride, long long bstride,
                          long long B, const int* d_stripe_ids, const int* d_targets, int S_sel,
                          unsigned* d_report /* [S_sel][k+m+2] */, void* stream);
/* The class's own check (ecg_ec_check_matrix) over strided stripes / over one stripe's block pointers.
 * ECG_MEM_DEVICE handles only; the per-stripe form launches on the handle's stream and takes its target as a host
 * value: a block id in [0, k+m), or -1 for ANY mode (anything else is ECG_EINVAL). */
int ecg_heal_ec_batch(ecg_ec* ec, void* d_stripes, long long sstride, long long bstride, long long B,
                      const int* d_stripe_ids, const int* d_targets, int S_sel,
                      unsigned* d_report /* [S_sel][k+m+2] */, void* stream);
int ecg_heal_ec(ecg_ec* ec, char** d_data_ptrs, char** d_coding_ptrs, int block_size, int target /* host; -1 = ANY */,
                unsigned* d_report /* [k+m+2] */);
/* Heal kernels launched and bytes they read as planned, process-wide: S_sel * B * n per call.  The bytes written
 * depend on the data and are not counted. */
int ecg_heal_counters(long long* launches, long long* bytes);
/* Launch geometry of the most recent vector-path (16-byte column) heal launch, process-wide: a diagnostic that says
 * which workgroup -> chunk map a call really ran, after the fallbacks of ECG_OPT_GRID_MAP, ECG_OPT_MAP_GROUP and
 * ECG_OPT_COLS_PER_WG.  Six values, in order (those of ecg_scrub_last_launch and ecg_locate_last_launch):
 *   v[0] grid_map       0 linear, 1 XCD-contiguous, 2 stripe groups per XCD
 *   v[1] map_group      stripes per group, reduced to a power-of-two fraction of the option that divides S_sel / 8
 *   v[2] cols_per_wg    16-byte columns per workgroup
 *   v[3] wg_per_stripe  workgroups per selected stripe
 *   v[4] S              S_sel, the launch stripes
 *   v[5] rtiles         row tiles, always 1
 * All zero before the first such launch; byte-kernel launches (tails, unaligned blocks) do not change it.  Host
 * only.  Returns the number of values, 6; v is written when cap >= 6 (v may be NULL with cap == 0). */
int ecg_heal_last_launch(int* v, int cap);

#ifdef __cplusplus
}
#endif
#endif /* ECG_HEAL_H */
