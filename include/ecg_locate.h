/*
 * ecg_locate.h — corruption localisation on the MI355X (gfx950): name a dirty stripe's damaged block
 * (libecg_locate.so).
 *
 * A scrub (ecg_scrub.h) says THAT a stored stripe no longer satisfies its code.  This says WHICH block is damaged,
 * from the syndrome bytes the scrub never writes: a second, read-only pass over the dirty stripes only.
 *
 * Definition.  H is a check matrix (r x n over GF(2^8) / 0x11d), v[x] the n stored bytes of one stripe at byte
 * position x in [0, B), and s[x] = H * v[x] its r syndrome bytes.
 *   - x is BAD if s[x] != 0.
 *   - block b EXPLAINS a bad x if s[x] = e * H[:, b] for some e != 0: damaging block b alone, by e, gives exactly
 *     this syndrome.  Equivalently, with p0 the first row where H[p0][b] != 0: s_p0[x] != 0 and
 *     s_q[x] = s_p0[x] * (H[q][b] / H[p0][b]) for every other row q.  A zero column explains nothing.
 *   - the result for one selected stripe is n + 2 unsigned counters:
 *         votes[b]     (b < n)  bad positions that block b explains (block b = column b of H),
 *         votes[n]              bad positions,
 *         votes[n + 1]          bad positions that no single block explains.
 * Counts are exact and reproducible (integer adds commute).  Every stored byte of a selected stripe is read once
 * (n * B per stripe, see ecg_locate_counters); nothing is written but the counters, and those only where a syndrome
 * is nonzero.  Clean data costs what the scrub costs; only columns with a nonzero syndrome run the candidate test.
 *
 * Limits.  One lane holds all r syndromes: r <= 8 and n <= 128, otherwise ECG_EINVAL with ecg_last_error() set.
 * Product codes (PC, HV_PC: r > 8 from PC(4,1,4,1) on) stay with ecg_scrub_suspects, whose row / column supports
 * already name the block.
 *
 * What a verdict means, and what it does not.  The candidate test assumes AT MOST ONE damaged block per byte
 * position.  Under that assumption, and when no two columns of H are proportional (true of every RS, ERS and LRC
 * check this library builds with r >= 2; never true for r = 1), the block named is the damaged one.  Two blocks damaged
 * at DISJOINT positions are told apart position by position: both get votes (ecg_locate_verdict: MULTIPLE, both ids).
 * Two blocks damaged at the SAME position are a different matter: with r = 2 any three columns are linearly
 * dependent, so the two error values can add up to a multiple of a third, undamaged block's column and that block
 * is named (miscorrection); with r >= 3 over an MDS check (any 3 columns independent: RS) two damaged blocks cannot
 * imitate a third, and such positions count as unexplained; three blocks at one position can imitate a fourth when
 * r = 3, and so on.  An LRC check is not MDS: blocks of one local group can imitate each other's group mates sooner.
 * A store that rebuilds the named block should re-scrub, and keep its own block checksums as the last word.
 *
 * Links against libecg.so (include/ecg.h): same status codes, coefficient-table cache, batch scopes and streams.
 * All pointers are DEVICE pointers unless noted; `stream` is a hipStream_t (NULL = default stream) and the calls are
 * asynchronous on it.  A call flushes the thread's batch scope first (it sees the recorded calls' results), zeroes
 * `d_votes` on the stream, then launches: once it completes d_votes holds this call's result, not an accumulation.
 *
 * Arguments: NULL pointers (d_stripe_ids excepted), negative sizes, B >= 2^31, r < 1, n < 1, r > 8, n > 128 and
 * host-memory handles are ECG_EINVAL before any device is touched; S_sel == 0 or B == 0 is a no-op returning 0.
 * Blocks, strides or a base that are not 16-byte aligned run a byte kernel.
 *
 * Stripe selection: d_stripe_ids is a device array of S_sel stripe indices (int32), NULL = 0 .. S_sel-1.  Row i of
 * d_votes is the result of stripe d_stripe_ids[i].  The ids are not checked: an id outside the stripes the caller
 * owns is read like any other, and is the caller's responsibility.
 */
#ifndef ECG_LOCATE_H
#define ECG_LOCATE_H

#include "ecg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ecg_locate_verdict statuses (negative, apart from the ECG_E* codes; a value >= 0 is a block id). */
#define ECG_LOCATE_CLEAN (-100)     /* no bad position */
#define ECG_LOCATE_AMBIGUOUS (-101) /* several blocks each explain every bad position (proportional columns, r = 1) */
#define ECG_LOCATE_MULTIPLE (-102)  /* no single block explains every bad position */

/* The primitive: H (r x n, row-major) over blocks src_ids[0..n) of every selected stripe (block b of stripe s at
 * d_base + s*sstride + b*bstride).  votes[j] counts for column j of H, i.e. block src_ids[j]. */
int ecg_locate_matrix_batch(int n, int r, const int* H, const int* src_ids, const void* d_base,
                            long long sstride, long long bstride, long long B,
                            const int* d_stripe_ids /* device, [S_sel]; NULL = 0..S_sel-1 */, int S_sel,
                            unsigned* d_votes /* [S_sel][n+2] */, void* stream);
/* H = [matrix | I] over stripes of k+m blocks (data 0..k-1, coding k..k+m-1: the layout of ecg_decode_batch and
 * ecg_scrub_encode_batch); n = k + m, r = m. */
int ecg_locate_encode_batch(int k, int m, const int* matrix, const void* d_stripes, long long sstride,
                            long long bstride, long long B, const int* d_stripe_ids, int S_sel,
                            unsigned* d_votes /* [S_sel][k+m+2] */, void* stream);
/* The class's own check (ecg_ec_check_matrix) over strided stripes / over one stripe's block pointers.
 * ECG_MEM_DEVICE handles only; the per-stripe form launches on the handle's stream. */
int ecg_locate_ec_batch(ecg_ec* ec, const void* d_stripes, long long sstride, long long bstride, long long B,
                        const int* d_stripe_ids, int S_sel, unsigned* d_votes /* [S_sel][k+m+2] */, void* stream);
int ecg_locate_ec(ecg_ec* ec, char** d_data_ptrs, char** d_coding_ptrs, int block_size,
                  unsigned* d_votes /* [k+m+2] */);
/* One stripe's votes (HOST memory, n + 2 values) -> a verdict.  Host only.  Returns
 *   ECG_LOCATE_CLEAN      votes[n] == 0;
 *   b >= 0                exactly one block has votes[b] == votes[n], and votes[n+1] == 0: block b explains every
 *                         bad position (under the one-block-per-position assumption above, it is the damaged one);
 *   ECG_LOCATE_AMBIGUOUS  several blocks have votes[b] == votes[n];
 *   ECG_LOCATE_MULTIPLE   otherwise;
 *   ECG_EINVAL            n < 1, h_votes NULL, cap < 0, or ids NULL with cap > 0.
 * *n_ids (if not NULL) receives the number of blocks with votes > 0, and ids[0 .. *n_ids) those blocks in ascending
 * order when cap suffices (nothing is written to ids otherwise): what a store passes on as erasures when two blocks
 * are damaged at disjoint positions. */
int ecg_locate_verdict(int n, const unsigned* h_votes /* n+2 */, int* ids, int cap, int* n_ids);
/* Locate kernels launched and bytes they read as planned, process-wide: S_sel * B * n per call. */
int ecg_locate_counters(long long* launches, long long* bytes);
/* Launch geometry of the most recent vector-path (16-byte column) locate launch, process-wide: a diagnostic that says
 * which workgroup -> chunk map a call really ran, after the fallbacks of ECG_OPT_GRID_MAP, ECG_OPT_MAP_GROUP and
 * ECG_OPT_COLS_PER_WG.  Six values, in order (those of ecg_scrub_last_launch):
 *   v[0] grid_map       0 linear, 1 XCD-contiguous, 2 stripe groups per XCD
 *   v[1] map_group      stripes per group, reduced to a power-of-two fraction of the option that divides S_sel / 8
 *   v[2] cols_per_wg    16-byte columns per workgroup
 *   v[3] wg_per_stripe  workgroups per selected stripe
 *   v[4] S              S_sel, the launch stripes
 *   v[5] rtiles         row tiles, always 1
 * All zero before the first such launch; byte-kernel launches (tails, unaligned blocks) do not change it.  Host
 * only.  Returns the number of values, 6; v is written when cap >= 6 (v may be NULL with cap == 0). */
int ecg_locate_last_launch(int* v, int cap);

#ifdef __cplusplus
}
#endif
#endif /* ECG_LOCATE_H */
