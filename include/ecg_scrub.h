/*
 * ecg_scrub.h — stripe scrubbing on the MI355X (gfx950): a read-only GF(2^8) parity check (libecg_scrub.so).
 *
 * Do these stored stripes still satisfy their code?  For a check matrix H (r x k_in over GF(2^8)) and S stripes
 *
 *     counts[s * r + p] = number of byte positions x in [0, B) with  XOR_j H[p][j] * in_j[x] != 0 .
 *
 * An encode P = C * D is checked with H = [C | I] over the k+m stored blocks.  Every input byte is read once
 * (k_in * B per stripe and row tile; tiles as in the region product: 8 rows, 16 when H is all 0/1; H = [C | I]
 * costs the arithmetic of C alone, see ecg_scrub_counters) and nothing is written but the counters, and those only
 * where a check fails: a clean stripe costs no HBM write.
 *
 * Links against libecg.so (include/ecg.h): same status codes, same coefficient-table cache, batch scopes and
 * streams.  All pointers are DEVICE pointers unless noted; `stream` is a hipStream_t (NULL = default stream) and
 * the calls are asynchronous on it.  A call zeroes `d_counts` on the stream, then launches: once it completes,
 * d_counts holds this call's result, not an accumulation.  Inside a batch scope (ecg_batch_begin) a scrub
 * flushes the recorded calls first, so it sees their results.
 *
 * Arguments: B >= 2^31, negative S or B, r < 1, k_in < 1 and NULL pointers are ECG_EINVAL before any device is
 * touched; S == 0 or B == 0 is a no-op returning 0.  Blocks that are not 16-byte aligned run a byte kernel.
 */
#ifndef ECG_SCRUB_H
#define ECG_SCRUB_H

#include "ecg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The primitive: row p of H over blocks src_ids[0..k_in) of every stripe (block b of stripe s at
 * d_base + s*sstride + b*bstride). */
int ecg_scrub_matrix_batch(int k_in, int r, const int* H, const int* src_ids,
                           const void* d_base, long long sstride, long long bstride,
                           long long B, int S, unsigned* d_counts /* [S*r] */, void* stream);
/* H = [matrix | I] over stripes of k+m blocks (data 0..k-1, coding k..k+m-1, the layout of ecg_decode_batch).
 * An all-zero matrix row is not checked (count 0): jerasure_matrix_dotprod leaves such a block untouched. */
int ecg_scrub_encode_batch(int k, int m, const int* matrix, const void* d_stripes, long long sstride,
                           long long bstride, long long B, int S, unsigned* d_counts /* [S*m] */, void* stream);
/* The class's own check (ecg_ec_check_matrix) over strided stripes / over one stripe's block pointers.
 * ECG_MEM_DEVICE handles only (ECG_EINVAL otherwise: host-resident data is PCIe-bound and the CPU is faster there,
 * INTEGRATION.md); the per-stripe form launches on the handle's stream and takes at most 128 blocks (k + m). */
int ecg_scrub_ec_batch(ecg_ec* ec, const void* d_stripes, long long sstride, long long bstride, long long B,
                       int S, unsigned* d_counts /* [S*m] */, void* stream);
int ecg_scrub_ec(ecg_ec* ec, char** d_data_ptrs, char** d_coding_ptrs, int block_size, unsigned* d_counts /* [m] */);
/* Blocks b whose column support {p : H[p][b] != 0} equals the set of rows with a nonzero count: the blocks a
 * single corrupted block can be.  Host only.  Returns how many (ids written when cap suffices); 0 if the stripe is
 * clean or no single block explains the rows. */
int ecg_scrub_suspects(int r, int n, const int* H, const unsigned* h_counts, int* ids, int cap);
/* Scrub kernels launched and bytes they read as planned, process-wide: S*B*k_in per row tile; when the last r
 * columns of H are unit columns over consecutive blocks (H = [C | I]: every encode check) only C goes through the
 * coefficient tables and each of those r blocks is read once, by its own row's tile: S*B*(tiles*(k_in-r) + r). */
int ecg_scrub_counters(long long* launches, long long* bytes);
/* Launch geometry of the most recent vector-path (16-byte column) scrub launch, process-wide: a diagnostic that says
 * which workgroup -> chunk map a call really ran, after the fallbacks of ECG_OPT_GRID_MAP, ECG_OPT_MAP_GROUP and
 * ECG_OPT_COLS_PER_WG.  Six values, in order:
 *   v[0] grid_map       0 linear, 1 XCD-contiguous, 2 stripe groups per XCD
 *   v[1] map_group      stripes per group, reduced to a power-of-two fraction of the option that divides S / 8
 *   v[2] cols_per_wg    16-byte columns per workgroup
 *   v[3] wg_per_stripe  workgroups per stripe and row tile
 *   v[4] S              stripes of the launch
 *   v[5] rtiles         row tiles (gridDim.y)
 * All zero before the first such launch; byte-kernel launches (tails, unaligned blocks) do not change it.  Host
 * only.  Returns the number of values, 6; v is written when cap >= 6 (v may be NULL with cap == 0). */
int ecg_scrub_last_launch(int* v, int cap);

#ifdef __cplusplus
}
#endif
#endif /* ECG_SCRUB_H */
