/*
 * ecg_usum.h — update sums on the MI355X (gfx950): carry the recorded CRC-32C of blocks and pieces through a delta
 * update (libecg_usum.so).
 *
 * ecg_update.h changes len bytes of a data block and of the parities that depend on them; the sums a store keeps of
 * those blocks (ecg_sum.h per block, ecg_psum.h per piece) are then stale, and re-summing reads n * B bytes per touched
 * stripe.  CRC-32C is linear over GF(2), so the new sum follows from the old one and the change alone.  With raw(d)
 * the remainder for initial value 0 and no final XOR, two messages A, A' of equal length have
 *         crc32c(A) ^ crc32c(A') = raw(A ^ A'),
 * leading zero bytes do not change raw, and t trailing zero bytes multiply it by x^(8 t) mod P.  A change D on bytes
 * [a, b) of a summed range that ends at e therefore gives
 *         sum_new = sum_old ^ raw(D[a..b)) * x^(8 (e - b)).
 * This call reads delta, the records and the sum table and nothing else: the stripes are not an argument.
 *
 * Inputs.  G (m_out x k_in over GF(2^8) / 0x11d), src_ids, dst_ids, B, S, max_len and the records
 * d_records[R][5] = {stripe, col, off, len, in_off} are those of the update call (ecg_update.h), whatever its mode.
 * d_delta[in_bytes] holds delta at the records' staging ranges: the d_delta_out of an ECG_UPDATE_WRITE call, or the
 * d_in of an ECG_UPDATE_DELTA call.
 *
 * The sum table.  d_sums[S][n_sums][Q] (unsigned, device, 4-byte aligned) is the store's recorded table: row s is
 * stripe s, column c is block sum_ids[c] (host array, distinct ids, 1 <= n_sums <= 128).
 *   piece_bytes = 0     Q = 1, one sum per block: the layout of ecg_sum_verify_batch's d_expected with
 *                       d_stripe_ids = NULL.
 *   piece_bytes = P     a power of two in [512, 2^30]: Q = ceil(B / P), piece q ends at min((q + 1) P, B): the layout of
 *                       ecg_psum_verify_batch's d_expected.
 * A block of src_ids / dst_ids that sum_ids does not name has no recorded sum and is skipped.
 *
 * `which` is a bit set: 1 = the record's data block, 2 = the parities with a nonzero coefficient in the record's
 * column.  A data holder that ships delta passes 1, a parity holder in ECG_UPDATE_DELTA mode 2, a node that holds all
 * 3.  0 or any other bit is ECG_EINVAL.
 *
 * Per record.  For every applied record, every block b it concerns (by `which`) and every piece q of b that
 * [off, off + len) meets, in [a, b') with piece end e:
 *         sums[stripe][col_of(b)][q] ^= raw(c_b * delta[a..b')) * x^(8 (e - b'))
 * with c_b = 1 for the data block and G[i][col] for parity dst_ids[i] (the product byte by byte).  Contributions are
 * XORed atomically: the result is exact whatever the launch geometry, the order, or the number of records that meet
 * one sum word.  Unlike in the update, overlapping records are not undefined here: they simply add.  A contribution
 * that is zero need not be stored.  No word of d_sums other than those named above is written, and the call never
 * zeroes d_sums.
 *
 * Record state and report.  The device validates every record as a whole; states 0-5 have the meaning and order of
 * ecg_update.h (0 applied, 1 stripe, 2 col, 3 off / len, 4 len > max_len, 5 staging range).  d_report[R][2] (unsigned)
 * holds {state, nonzero}: `nonzero` is the number of positions of the record with delta != 0, and 0 for a refused
 * record -- the update's `changed`, so a caller can hold the two reports against each other.  d_update_report, if not
 * NULL, is the [R][2] report of the update call: a record whose d_update_report[r][0] != 0 is reported with that state,
 * before any rule of this call is tried, and contributes nothing.  The call zeroes d_report on the stream first.
 *
 * Limits.  ECG_EINVAL with ecg_last_error() set, before any device is touched:
 *   - NULL pointers (d_update_report excepted);
 *   - k_in < 1, m_out < 1 or k_in + m_out > 128; more than 8 nonzero coefficients in a column;
 *   - ids that are negative, repeated within src_ids, within dst_ids or within sum_ids, or shared between src_ids and
 *     dst_ids; n_sums < 1 or n_sums > 128;
 *   - B < 0, B >= 2^31, S < 0, R < 0, max_len < 0, max_len > B or in_bytes < 0;
 *   - a piece_bytes that is neither 0 nor a power of two in [512, 2^30]; S * n_sums * Q >= 2^31 sum words;
 *   - a `which` outside 1 .. 3;
 *   - d_records not 8-byte aligned, d_sums not 4-byte aligned;
 *   - a launch that would need more than 2^31 - 1 workgroups (R * wg_per_record, see below);
 *   - in the `ec` form: a host-memory handle, or a class without an encoding matrix (the product codes).
 * R == 0 is a no-op returning 0.
 *
 * The launch.  One launch whatever the mix of records.  Chunks of chunk = 16 * cols_per_wg bytes (ECG_OPT_COLS_PER_WG
 * rounded up to a multiple of 128 columns, default 128 = 2 KiB) are cut on the BLOCK's own grid, so that piece borders
 * fall on chunk borders; a record gets wg_per_record = (chunk + max_len - 2) / chunk + 1 workgroups (1 for
 * max_len == 0), and one whose chunk lies past its record's end exits at once.  The alignment of in_off does not
 * matter.
 *
 * Links against libecg.so (include/ecg.h): same status codes, coefficient-table cache (the update's own entry), batch
 * scopes and streams.  All pointers are DEVICE pointers unless noted; `stream` is a hipStream_t (NULL = default stream)
 * and the calls are asynchronous on it.  A call flushes the thread's batch scope first.  No call allocates.
 */
#ifndef ECG_USUM_H
#define ECG_USUM_H

#include "ecg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ECG_USUM_DATA 1
#define ECG_USUM_PARITY 2

/* The primitive: G = coef (m_out x k_in, row-major) over data blocks src_ids[0..k_in) and parity blocks
 * dst_ids[0..m_out). */
int ecg_usum_matrix_batch(int k_in, int m_out, const int* coef, const int* src_ids, const int* dst_ids, long long B,
                          int S, const long long* d_records /* device, [R][5] */, int R, long long max_len,
                          const void* d_delta, long long in_bytes, const int* sum_ids /* host, [n_sums] */, int n_sums,
                          long long piece_bytes, int which, unsigned* d_sums /* [S][n_sums][Q] */,
                          const unsigned* d_update_report /* [R][2], or NULL */, unsigned* d_report /* [R][2] */,
                          void* stream);
/* G = matrix (m x k) over stripes of k+m blocks, data 0..k-1, coding k..k+m-1; sum_ids = 0..k+m-1. */
int ecg_usum_encode_batch(int k, int m, const int* matrix, long long B, int S, const long long* d_records, int R,
                          long long max_len, const void* d_delta, long long in_bytes, long long piece_bytes, int which,
                          unsigned* d_sums /* [S][k+m][Q] */, const unsigned* d_update_report, unsigned* d_report,
                          void* stream);
/* The class's own encoding matrix (ecg_ec_make_encoding_matrix); sum_ids = 0..k+m-1.  ECG_MEM_DEVICE handles only. */
int ecg_usum_ec_batch(ecg_ec* ec, long long B, int S, const long long* d_records, int R, long long max_len,
                      const void* d_delta, long long in_bytes, long long piece_bytes, int which, unsigned* d_sums,
                      const unsigned* d_update_report, unsigned* d_report, void* stream);
/* Host only, no device: the same definition on HOST arrays (h_records, h_delta, h_sums, h_update_report, h_report), one
 * record after the other, for callers and tests.  The limits above apply but the alignment and grid rules.  It reads
 * len bytes per record, so a block of 2^31 - 1 bytes costs no more than a small one. */
int ecg_usum_expected(int k_in, int m_out, const int* coef, const int* src_ids, const int* dst_ids, long long B, int S,
                      const long long* h_records, int R, long long max_len, const void* h_delta, long long in_bytes,
                      const int* sum_ids, int n_sums, long long piece_bytes, int which, unsigned* h_sums,
                      const unsigned* h_update_report, unsigned* h_report);
/* Host only: the bytes the records move by the definition.  Per record with len > 0 (all taken as applied, every block
 * taken as recorded): len bytes of delta read, and 8 bytes -- one word read and written -- per sum it meets:
 * pieces met * ((which & 1 ? 1 : 0) + (which & 2 ? nnz_per_col[col] : 0)). */
long long ecg_usum_traffic_bytes(const unsigned char* nnz_per_col /* [k_in] */, const long long* h_records, int R,
                                 long long B, long long piece_bytes, int which);
/* Usum kernels launched and records they covered, process-wide. */
int ecg_usum_counters(long long* launches, long long* records);
/* Launch geometry of the most recent usum launch, process-wide.  Five values, in order:
 *   v[0] cols_per_wg    16-byte columns of a block per workgroup
 *   v[1] wg_per_record  workgroups per record
 *   v[2] R              the records of the launch
 *   v[3] max_nnz        the most nonzero coefficients in a column
 *   v[4] piece_bytes    P, 0 for block sums
 * All zero before the first launch.  Host only.  Returns the number of values, 5; v is written when cap >= 5 (v may be
 * NULL with cap == 0). */
int ecg_usum_last_launch(int* v, int cap);

#ifdef __cplusplus
}
#endif
#endif /* ECG_USUM_H */
