/*
 * ecg_update.h — delta update on the MI355X (gfx950): apply small overwrites to data and parity in place
 * (libecg_update.so).
 *
 * The check libraries (ecg_scrub.h .. ecg_restore.h) read stripes that already are codewords.  This is the write side:
 * it changes bytes of a stored data block and keeps the stripe a codeword without re-encoding it.  A re-encode moves
 * (k + m) * B bytes per stripe whatever the size of the change; the parity-delta path moves (3 + 2 * nnz) * len.
 *
 * Definition.  G is an m_out x k_in coefficient matrix over GF(2^8) / 0x11d.  Column j stands for the data block
 * src_ids[j], row i for the parity block dst_ids[i].  All blocks live in one strided layout: block b of stripe s is at
 * d_base + s*sstride + b*bstride, it has B bytes, and the layout has S stripes.  One call applies R records.  A record
 * is five int64 values in device memory, d_records[R][5]: {stripe, col, off, len, in_off}; its len input bytes are
 * d_in[in_off .. in_off+len), inside a staging buffer of in_bytes bytes.  Two modes:
 *   ECG_UPDATE_WRITE (0)  the input bytes are the new contents.  For every x in [off, off+len):
 *                           delta = data[x] ^ new[x];  data[x] = new[x];
 *                           parity_i[x] ^= G[i][col] * delta   for every row i with G[i][col] != 0.
 *                         If d_delta_out is not NULL, delta is also written to d_delta_out[in_off + (x - off)]: what a
 *                         data node ships to remote parity holders.
 *   ECG_UPDATE_DELTA (1)  the input bytes are delta itself.  The data block is neither read nor written; only the
 *                         parities change.  A non-NULL d_delta_out in this mode is ECG_EINVAL.
 * No other byte of memory changes, not even with its own value: two records may touch disjoint byte ranges that share a
 * 16-byte column, and different workgroups may handle them, so bytes outside a record's range are never stored to.
 * This holds for data, parity and d_delta_out.  Parity blocks whose coefficient in the record's column is zero are
 * neither read nor written (LRC local parities of other groups).  A 16-byte column whose delta is all zero is skipped
 * after delta_out: its data and parity bytes are not stored.
 *
 * Record state and report.  The device validates every record and refuses it as a whole: nothing of a refused record
 * is read or written.  d_report[R][2] (unsigned) holds {state, changed}.  The state is the first of these that applies:
 *         0  applied
 *         1  stripe not in [0, S)
 *         2  col not in [0, k_in)
 *         3  off < 0, len < 0 or off + len > B
 *         4  len > max_len
 *         5  in_off < 0 or in_off + len > in_bytes
 * `changed` is the number of positions of the record with delta != 0; it is 0 for a refused record.  The count is
 * exact and reproducible.  The call zeroes d_report on the stream before it launches.
 *
 * Disjointness.  Records of one call that name the same stripe must have pairwise disjoint ranges [off, off+len),
 * whatever their columns: otherwise two workgroups update the same parity bytes and the result on the shared range is
 * undefined.  The device does not check this (ecg_update_check_records does, on the host).  Touching ranges such as
 * [0,5) and [5,9) are legal.  The staging ranges [in_off, in_off+len) must also be pairwise disjoint when d_delta_out
 * is given.
 *
 * Limits.  ECG_EINVAL with ecg_last_error() set, before any device is touched:
 *   - NULL pointers (d_delta_out excepted);
 *   - k_in < 1, m_out < 1 or k_in + m_out > 128;
 *   - more than 8 nonzero coefficients in a column (one lane holds the parity columns of its record);
 *   - ids that are negative, repeated within src_ids or within dst_ids, or shared between the two;
 *   - B < 0, B >= 2^31, S < 0, R < 0, max_len < 0, max_len > B or in_bytes < 0;
 *   - a mode other than 0 or 1;
 *   - d_records not 8-byte aligned;
 *   - a launch that would need more than 2^31 - 1 workgroups (R * ceil((max_len + 15) / chunk), see below);
 *   - in the `ec` forms: a host-memory handle, or a class without an encoding matrix (the product codes).
 * R == 0 is a no-op returning 0.  With max_len == 0 no data or parity byte can move (every record with len > 0 is
 * state 4): the call still zeroes and fills the report, in one launch of one workgroup per record.
 * A column that is all zero is legal: in WRITE mode the record then only writes data and delta.
 *
 * The launch.  One launch whatever the mix of stripes, columns, offsets and lengths: R * ceil((max_len + 15) / chunk)
 * workgroups, chunk = 16 * cols_per_wg bytes (ECG_OPT_COLS_PER_WG, default 128 columns = 2 KiB).  A workgroup whose
 * chunk lies past its record's end exits at once, so max_len should be the batch's real maximum.  Chunks are cut on
 * the blocks' 16-byte grid; the alignment of in_off relative to off does not matter.  Partial first and last columns,
 * and layouts whose base or strides are not 16-byte aligned, move byte by byte.
 *
 * Links against libecg.so (include/ecg.h): same status codes, coefficient-table cache, batch scopes and streams.
 * All pointers are DEVICE pointers unless noted; `stream` is a hipStream_t (NULL = default stream) and the calls are
 * asynchronous on it.  A call flushes the thread's batch scope first (it sees the recorded calls' results).  No call
 * allocates.  Checksums (ecg_sum.h, ecg_psum.h) are not updated: re-sum the touched stripes, or carry the recorded sums
 * through the same records from delta alone with ecg_usum.h.
 */
#ifndef ECG_UPDATE_H
#define ECG_UPDATE_H

#include "ecg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ECG_UPDATE_WRITE 0
#define ECG_UPDATE_DELTA 1

/* The primitive: G = coef (m_out x k_in, row-major) over data blocks src_ids[0..k_in) and parity blocks
 * dst_ids[0..m_out) of the strided layout. */
int ecg_update_matrix_batch(int k_in, int m_out, const int* coef, const int* src_ids, const int* dst_ids, void* d_base,
                            long long sstride, long long bstride, long long B, int S, int mode,
                            const long long* d_records /* device, [R][5] */, int R, long long max_len,
                            const void* d_in, long long in_bytes, void* d_delta_out /* in_bytes, or NULL */,
                            unsigned* d_report /* [R][2] */, void* stream);
/* G = matrix (m x k) over stripes of k+m blocks: data are blocks 0..k-1, coding blocks k..k+m-1 (the layout of
 * ecg_decode_batch). */
int ecg_update_encode_batch(int k, int m, const int* matrix, void* d_stripes, long long sstride, long long bstride,
                            long long B, int S, int mode, const long long* d_records, int R, long long max_len,
                            const void* d_in, long long in_bytes, void* d_delta_out, unsigned* d_report, void* stream);
/* The class's own encoding matrix (ecg_ec_make_encoding_matrix) over strided stripes.  ECG_MEM_DEVICE handles only. */
int ecg_update_ec_batch(ecg_ec* ec, void* d_stripes, long long sstride, long long bstride, long long B, int S, int mode,
                        const long long* d_records, int R, long long max_len, const void* d_in, long long in_bytes,
                        void* d_delta_out, unsigned* d_report, void* stream);
/* One record on one stripe through its block pointers, on the handle's stream: bytes [off, off+len) of data block
 * `col`, the input at d_in[0 .. len), delta (WRITE, optional) at d_delta_out[0 .. len).  The record travels in the
 * kernel arguments; states 1, 4 and 5 cannot occur. */
int ecg_update_ec(ecg_ec* ec, char** d_data_ptrs, char** d_coding_ptrs, int block_size, int mode, int col,
                  long long off, long long len, const void* d_in, void* d_delta_out, unsigned* d_report /* [2] */);
/* Host only, no device: -1 if every record of h_records[R][5] is state 0 and the disjointness rules hold (staging
 * ranges are compared when with_delta_out != 0; empty ranges overlap nothing).  Otherwise the index of the first
 * offending record -- the first that is refused, or that overlaps a record before it -- with ecg_last_error() saying
 * which rule broke.  ECG_EINVAL (-2) for a NULL array or a negative R. */
int ecg_update_check_records(const long long* h_records, int R, int k_in, long long B, int S, long long max_len,
                             long long in_bytes, int with_delta_out);
/* Host only: the bytes the records move by the definition, len * ((mode == WRITE ? 3 : 1) + (with_delta_out ? 1 : 0)
 * + 2 * nnz_per_col[col]) summed over the records (all taken as applied; len <= 0 counts nothing). */
long long ecg_update_traffic_bytes(const unsigned char* nnz_per_col /* [k_in] */, const long long* h_records, int R,
                                   int mode, int with_delta_out);
/* Update kernels launched and records they covered, process-wide.  The lengths live on the device, so this counts
 * records, not bytes. */
int ecg_update_counters(long long* launches, long long* records);
/* Launch geometry of the most recent update launch that covered 16-byte columns, process-wide.  Four values, in order:
 *   v[0] cols_per_wg    16-byte columns per workgroup
 *   v[1] wg_per_record  workgroups per record
 *   v[2] R              the records of the launch
 *   v[3] max_nnz        the most nonzero coefficients in a column
 * All zero before the first such launch; launches over an unaligned layout (byte lanes only) and launches with
 * max_len == 0 do not change it.  Host only.  Returns the number of values, 4; v is written when cap >= 4 (v may be
 * NULL with cap == 0). */
int ecg_update_last_launch(int* v, int cap);

#ifdef __cplusplus
}
#endif
#endif /* ECG_UPDATE_H */
