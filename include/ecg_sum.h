/*
 * ecg_sum.h — block checksums on the MI355X (gfx950): CRC-32C of every stored block, computed where the blocks are
 * (libecg_sum.so).
 *
 * The scrub (ecg_scrub.h), the locate (ecg_locate.h) and the heals (ecg_heal.h, ecg_heal2.h) all end at "the store's
 * own block checksums remain the last word".  This is that word for blocks resident in HBM: a read-only pass that
 * sums every block of every selected stripe, and a verify whose output is exactly the d_targets array that
 * ecg_heal_* TARGET and ecg_heal2_* TARGET2 take.
 *
 * Definition.  crc32c(bytes) is the reflected CRC with polynomial 0x1EDC6F41 (reflected constant 0x82F63B78),
 * initial value 0xFFFFFFFF and final XOR 0xFFFFFFFF: CRC-32C (Castagnoli), the checksum of iSCSI, ext4, Ceph and
 * RocksDB.  Known answers:
 *         "123456789"   0xE3069283          bytes 0..31    0x46DD794E
 *         32 x 0x00     0x8A9136AA          bytes 31..0    0x113FDB5C
 *         32 x 0xFF     0x62A8AB43          one 0x00 byte  0x527D5351          empty  0
 * sums[i][j] is the crc32c of the B bytes of block src_ids[j] of stripe d_stripe_ids[i].  The sums are exact and
 * reproducible whatever the launch geometry.  Every stored byte of a selected block is read once (n * B per stripe,
 * see ecg_sum_counters) and nothing is written but the outputs.
 *
 * Verify.  With expected[i][j] the sums the store recorded, bad[i] is the number of columns j with
 * sums[i][j] != expected[i][j], and targets[i] is -1 if there is none, j if exactly column j differs, and n if more
 * than one does.  Both -1 and n lie outside [0, n): the heal's rule (ecg_heal.h) leaves such a stripe read, counted
 * and unwritten.  The compare runs after every sum of the call is complete, as a second small launch on the stream.
 *
 * Links against libecg.so (include/ecg.h): same status codes, ecg_last_error, batch scopes and streams.
 * All pointers are DEVICE pointers unless noted; `stream` is a hipStream_t (NULL = default stream) and the calls are
 * asynchronous on it.  A call flushes the thread's batch scope first (it sees the recorded calls' results), zeroes
 * `d_sums` on the stream, then launches: once it completes d_sums holds this call's result, not an accumulation.
 *
 * Arguments: NULL pointers (d_stripe_ids excepted), negative sizes, B >= 2^31, n < 1, n > 128 for the pointer form
 * and host-memory handles are ECG_EINVAL before any device is touched, with ecg_last_error() set; otherwise
 * S_sel == 0 or B == 0 is a no-op returning 0 that leaves every output untouched -- not even the zeros that the
 * crc32c of an empty block would be.  Blocks, strides or a base that are not 16-byte aligned, and the last B % 16
 * bytes of a block, run a byte kernel: slow, and correct.
 * One launch holds at most 2^31 - 1 workgroups: a call with S_sel * min(n, 256) * ceil(B / segment) beyond that (a
 * forced 2 KiB segment over a large store; the auto segment is 256 KiB) returns ECG_EHIP with ecg_last_error() set
 * before anything is zeroed, counted or launched.
 *
 * Stripe selection: d_stripe_ids is a device array of S_sel stripe indices (int32), NULL = 0 .. S_sel-1.  Row i of
 * d_sums, d_expected, and d_targets[i] and d_bad[i], belong to stripe d_stripe_ids[i], as d_targets does in
 * ecg_heal.h.  Duplicate ids are allowed: nothing is written to the stripes.
 */
#ifndef ECG_SUM_H
#define ECG_SUM_H

#include "ecg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The primitive: blocks src_ids[0..n) (host array) of every selected stripe, block b of stripe s at
 * d_base + s*sstride + b*bstride. */
int ecg_sum_blocks_batch(int n, const int* src_ids, const void* d_base, long long sstride, long long bstride,
                         long long B, const int* d_stripe_ids /* device, [S_sel]; NULL = 0..S_sel-1 */, int S_sel,
                         unsigned* d_sums /* [S_sel][n] */, void* stream);
int ecg_sum_verify_batch(int n, const int* src_ids, const void* d_base, long long sstride, long long bstride,
                         long long B, const int* d_stripe_ids, int S_sel, const unsigned* d_expected /* [S_sel][n] */,
                         unsigned* d_sums /* [S_sel][n], the computed sums; required */, int* d_targets /* [S_sel] */,
                         unsigned* d_bad /* [S_sel] */, void* stream);
/* All k+m blocks of an ErasureCode handle's stripes, blocks 0..k+m-1 in the layout of ecg_decode_batch; n = k + m.
 * ECG_MEM_DEVICE handles only. */
int ecg_sum_ec_batch(ecg_ec* ec, const void* d_stripes, long long sstride, long long bstride, long long B,
                     const int* d_stripe_ids, int S_sel, unsigned* d_sums /* [S_sel][k+m] */, void* stream);
int ecg_sum_verify_ec_batch(ecg_ec* ec, const void* d_stripes, long long sstride, long long bstride, long long B,
                            const int* d_stripe_ids, int S_sel, const unsigned* d_expected, unsigned* d_sums,
                            int* d_targets, unsigned* d_bad, void* stream);
/* One stripe through its block pointers (host arrays of k and m device pointers), on the handle's stream;
 * k + m <= 128. */
int ecg_sum_ec(ecg_ec* ec, char** d_data_ptrs, char** d_coding_ptrs, int block_size, unsigned* d_sums /* [k+m] */);

/* Host only: the crc32c of len bytes of HOST memory (len == 0: 0; NULL with len > 0 or len < 0: 0 with
 * ecg_last_error() set). */
unsigned ecg_sum_crc32c(const void* host_bytes, long long len);
/* Host only: crc32c(A || B) from crc_a = crc32c(A), crc_b = crc32c(B) and len_b = |B|, any value in
 * [0, 2^63) -- pieces of 4 GiB and more included --, in O(log len_b) (len_b < 0: 0 with ecg_last_error() set) -- for a
 * store that keeps sums of sub-block pieces.  The kernels' position multipliers use the same arithmetic. */
unsigned ecg_sum_combine(unsigned crc_a, unsigned crc_b, long long len_b);
/* Kernels launched and bytes they read as planned, process-wide: S_sel * n * B per call (the verify's compare is a
 * launch that reads no block). */
int ecg_sum_counters(long long* launches, long long* bytes);
/* Launch geometry of the most recent call's main launch (the vector launch over the 16-byte columns if the call had
 * one, else its byte launch), process-wide.  Five values, in order:
 *   v[0] path                0 vector (dwordx4 rows through the LDS tables), 1 byte (tails, unaligned blocks)
 *   v[1] segment_bytes       bytes of one block that one workgroup sums
 *   v[2] segments_per_block  workgroups per block
 *   v[3] blocks              S_sel * n
 *   v[4] table_scheme        LDS layout of the row tables the vector launch ran: 0 = one copy (4 x 256 x 4 B),
 *                            1 = C copies of every entry, a lane reading copy lane % C (fewer bank conflicts,
 *                            C times the LDS; C = kSumCopies of csrc/sum_kernels.hpp); 0 for a byte launch
 * All zero before the first launch.  Host only.  Returns the number of values, 5; v is written when cap >= 5 (v may
 * be NULL with cap == 0). */
int ecg_sum_last_launch(int* v, int cap);
/* Bytes of a block per workgroup on the vector path, process-wide: 0 = auto (256 KiB, or the whole block if it is
 * shorter), otherwise a multiple of the workgroup's 2 KiB row; anything else is ECG_EINVAL.  A knob for tests, which
 * reach many-segment blocks at small B with it. */
int ecg_sum_set_segment_bytes(long long bytes);
/* The LDS layout of the row tables, process-wide: -1 = auto (the faster one as measured), 0 or 1 as
 * table_scheme above; anything else is ECG_EINVAL.  The sums do not depend on it.  A knob for tests and measurements. */
int ecg_sum_set_table_scheme(int scheme);

#ifdef __cplusplus
}
#endif
#endif /* ECG_SUM_H */
