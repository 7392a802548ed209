/*
 * ecg_psum.h — piece checksums on the MI355X (gfx950): CRC-32C of every fixed-size piece of every stored block,
 * computed where the blocks are (libecg_psum.so).
 *
 * ecg_sum.h gives the store's last word for whole blocks.  Stores that keep CRC-32C keep it per fixed-size piece of a
 * block -- HDFS one sum per 512 bytes, Ceph one per 4 KiB -- and piece sums say what block sums cannot: WHERE in a
 * block the damage is.  A verify at piece granularity names, per piece row, the one block that differs, so blocks
 * damaged at disjoint positions are corrected however many they are: a piece row of a strided batch is itself a
 * strided "stripe" of piece_bytes-long blocks, and its d_targets plug into ecg_heal_* TARGET and ecg_heal2_* TARGET2
 * unchanged (ecg_psum.py heal_rows builds the views).
 *
 * Definition.  crc32c is the CRC-32C of ecg_sum.h: initial value and final XOR 0xFFFFFFFF.  P = piece_bytes is a
 * power of two, 512 <= P <= 2^30; Q = ceil(B / P); piece q of a block is its bytes [q P, min((q + 1) P, B)), so the
 * last piece may be shorter than P, down to one byte, and P >= B gives Q = 1.
 *         sums[i][j][q] = crc32c(piece q of block src_ids[j] of stripe d_stripe_ids[i])
 * The sums are exact and reproducible whatever the launch geometry.  Every stored byte of a selected block is read
 * once (n * B per stripe, see ecg_psum_counters) and nothing is written but the outputs.
 *
 * Verify works per piece row (i, q).  With expected[i][j][q] the sums the store recorded, bad[i][q] is the number of
 * columns j with sums[i][j][q] != expected[i][j][q], and targets[i][q] is -1 if there is none, j if exactly column j
 * differs, and n if more than one does: the three values of ecg_sum_verify_batch, with the same meaning.  Both -1 and
 * n lie outside [0, n): the heal's rule (ecg_heal.h) leaves such a row read, counted and unwritten.  The compare runs
 * after every sum of the call is complete, as a second small launch on the stream.
 *
 * Links against libecg.so (include/ecg.h): same status codes, ecg_last_error, batch scopes and streams.
 * All pointers are DEVICE pointers unless noted; `stream` is a hipStream_t (NULL = default stream) and the calls are
 * asynchronous on it.  A call flushes the thread's batch scope first (it sees the recorded calls' results), zeroes
 * `d_sums` on the stream, then launches: once it completes d_sums holds this call's result, not an accumulation.
 *
 * Arguments: NULL pointers (d_stripe_ids excepted), negative sizes, B >= 2^31, n < 1, n > 128 for the pointer form,
 * host-memory handles, a piece_bytes that is not a power of two in [512, 2^30], and S_sel * n * Q >= 2^31 output
 * words are ECG_EINVAL before any device is touched, with ecg_last_error() set; otherwise S_sel == 0 or B == 0 is a
 * no-op returning 0 that leaves every output untouched.  Blocks, strides or a base that are not 16-byte aligned, and
 * the last B % 16 bytes of a block (they belong to the last piece), run a byte kernel: slow, and correct.
 * One launch holds at most 2^31 - 1 workgroups: a call with S_sel * min(n, 256) * ceil(B / span) beyond that returns
 * ECG_EHIP with ecg_last_error() set before anything is zeroed, counted or launched.
 *
 * Stripe selection: d_stripe_ids is a device array of S_sel stripe indices (int32), NULL = 0 .. S_sel-1.  Row i of
 * d_sums, d_expected, d_targets and d_bad belongs to stripe d_stripe_ids[i].  Duplicate ids are allowed: nothing is
 * written to the stripes.
 */
#ifndef ECG_PSUM_H
#define ECG_PSUM_H

#include "ecg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The primitive: blocks src_ids[0..n) (host array) of every selected stripe, block b of stripe s at
 * d_base + s*sstride + b*bstride. */
int ecg_psum_pieces_batch(int n, const int* src_ids, const void* d_base, long long sstride, long long bstride,
                          long long B, long long piece_bytes,
                          const int* d_stripe_ids /* device, [S_sel]; NULL = 0..S_sel-1 */, int S_sel,
                          unsigned* d_sums /* [S_sel][n][Q] */, void* stream);
int ecg_psum_verify_batch(int n, const int* src_ids, const void* d_base, long long sstride, long long bstride,
                          long long B, long long piece_bytes, const int* d_stripe_ids, int S_sel,
                          const unsigned* d_expected /* [S_sel][n][Q] */,
                          unsigned* d_sums /* [S_sel][n][Q], the computed sums; required */,
                          int* d_targets /* [S_sel][Q] */, unsigned* d_bad /* [S_sel][Q] */, void* stream);
/* All k+m blocks of an ErasureCode handle's stripes, blocks 0..k+m-1 in the layout of ecg_decode_batch; n = k + m.
 * ECG_MEM_DEVICE handles only. */
int ecg_psum_ec_batch(ecg_ec* ec, const void* d_stripes, long long sstride, long long bstride, long long B,
                      long long piece_bytes, const int* d_stripe_ids, int S_sel,
                      unsigned* d_sums /* [S_sel][k+m][Q] */, void* stream);
int ecg_psum_verify_ec_batch(ecg_ec* ec, const void* d_stripes, long long sstride, long long bstride, long long B,
                             long long piece_bytes, const int* d_stripe_ids, int S_sel, const unsigned* d_expected,
                             unsigned* d_sums, int* d_targets, unsigned* d_bad, void* stream);
/* One stripe through its block pointers (host arrays of k and m device pointers), on the handle's stream;
 * k + m <= 128. */
int ecg_psum_ec(ecg_ec* ec, char** d_data_ptrs, char** d_coding_ptrs, int block_size, long long piece_bytes,
                unsigned* d_sums /* [k+m][Q] */);

/* Host only: the crc32c of a block of B bytes from its Q = ceil(B / piece_bytes) piece sums (HOST array), in
 * O(Q log piece_bytes): what ecg_sum_blocks_batch gives for the block.  Q == 0 with B == 0: 0.  A Q that is not
 * ceil(B / piece_bytes), a bad piece_bytes, negative sizes or NULL with Q > 0: 0 with ecg_last_error() set. */
unsigned ecg_psum_fold(const unsigned* h_sums, long long Q, long long piece_bytes, long long B);
/* Kernels launched and bytes they read as planned, process-wide: S_sel * n * B per call (the verify's compare is a
 * launch that reads no block). */
int ecg_psum_counters(long long* launches, long long* bytes);
/* Launch geometry of the most recent call's main launch (the vector launch over the 16-byte columns if the call had
 * one, else its byte launch), process-wide.  Five values, in order:
 *   v[0] path                0 vector (dwordx4 rows through the LDS tables), 1 byte (tails, unaligned blocks)
 *   v[1] piece_bytes         P
 *   v[2] pieces_per_block    Q
 *   v[3] blocks              S_sel * n
 *   v[4] span_bytes          bytes of one block that one workgroup covers
 * All zero before the first launch.  Host only.  Returns the number of values, 5; v is written when cap >= 5 (v may
 * be NULL with cap == 0). */
int ecg_psum_last_launch(int* v, int cap);
/* Bytes of a block per workgroup on the vector path, process-wide: 0 = auto (256 KiB, or the whole block if it is
 * shorter), otherwise a multiple of the workgroup's 2 KiB row; anything else is ECG_EINVAL.  The sums do not depend
 * on it.  A knob for tests, which reach many workgroups per block and a piece split over workgroups at blocks of a few
 * KiB with it. */
int ecg_psum_set_span_bytes(long long bytes);

#ifdef __cplusplus
}
#endif
#endif /* ECG_PSUM_H */
