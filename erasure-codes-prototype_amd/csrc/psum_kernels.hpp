// Piece checksums (psum_kernels.hip, libecg_psum.so): CRC-32C of every fixed-size piece of every block of every
// selected stripe, and their launch descriptor.
//
//   sums[(i * n + j) * Q + q] = crc32c(bytes [q P, min((q + 1) P, B)) of block src_ids[j] of stripe stripe_of[i])
//
// P = piece_bytes is a power of two in [kPsumMinPiece, kPsumMaxPiece], Q = ceil(B / P).  The CRC, its arithmetic mod
// the polynomial and the power ladder are those of the block checksums (sum_kernels.hpp), included and not restated.
#pragma once
#include "sum_kernels.hpp"

namespace ecg {

constexpr long long kPsumMinPiece = 512;
constexpr long long kPsumMaxPiece = 1LL << 30;
constexpr int kPsumRowBytes = kSumRowBytes;      // one workgroup row: kThreads lanes x 16 bytes
// Auto span, the bytes of one block that one workgroup covers: the 36 KiB of tables a workgroup fetches (from L2, after
// the first) are 14 % of it, and a store of a few thousand 1 MiB blocks still gives every CU several workgroups.
constexpr long long kPsumAutoSpan = 256 << 10;
constexpr int kPsumIds = kSumIds;                // STRIDED: block ids per launch (wider calls take several launches)
constexpr int kPsumPtrs = kSumPtrs;              // INLINE: block pointers per launch
constexpr int kPsumRunBytes = kSumRunBytes;      // byte path: consecutive bytes per lane; divides kPsumMinPiece

// The multiplication tables a workgroup keeps in LDS, 4 x 256 words each (one byte table per byte of the operand):
// table 0 is * x^32 (the dword step), table 1 + d is * x^(8 * 16 * 2^d), the tree's level d over 2^d lanes (d < 6
// inside a wave, d = 6 from wave 0 to the row's end), table 8 is * x^(8 * 2048), the row step.
constexpr int kPsumTableWords = 4 * 256;
constexpr int kPsumTablesSmall = 7;              // P < 2048: the dword step and levels 0..5
constexpr int kPsumTablesRows = 9;               // P >= 2048: all of them

struct PsumLaunch {
    union {
        int ids[kPsumIds];                   // STRIDED: block id of column col0 + c
        const uint8_t* ptrs[kPsumPtrs];      // INLINE: block pointer of column c
    } src;
    const uint8_t* base;                     // STRIDED
    long long sstride, bstride;
    const int* stripe_of;                    // [S] or nullptr: launch stripe i is stripe stripe_of[i]
    unsigned* sums;                          // [S][n][Q], zeroed by the caller before the launch; XORed into
    long long B, P, Q;
    long long lo, hi;                        // this launch covers bytes [lo, hi) of every block
    long long span;                          // bytes of a block per workgroup: a multiple of kPsumRowBytes (vector path)
    int segs;                                // workgroups per block
    int S, n;                                // launch stripes; columns of a row of `sums`
    int col0, cols;                          // this launch covers columns [col0, col0 + cols)
    unsigned affine_full, affine_last;       // crc32c(0^P); crc32c(0^(B - (Q - 1) P)), the last piece's
    uint32_t pw[32];                         // kCrcPowers
};

// What a call of ecg_psum_verify_* compares once every sum is complete: one lane per piece row (i, q).
struct PsumVerify {
    const unsigned* sums;      // [S][n][Q]
    const unsigned* expected;  // [S][n][Q]
    int* targets;              // [S][Q]: -1 no column differs, j exactly column j does, n more than one
    unsigned* bad;             // [S][Q]: columns that differ
    long long Q;
    int S, n;
};

// The fields of ecg_psum_last_launch: path, piece_bytes, pieces_per_block, blocks, span_bytes.
constexpr int kPsumLaunchFields = 5;

// Sum the pieces of bytes [0, B) of n blocks of S stripes into d_sums (zeroed here, on the stream): the vector path
// over [0, B & ~15) when vec_ok (every block 16-byte aligned), the byte path over the rest.  Modes and sources as
// launch_sum (sum_kernels.hpp).  span_bytes: 0 = kPsumAutoSpan.  Returns a hipError_t; hipErrorInvalidConfiguration,
// before anything is zeroed, counted or launched, if a launch would need more than 2^31 - 1 workgroups.
hipError_t launch_psum(int mode, int n, const int* src_ids, const uint8_t* const* ptrs, const void* base,
                       long long sstride, long long bstride, long long B, long long P, const int* d_stripe_of, int S,
                       unsigned* d_sums, bool vec_ok, long long span_bytes, hipStream_t stream);
hipError_t launch_psum_verify(const PsumVerify& v, hipStream_t stream);
// Kernels launched in this process and the bytes they read as planned (S * n * B per call).
void psum_traffic(long long* launches, long long* bytes);
// Geometry of the most recent call's main launch (the vector launch if it had one, else the byte launch); returns
// kPsumLaunchFields, v is written when cap suffices.
int psum_last_launch(int* v, int cap);

}  // namespace ecg
