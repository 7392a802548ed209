// Block checksums (sum_kernels.hip, libecg_sum.so): CRC-32C of every block of every selected stripe, its arithmetic
// and its launch descriptor.
//
//   sums[i * n + j] = crc32c(the B bytes of block src_ids[j] of stripe stripe_of[i])
//
// crc32c is the reflected CRC with polynomial 0x1EDC6F41 (reflected constant 0x82F63B78), initial value 0xFFFFFFFF
// and final XOR 0xFFFFFFFF (include/ecg_sum.h).  Everything here rests on its linearity over GF(2): with raw(d) the
// remainder for initial value 0 and no final XOR,
//   crc32c(d) = raw(d) ^ crc32c(0^len(d))          raw(A || B) = raw(A) * x^(8 |B|) ^ raw(B)      (mod P).
// A 32-bit value stands for a polynomial of degree < 32 in the reflected order: bit 31 is x^0, bit 0 is x^31, so a
// little-endian dword of data is the polynomial of its four bytes as the CRC reads them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ecg {

// ---- arithmetic mod P, shared by the host entry points (sum.cpp), the compile-time tables and the kernels

constexpr uint32_t kCrcPoly = 0x82F63B78u;  // P without x^32, reflected
constexpr uint32_t kCrcOne = 0x80000000u;   // x^0

// a * x
__host__ __device__ constexpr uint32_t crc_mulx(uint32_t a) { return (a >> 1) ^ (kCrcPoly & (0u - (a & 1u))); }

// a * b: the generic 32-step multiply
__host__ __device__ constexpr uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        p ^= b & (0u - ((a >> (31 - i)) & 1u));
        b = crc_mulx(b);
    }
    return p;
}

// x^(8 * 2^j), j in [0, 32): the power ladder's table.
struct CrcPowers {
    uint32_t p[32];
};
constexpr CrcPowers crc_make_powers() {
    CrcPowers t{};
    t.p[0] = kCrcOne >> 8;
    for (int j = 1; j < 32; ++j) t.p[j] = crc_mul(t.p[j - 1], t.p[j - 1]);
    return t;
}
inline constexpr CrcPowers kCrcPowers = crc_make_powers();

// a * x^(8 * bytes) for any 64-bit byte count.  The exponent in bits passes 2^32 from bytes = 2^29: the ladder walks
// the byte count, never 8 * bytes.  Bits 0..31 of the count take their power from pw; bits 32..63 (host callers only: a
// device block is shorter than 2^31) go on squaring from pw[31].
__host__ __device__ constexpr uint32_t crc_shift(uint32_t a, unsigned long long bytes, const uint32_t (&pw)[32]) {
    for (int j = 0; j < 32 && (bytes >> j) != 0; ++j)
        if ((bytes >> j) & 1u) a = crc_mul(a, pw[j]);
    uint32_t p = pw[31];
    for (int j = 32; j < 64 && (bytes >> j) != 0; ++j) {
        p = crc_mul(p, p);
        if ((bytes >> j) & 1u) a = crc_mul(a, p);
    }
    return a;
}

// ---- launch geometry

constexpr int kSumRowBytes = 2048;               // one workgroup row: kThreads lanes x 16 bytes
constexpr long long kSumAutoSegment = 256 << 10;  // auto segment: the 4.5 KiB of tables a workgroup fetches are 1.8 % of it
constexpr int kSumIds = 256;                     // STRIDED: block ids per launch (wider calls take several launches)
constexpr int kSumPtrs = 128;                    // INLINE: block pointers per launch
constexpr int kSumRunBytes = 64;                 // byte path: consecutive bytes per lane
constexpr int kSumCopies = 4;                    // table scheme 1: copies of every table entry in LDS (a power of two)

struct SumLaunch {
    union {
        int ids[kSumIds];                   // STRIDED: block id of column col0 + c
        const uint8_t* ptrs[kSumPtrs];      // INLINE: block pointer of column c
    } src;
    const uint8_t* base;                    // STRIDED
    long long sstride, bstride;
    const int* stripe_of;                   // [S] or nullptr: launch stripe i is stripe stripe_of[i]
    unsigned* sums;                         // [S][n], zeroed by the caller before the launch; XORed into
    long long B;
    long long lo, hi;                       // this launch covers bytes [lo, hi) of every block
    long long seg_bytes;                    // bytes per workgroup: a multiple of kSumRowBytes (vector path)
    int segs;                               // workgroups per block
    int S, n;                               // launch stripes; columns of a row of `sums`
    int col0, cols;                         // this launch covers columns [col0, col0 + cols)
    unsigned affine;                        // crc32c(0^B), XORed in by segment 0 -- or 0 when another launch of the
                                            // call does that
    uint32_t pw[32];                        // kCrcPowers
};

enum SumMode : int { SUM_MODE_INLINE = 0, SUM_MODE_STRIDED = 2 };  // the values of gf_kernels.hpp GfMode

// What a call of ecg_sum_verify_* compares once every sum is complete.
struct SumVerify {
    const unsigned* sums;      // [S][n]
    const unsigned* expected;  // [S][n]
    int* targets;              // [S]: -1 no column differs, j exactly column j does, n more than one
    unsigned* bad;             // [S]: columns that differ
    int S, n;
};

// The fields of ecg_sum_last_launch: path, segment_bytes, segments_per_block, blocks, table_scheme.
constexpr int kSumLaunchFields = 5;

// Sum bytes [0, B) of n blocks of S stripes into d_sums (zeroed here, on the stream): the vector path over
// [0, B & ~15) when vec_ok (every block 16-byte aligned), the byte path over the rest.  STRIDED takes src_ids (host,
// [n]) and base / strides, INLINE takes ptrs (host array of n <= kSumPtrs device pointers) and S == 1.
// segment_bytes: 0 = kSumAutoSegment.  table_scheme: -1 = auto (scheme 0), 0 one copy of the row tables in LDS, 1
// kSumCopies copies.  Returns a hipError_t; hipErrorInvalidConfiguration, before anything is zeroed, counted or
// launched, if a launch would need more than 2^31 - 1 workgroups (S * min(n, ids per launch) * segments per block).
hipError_t launch_sum(int mode, int n, const int* src_ids, const uint8_t* const* ptrs, const void* base,
                      long long sstride, long long bstride, long long B, const int* d_stripe_of, int S,
                      unsigned* d_sums, bool vec_ok, long long segment_bytes, int table_scheme, hipStream_t stream);
hipError_t launch_sum_verify(const SumVerify& v, hipStream_t stream);
// Kernels launched in this process and the bytes they read as planned (S * n * B per call).
void sum_traffic(long long* launches, long long* bytes);
// Geometry of the most recent call's main launch (the vector launch if it had one, else the byte launch); returns
// kSumLaunchFields, v is written when cap suffices.
int sum_last_launch(int* v, int cap);

}  // namespace ecg
