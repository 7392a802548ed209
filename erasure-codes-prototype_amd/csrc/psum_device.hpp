// The table-driven CRC-32C folds of the piece checksums, device side: what the vector kernels of psum_kernels.hip and
// of vread_kernels.hip share, each in its own code object.  Everything here is inlined into the kernels that use it;
// the header defines no kernel and no host state.
//
// Every multiplication on the way to a piece's remainder is a table: four byte-indexed lookups in a 4 x 256-word LDS
// table per constant (* x^32, * x^(8 * 16 * 2^d) for d = 0..6, * x^(8 * 2048)), computed at compile time and fetched
// once per workgroup.  A 128-lane workgroup reads rows of 2 KiB, 16 bytes per lane:
//   * fold of a lane: its four dword states become the remainder of its 16 bytes, ((s0 x^32 ^ s1) x^32 ^ s2) x^32 ^ s3)
//     x^32, four passes through table 0;
//   * fold of G lanes (always inside a wave): a tree, level d computing v = T_d(v of the lane 2^d to the left) ^ v,
//     after which the group's last lane holds the remainder of the group's 16 G bytes;
//   * a lane's four chains go down the rows of a run by Horner with the row table.
#pragma once
#include "gf_kernels.hpp"
#include "psum_kernels.hpp"

namespace ecg {

static_assert(kPsumRowBytes == 16 * kThreads, "a row is one dwordx4 per lane");
static_assert(kThreads == 128, "two waves per row: the tree's level 6 is the step from wave 0 to the row's end");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---- compile-time tables

constexpr int kTabDword = 0, kTabLevel0 = 1, kTabLevel6 = 7, kTabRow = 8;

constexpr uint32_t table_multiplier(int k) {
    if (k == kTabDword) return crc_shift(kCrcOne, 4, kCrcPowers.p);
    if (k == kTabRow) return crc_shift(kCrcOne, kPsumRowBytes, kCrcPowers.p);
    return crc_shift(kCrcOne, 16ull << (k - kTabLevel0), kCrcPowers.p);
}

// t[(k * 4 + b) * 256 + v] = (v << 8 b) * multiplier k.  Linear in v: built from the 32 single bits.
struct PsumTables {
    uint32_t t[kPsumTablesRows * kPsumTableWords];
};
constexpr PsumTables make_tables() {
    PsumTables r{};
    for (int k = 0; k < kPsumTablesRows; ++k) {
        const uint32_t m = table_multiplier(k);
        for (int b = 0; b < 4; ++b) {
            uint32_t* t = r.t + (k * 4 + b) * 256;
            for (int v = 1; v < 256; ++v) {
                const int low = v & -v;
                t[v] = v == low ? crc_mul((uint32_t)v << (8 * b), m) : t[v ^ low] ^ t[low];
            }
        }
    }
    return r;
}

static __device__ const PsumTables kTables = make_tables();  // one copy per code object

// ---- device pieces

// The first TABLES tables into LDS, 16 bytes per lane and step.
template <int TABLES>
__device__ __forceinline__ void fetch_tables(uint32_t* tab) {
    for (int e = 4 * (int)threadIdx.x; e < TABLES * kPsumTableWords; e += 4 * kThreads)
        *reinterpret_cast<u32x4*>(tab + e) = *reinterpret_cast<const u32x4*>(kTables.t + e);
}

// a * (the multiplier of the table at tab)
__device__ __forceinline__ uint32_t tmul(const uint32_t* tab, uint32_t a) {
    return tab[a & 0xffu] ^ tab[256 + ((a >> 8) & 0xffu)] ^ tab[512 + ((a >> 16) & 0xffu)] ^ tab[768 + (a >> 24)];
}

// The remainder of a lane's 16 bytes from its four dword states.
__device__ __forceinline__ uint32_t lane_fold(const uint32_t* tab, const uint32_t (&s)[4]) {
    const uint32_t* const t32 = tab + kTabDword * kPsumTableWords;
    uint32_t f = tmul(t32, s[0]) ^ s[1];
    f = tmul(t32, f) ^ s[2];
    f = tmul(t32, f) ^ s[3];
    return tmul(t32, f);
}

// Level d of the tree: the lane 2^d to the left holds the remainder of the 2^d lanes that end there.
__device__ __forceinline__ uint32_t tree_level(const uint32_t* tab, uint32_t f, int d) {
    const uint32_t left = (uint32_t)__shfl_up((int)f, 1u << d, 64);
    return tmul(tab + (kTabLevel0 + d) * kPsumTableWords, left) ^ f;
}

// state = state * x^(8 * 2048) ^ word for a lane's four chains
__device__ __forceinline__ void row_step(const uint32_t* tab, uint32_t (&s)[4], const u32x4 w) {
    const uint32_t* const row = tab + kTabRow * kPsumTableWords;
    const uint32_t x[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int d = 0; d < 4; ++d) s[d] = tmul(row, s[d]) ^ x[d];
}

}  // namespace ecg
