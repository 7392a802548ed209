// Block checksums for MI355X (gfx950, CDNA4): CRC-32C of every block of every selected stripe.
//
//   sums[i * n + j] = crc32c(block src_ids[j] of stripe stripe_of[i])        (sum_kernels.hpp: definition, arithmetic)
//
// gfx950 has no CRC and no carry-less multiply instruction; the sum is parallel because it is linear over GF(2).
// A 128-lane workgroup owns one SEGMENT of one block and reads it in rows of 2 KiB, one non-temporal dwordx4 per lane.
// Every (lane, dword) keeps a 32-bit state and runs Horner down the rows,
//       state = M(state) ^ word,        M = multiplication by x^(8 * 2048) mod P,
// the same M for every lane and dword: four byte-indexed lookups in LDS tables (kRowTables, 4 x 256 x 4 B, computed at
// compile time and fetched once per workgroup).  A lane's four dwords are four independent chains, and the loads of two
// rows are in flight while a third goes through the tables.  At the segment's end a lane folds its four states with
// the ordinary dword step (* x^32), multiplies by its distance to the segment's end (kLaneTable, a generic 32-step
// multiply), the workgroup XOR-reduces, and one lane multiplies by x^(8 * bytes after the segment) with the power
// ladder of the kernel arguments and XORs the result into sums[i][j] with one atomic.  XOR commutes: the sums are exact
// and reproducible whatever the grid.  Segment 0 also XORs in crc32c(0^B), the affine term.
// Rows are aligned to the segment's END, so a ragged segment (the last of a block whose vector part is no multiple of
// the segment) has its missing bytes in FRONT, where zeros cost nothing: only a segment's first row masks lanes.
// The lookups are what bounds the kernel: random bytes into one 256-entry table conflict about 3-way in the LDS banks
// (DESIGN.md 4m).  Table scheme 1 keeps kSumCopies copies of every entry, a lane reading copy lane % kSumCopies; it
// measured slower at every copy count (fewer resident waves), so scheme 0 is what a call runs unless told otherwise.
// The byte path (tails, unaligned blocks) is a per-lane bitwise loop over kSumRunBytes consecutive bytes and the same
// ladder per lane: slow, and correct.
#include <string.h>

#include "launch_rule.hpp"
#include "sum_kernels.hpp"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "sum_kernels.hip is gfx950 (CDNA4) code"
#endif

namespace ecg {

namespace {

static_assert(kSumRowBytes == 16 * kThreads, "a row is one dwordx4 per lane");
static_assert(kThreads % 64 == 0 && kThreads <= 256, "whole waves; the table fetch below");
static_assert((kSumCopies & (kSumCopies - 1)) == 0 && kSumCopies > 1, "a lane's copy is lane % C");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---- compile-time tables

constexpr uint32_t kRowMul = crc_shift(kCrcOne, kSumRowBytes, kCrcPowers.p);  // x^(8 * 2048)

// t[b * 256 + v] = (v << 8 b) * x^(8 * 2048): the four byte tables of M.  Linear in v: built from the 32 single bits.
struct RowTables {
    uint32_t t[4 * 256];
};
constexpr RowTables make_row_tables() {
    RowTables r{};
    for (int b = 0; b < 4; ++b)
        for (int v = 1; v < 256; ++v) {
            const int low = v & -v;
            r.t[b * 256 + v] = v == low ? crc_mul((uint32_t)v << (8 * b), kRowMul)
                                        : r.t[b * 256 + (v ^ low)] ^ r.t[b * 256 + low];
        }
    return r;
}

// d[l] = x^(8 * (2048 - 16 (l + 1)) + 32): the bytes of a row after lane l's 16, and the x^32 that turns the sum of
// words into a remainder.
struct LaneTable {
    uint32_t d[kThreads];
};
constexpr LaneTable make_lane_table() {
    LaneTable r{};
    const uint32_t step = crc_shift(kCrcOne, 16, kCrcPowers.p);
    r.d[kThreads - 1] = crc_shift(kCrcOne, 4, kCrcPowers.p);
    for (int l = kThreads - 2; l >= 0; --l) r.d[l] = crc_mul(r.d[l + 1], step);
    return r;
}

__device__ const RowTables kRowTables = make_row_tables();
__device__ const LaneTable kLaneTable = make_lane_table();

// ---- device pieces

template <int MODE>
__device__ __forceinline__ const uint8_t* block_ptr(const SumLaunch& a, int i, int c) {
    if constexpr (MODE == SUM_MODE_INLINE) return a.src.ptrs[c];
    else {
        const long long st = a.stripe_of ? (long long)a.stripe_of[i] : (long long)i;
        return a.base + st * a.sstride + (long long)a.src.ids[c] * a.bstride;
    }
}

// blockIdx.x -> (launch stripe, column of this launch, segment): a block's segments are adjacent workgroups
__device__ __forceinline__ void sum_coords(const SumLaunch& a, int& i, int& c, int& g) {
    const unsigned blk = blockIdx.x / (unsigned)a.segs;
    g = (int)(blockIdx.x % (unsigned)a.segs);
    i = (int)(blk / (unsigned)a.cols);
    c = (int)(blk % (unsigned)a.cols);
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v ^= (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

// a * x^32, the ordinary dword step
__device__ __forceinline__ uint32_t dword_step(uint32_t a) {
#pragma unroll
    for (int i = 0; i < 32; ++i) a = crc_mulx(a);
    return a;
}

__device__ __forceinline__ u32x4 load_row(const uint8_t* p) {
    return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
}

// state = M(state) ^ word for a lane's four chains.  `tab` is the lane's view of the tables: entry e of byte table b
// is tab[(b * 256 + e) * C], the lane's own copy of it (C = 1: the one copy).
template <int C>
__device__ __forceinline__ void row_step(const uint32_t* tab, uint32_t (&s)[4], const u32x4 w) {
    const uint32_t x[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int d = 0; d < 4; ++d)
        s[d] = tab[(s[d] & 0xffu) * C] ^ tab[(256 + ((s[d] >> 8) & 0xffu)) * C] ^
               tab[(512 + ((s[d] >> 16) & 0xffu)) * C] ^ tab[(768 + (s[d] >> 24)) * C] ^ x[d];
}

// Vector path: bytes [0, hi) of every block, hi a multiple of 16, every block 16-byte aligned.
// grid.x = S * cols * segs.  C = copies of every table entry in LDS (table scheme 0: 1; scheme 1: kSumCopies, entry e's
// copy c at word e * C + c, read by the lanes with lane % C == c, so that lanes of one bank group that look up
// different entries meet in a bank C times less often).
template <int MODE, int C>
__global__ void __launch_bounds__(kThreads) crc_sum_kernel(const SumLaunch a) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[4 * 256 * C];
    __shared__ uint32_t part[kThreads / 64];
    const int t = threadIdx.x;
#pragma unroll
    for (int e = 4 * t; e < 4 * 256; e += 4 * kThreads) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(kRowTables.t + e);
        const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int c = 0; c < C; ++c) tab[(e + u) * C + c] = x[u];
    }
    const uint32_t* const my = tab + (t & (C - 1));
    const uint32_t lane_mul = kLaneTable.d[t];

    int i, c, g;
    sum_coords(a, i, c, g);
    const uint8_t* p = block_ptr<MODE>(a, i, c);
    const long long s0 = (long long)g * a.seg_bytes;
    const long long s1 = min(s0 + a.seg_bytes, a.hi);
    const int T = (int)((s1 - s0 + kSumRowBytes - 1) / kSumRowBytes);
    // row r of this lane is at off + r * 2048; only row 0 can start before the segment
    const long long off = s1 - (long long)T * kSumRowBytes + 16 * t;
    const uint8_t* q = p + off;
    const u32x4 zero = {0u, 0u, 0u, 0u};

    u32x4 r0 = off >= s0 ? load_row(q) : zero;
    u32x4 r1 = T > 1 ? load_row(q + kSumRowBytes) : zero;
    __syncthreads();  // the tables are in LDS

    uint32_t s[4] = {0u, 0u, 0u, 0u};
    int r = 0;
    for (; r + 1 < T; r += 2) {
        u32x4 n0 = zero, n1 = zero;
        if (r + 2 < T) n0 = load_row(q + (long long)(r + 2) * kSumRowBytes);
        if (r + 3 < T) n1 = load_row(q + (long long)(r + 3) * kSumRowBytes);
        row_step<C>(my, s, r0);
        row_step<C>(my, s, r1);
        r0 = n0;
        r1 = n1;
    }
    if (r < T) row_step<C>(my, s, r0);

    // the lane's 16 bytes as one remainder-to-be, then its distance to the segment's end
    uint32_t f = dword_step(s[0]) ^ s[1];
    f = dword_step(f) ^ s[2];
    f = dword_step(f) ^ s[3];
    f = wave_xor(crc_mul(f, lane_mul));
    if ((t & 63) == 0) part[t >> 6] = f;
    __syncthreads();
    if (t == 0) {
        uint32_t v = 0u;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) v ^= part[w];
        v = crc_shift(v, (unsigned long long)(a.B - s1), a.pw);
        if (g == 0) v ^= a.affine;
        atomicXor(a.sums + (size_t)i * a.n + a.col0 + c, v);
    }
}

// Byte path: bytes [lo, B) of every block.  seg_bytes = bytes per workgroup, kSumRunBytes consecutive bytes per lane.
template <int MODE>
__global__ void __launch_bounds__(kThreads) crc_sum_byte_kernel(const SumLaunch a) {
    int i, c, g;
    sum_coords(a, i, c, g);
    const uint8_t* p = block_ptr<MODE>(a, i, c);
    const long long b0 = a.lo + (long long)g * a.seg_bytes + (long long)threadIdx.x * kSumRunBytes;
    const long long b1 = min(b0 + kSumRunBytes, a.hi);
    uint32_t v = 0u;
    for (long long o = b0; o < b1; ++o) {
        v ^= p[o];
#pragma unroll
        for (int b = 0; b < 8; ++b) v = crc_mulx(v);
    }
    if (b0 < b1) v = crc_shift(v, (unsigned long long)(a.B - b1), a.pw);
    if (g == 0 && threadIdx.x == 0) v ^= a.affine;
    v = wave_xor(v);
    if ((threadIdx.x & 63) == 0 && v != 0u) atomicXor(a.sums + (size_t)i * a.n + a.col0 + c, v);
}

// One lane per stripe, after every sum of the call is complete (the same stream).
__global__ void __launch_bounds__(kThreads) crc_verify_kernel(const SumVerify v) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= v.S) return;
    unsigned bad = 0u;
    int first = -1;
    for (int j = 0; j < v.n; ++j)
        if (v.sums[(size_t)i * v.n + j] != v.expected[(size_t)i * v.n + j]) {
            if (bad == 0u) first = j;
            ++bad;
        }
    v.bad[i] = bad;
    v.targets[i] = bad > 1u ? v.n : first;
}

// ---------------------------------------------------------------------------------------------
// Dispatch

template <int MODE>
const void* pick_of(bool byte, int scheme) {
    if (byte) return (const void*)crc_sum_byte_kernel<MODE>;
    if (scheme == 0) return (const void*)crc_sum_kernel<MODE, 1>;
    if (scheme == 1) return (const void*)crc_sum_kernel<MODE, kSumCopies>;
    return nullptr;
}

const void* pick(int mode, bool byte, int scheme) {
    if (mode == SUM_MODE_INLINE) return pick_of<SUM_MODE_INLINE>(byte, scheme);
    if (mode == SUM_MODE_STRIDED) return pick_of<SUM_MODE_STRIDED>(byte, scheme);
    return nullptr;
}

LaunchLog<kSumLaunchFields> g_sum_log;  // the record has this library's own fields (sum_kernels.hpp)

}  // namespace

void sum_traffic(long long* launches, long long* bytes) { g_sum_log.traffic(launches, bytes); }

int sum_last_launch(int* v, int cap) { return g_sum_log.last_launch(v, cap); }

hipError_t launch_sum(int mode, int n, const int* src_ids, const uint8_t* const* ptrs, const void* base,
                      long long sstride, long long bstride, long long B, const int* d_stripe_of, int S,
                      unsigned* d_sums, bool vec_ok, long long segment_bytes, int table_scheme, hipStream_t st) {
    if (n < 1 || S < 1 || B < 1 || B >= (1LL << 31) || !d_sums || segment_bytes < 0 ||
        segment_bytes % kSumRowBytes != 0 || table_scheme < -1 || table_scheme > 1)
        return hipErrorInvalidValue;
    const int scheme = table_scheme < 0 ? 0 : table_scheme;  // auto: one copy, the faster one as measured
    if (mode == SUM_MODE_INLINE ? (S != 1 || n > kSumPtrs || !ptrs) : (mode != SUM_MODE_STRIDED || !src_ids || !base))
        return hipErrorInvalidValue;
    // the geometry of both paths, the same for every group of columns; the first group is the widest.  A grid past
    // 2^31 - 1 workgroups is refused here, before anything is zeroed, counted or launched.
    const long long vec_bytes = vec_ok ? (B & ~15LL) : 0;
    const int per = mode == SUM_MODE_INLINE ? kSumPtrs : kSumIds;
    const int groups = (n + per - 1) / per;
    long long seg = 0, vsegs = 0, bpw = 0, bsegs = 0;
    if (vec_bytes > 0) {
        seg = segment_bytes > 0 ? segment_bytes : kSumAutoSegment;
        const long long rows = (vec_bytes + kSumRowBytes - 1) / kSumRowBytes * kSumRowBytes;
        if (seg > rows) seg = rows;
        vsegs = (vec_bytes + seg - 1) / seg;
    }
    if (vec_bytes < B) {
        const long long nbytes = B - vec_bytes;
        bpw = (long long)kSumRunBytes * kThreads;
        if (nbytes < bpw) bpw = (nbytes + kSumRunBytes - 1) / kSumRunBytes * kSumRunBytes;
        bsegs = (nbytes + bpw - 1) / bpw;
    }
    const long long widest = (long long)S * (n < per ? n : per);
    if (widest * vsegs > 0x7fffffffLL || widest * bsegs > 0x7fffffffLL) return hipErrorInvalidConfiguration;

    if (const hipError_t e = hipMemsetAsync(d_sums, 0, (size_t)S * (size_t)n * sizeof(unsigned), st); e != hipSuccess)
        return e;

    SumLaunch a;
    memset(&a, 0, sizeof(a));
    a.base = (const uint8_t*)base;
    a.sstride = sstride;
    a.bstride = bstride;
    a.stripe_of = d_stripe_of;
    a.sums = d_sums;
    a.B = B;
    a.S = S;
    a.n = n;
    for (int j = 0; j < 32; ++j) a.pw[j] = kCrcPowers.p[j];
    const unsigned affine = crc_shift(0xFFFFFFFFu, (unsigned long long)B, kCrcPowers.p) ^ 0xFFFFFFFFu;  // crc32c(0^B)
    g_sum_log.count(groups * ((vec_bytes > 0) + (vec_bytes < B)), (long long)S * n * B);

    for (int col0 = 0; col0 < n; col0 += per) {
        a.col0 = col0;
        a.cols = n - col0 < per ? n - col0 : per;
        for (int c = 0; c < a.cols; ++c) {
            if (mode == SUM_MODE_INLINE) a.src.ptrs[c] = ptrs[col0 + c];
            else a.src.ids[c] = src_ids[col0 + c];
        }
        const long long blocks = (long long)S * a.cols;
        a.affine = affine;
        if (vec_bytes > 0) {
            a.lo = 0;
            a.hi = vec_bytes;
            a.seg_bytes = seg;
            a.segs = (int)vsegs;
            const long long gx = blocks * a.segs;
            g_sum_log.record({0, (int)seg, a.segs, S * n, scheme});
            if (const hipError_t e = launch_kernel(pick(mode, false, scheme), a, dim3((unsigned)gx), st); e != hipSuccess)
                return e;
            a.affine = 0u;
        }
        if (vec_bytes < B) {
            a.lo = vec_bytes;
            a.hi = B;
            a.seg_bytes = bpw;
            a.segs = (int)bsegs;
            const long long gx = blocks * a.segs;
            if (vec_bytes == 0) g_sum_log.record({1, (int)bpw, a.segs, S * n, 0});
            if (const hipError_t e = launch_kernel(pick(mode, true, 0), a, dim3((unsigned)gx), st); e != hipSuccess)
                return e;
        }
    }
    return hipSuccess;
}

hipError_t launch_sum_verify(const SumVerify& v, hipStream_t st) {
    if (v.S < 1 || v.n < 1 || !v.sums || !v.expected || !v.targets || !v.bad) return hipErrorInvalidValue;
    g_sum_log.count(1, 0);
    return launch_kernel((const void*)crc_verify_kernel, v, dim3((unsigned)((v.S + kThreads - 1) / kThreads)), st);
}

}  // namespace ecg
